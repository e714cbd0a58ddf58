"""CPU: the C-ABI library builds, loads and exports every symbol include/mink_hip.h declares, and the Python bindings are what
that header says (signatures, struct layouts, hook types, constants, ABI version)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "mink_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(mink_[a-z0-9_]+)\s*\(", text)))


def test_header_symbols_exported_and_bound():
    from nerf_downstream_amd import _lib

    _lib.build()
    names = _declared()
    assert len(names) >= 20
    assert sorted(_lib.SIGNATURES) == names, set(names) ^ set(_lib.SIGNATURES)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert hasattr(L, n), f"{n} declared in mink_hip.h but not exported"
    handle = _lib.lib()
    assert handle.mink_abi_version() == 4  # 2: every scratch buffer travels with its size; 3: MinkStem.xb (bf16 storage); 4: mink_net_*
    # pure host helpers can run without a GPU
    assert handle.mink_table_capacity(1000) == 2048
    assert handle.mink_conv_plan_ksplit(1_000_000, 27, 64, 0) == 1
    assert handle.mink_conv_plan_ksplit(512, 27, 512, 0) > 1
    assert handle.mink_unique_workspace_bytes(1000) > 5000


def test_argument_validation_without_gpu():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    assert L.mink_coords_make_keys(None, 0, 10, 1, None, None, None) == -1
    assert b"NULL" in L.mink_last_error()
    assert L.mink_kernel_map(None, None, 64, None, 5, None, 28, None, None, None) == -1
    assert L.mink_bn_apply(None, 4, 6, None, None, None, None, None, 0, None, None) == -1
    assert b"multiple of 4" in L.mink_last_error()


def test_one_error_text_serves_every_translation_unit():
    """set_error and the thread-local text behind mink_last_error live in csrc/lib.hip; one refused call into an entry point of
    each file that took over csrc/coords.hip's kernels (coords.hip, kmap.hip, rulebook.hip, plenoxel.hip) leaves ITS message
    there.  Every check comes before the first launch: no GPU."""
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced
    err = L.mink_last_error
    assert L.mink_coords_make_keys(None, 0, 10, 1, None, None, None) == -1
    assert err() == b"make_keys: NULL pointer"
    assert L.mink_kernel_map(None, None, 64, None, 5, None, 28, None, None, None) == -1
    assert err() == b"kernel_map: kernel volume 28 unsupported (1..27)"
    need = L.mink_class_partition_workspace_bytes(1000)
    assert L.mink_class_partition(P, 1000, 2, 128, P, P, need - 1, None) == -1
    assert err() == f"class_partition: workspace of {need - 1} bytes, {need} needed".encode()
    assert L.mink_rulebook(P, 1000, 28, P, P, P, P, 1 << 20, None) == -1
    assert err() == b"rulebook: bad arguments"
    assert L.mink_decode_plenoxel(P, P, P, P, 1, P, P, 10, 4, 4, 0, 1, -1, -1, None, 28, P, P, 27, None) == -1  # ldf < C
    assert err() == b"decode_plenoxel: bad shape"
    assert L.mink_coords_make_keys(None, 2, 10, 1, None, None, None) == -1  # ... and the first file again: the text moved on
    assert err() == b"make_keys: bad arguments (n=10 ts=1 mode=2)"


def test_undersized_workspace_is_refused_before_any_launch():
    """ABI v2: the size of a scratch buffer is an argument, checked against the plan the call is about to launch.  The
    split factors / row splits of a convolution depend on planner state (tuning knobs), so a size cached by the caller
    for another plan used to be written past; now it is MINK_EINVAL.  Dummy non-NULL pointers: the check comes before
    the first launch, so this runs without a GPU."""
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced
    # weight gradient of a mid layer: the plan wants row-split slabs
    n_out, K, cin, cout = 40000, 27, 64, 64
    need = L.mink_conv_wgrad_workspace_bytes(n_out, K, cin, cout)
    assert need > 0
    assert L.mink_conv_wgrad(P, n_out, cin, cin, P, cout, cout, P, n_out, K, P, P, need - 1, None) == -1
    assert b"workspace" in L.mink_last_error() and str(need).encode() in L.mink_last_error()
    # ... and a size that was right for the default plan is too small once a knob asks for more row splits
    old = L.mink_conv_set_stagger((2 << 12) | (200 << 16))  # force G = 3 and 200 row splits (scripts/kbench.py wsweep)
    try:
        assert L.mink_conv_wgrad_workspace_bytes(n_out, K, cin, cout) > need
        assert L.mink_conv_wgrad(P, n_out, cin, cin, P, cout, cout, P, n_out, K, P, P, need, None) == -1
        assert b"row splits of this plan" in L.mink_last_error()
    finally:
        L.mink_conv_set_stagger(old)
    # split-K forward: slabs
    assert L.mink_conv_gather_gemm(P, 512, 64, 64, P, 0, 0, P, 512, 27, None, 0, P, 64, 64, None, 4, P, 4 * 4 * 512 * 64 - 1, None) == -1
    assert b"slabs" in L.mink_last_error()
    # batch norm backward / statistics, coordinate pyramid, class partition
    assert L.mink_bn_bwd(P, P, P, 1000, 64, P, P, P, 1, P, None, P, P, P, L.mink_bn_workspace_bytes(1000, 64) - 1, None) == -1
    assert b"workspace" in L.mink_last_error()
    assert L.mink_bn_stats(P, 1000, 64, 1e-5, 0.1, P, P, None, None, P, 16, None) == -1
    assert L.mink_class_partition(P, 1000, 2, 128, P, P, 8, None) == -1
    assert b"workspace" in L.mink_last_error()


def test_conv_switches_reach_both_halves():
    """The convolution's switches are one object (g_conv, csrc/conv_common.h) written by the setters of csrc/conv.hip and read by the
    planners of both translation units: a bit set through mink_conv_set_stagger must change what wgrad_plan's callers in
    csrc/conv_wgrad.hip answer, and mink_conv_set_math what mink_conv_plan in csrc/conv.hip answers.  Host arithmetic only."""
    from nerf_downstream_amd import _lib

    L = _lib.lib()

    def stem_fused(n):  # the stem shape: wgrad_plan picks G = 9 from 342 row tiles of 128 up
        return L.mink_conv_wgrad_bn_relu_pool_supported(n, 28, 28, n, 27, 64)

    def plans():
        return [L.mink_conv_plan(rows, 27, 64, 64, 0) for rows in (2316, 10840, 20000)]

    try:
        L.mink_conv_set_stagger(0)
        L.mink_conv_set_math(0)
        # weight-gradient side
        assert stem_fused(43649) == 1
        assert stem_fused(43648) == 0
        L.mink_conv_set_stagger(1024)  # bit 10: the tiled weight-gradient kernel for the stem
        assert stem_fused(43649) == 0
        L.mink_conv_set_stagger(0)
        assert stem_fused(43649) == 1
        # forward side
        assert plans() == [14, 7, 6]
        L.mink_conv_set_math(1)
        assert plans() == [14, 6, 3]
        L.mink_conv_set_math(0)
        L.mink_conv_set_stagger(1 << 30)  # bit 30: the mid layers back on the dense kernel
        assert plans() == [14, 6, 3]
        L.mink_conv_set_stagger(0)
        assert plans() == [14, 7, 6]
    finally:
        L.mink_conv_set_stagger(0)
        L.mink_conv_set_math(0)


def test_trunk_branch_policy():
    """Where the native trunk runs its shortcut branch (minkowski/functional.py: trunk_branch_mode): a stream of its own by
    default; under a data-parallel reducer (fork off, branch-on-side on) the weight-gradient stream with fp32 / split-bf16
    math and no branch at all with bf16 math.  Host logic only: the math mode is read through the C ABI, no kernel runs."""
    from nerf_downstream_amd.minkowski import functional as Fn

    old_fork, old_side, old_math = Fn.set_branch_fork(True), Fn.set_trunk_branch_on_side(False), Fn.set_conv_math("fp32")
    try:
        assert Fn.conv_math() == "fp32" and Fn.trunk_branch_mode() == "own"
        Fn.set_branch_fork(False)
        assert Fn.trunk_branch_mode() is None
        Fn.set_trunk_branch_on_side(True)
        assert Fn.trunk_branch_mode() == "side"
        Fn.set_conv_math("bf16x3")
        assert Fn.trunk_branch_mode() == "side"
        Fn.set_conv_math("bf16")
        assert Fn.conv_math() == "bf16" and Fn.trunk_branch_mode() is None
        Fn.set_branch_fork(True)
        assert Fn.trunk_branch_mode() == "own"
    finally:
        Fn.set_branch_fork(old_fork), Fn.set_trunk_branch_on_side(old_side), Fn.set_conv_math(old_math)
    assert Fn.set_conv_storage("bf16") == "fp32" and Fn.set_conv_storage("fp32") == "bf16"
    with pytest.raises(ValueError):
        Fn.set_conv_storage("fp16")


def test_net_sizes_follow_the_documented_arena_layout():
    """mink_net_sizes (host arithmetic only: no GPU): the activation arena of mink_net_forward is, per block and 256-byte
    aligned, [y1 | h1 | y2 | out | (yd | sd)] of n_out x C floats + six C-vectors of statistics; the gradient arena the block's
    mink_block_grad_scratch_floats + its input gradient -- the layout include/mink_hip.h documents and
    nerf_downstream_amd/minkowski/trunk.py::_Saved walks."""
    import ctypes

    from nerf_downstream_amd._lib import BasicBlock, LevelMaps, Net, lib

    L = lib()
    blocks = (BasicBlock * 3)()
    spec = [(64, 64, 2, True), (64, 64, 1, False), (64, 128, 2, True)]  # cin, C, stride, shortcut convolution
    for b, (cin, C, stride, down) in zip(blocks, spec):
        b.conv1.K, b.conv1.cin, b.conv1.cout, b.conv1.stride = 27, cin, C, stride
        b.conv2.K, b.conv2.cin, b.conv2.cout, b.conv2.stride = 27, C, C, 1
        if down:
            b.down.w, b.down.K, b.down.cin, b.down.cout, b.down.stride = 1, 1, cin, C, 2  # (any non-NULL pointer: never dereferenced here)
    net = Net()
    net.blocks, net.n_blocks, net.with_stem = ctypes.cast(blocks, ctypes.POINTER(BasicBlock)), 3, 1
    levels = (LevelMaps * 3)()
    rows = [10840, 2316, 527]
    for lv, n in zip(levels, rows):
        lv.n = n
    a, g, w = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    assert L.mink_net_sizes(ctypes.byref(net), levels, 3, ctypes.byref(a), ctypes.byref(g), ctypes.byref(w)) == 0
    up = lambda v: -(-v // 64) * 64  # noqa: E731
    shapes = [(rows[0], rows[1], 64, 64, True), (rows[1], rows[1], 64, 64, False), (rows[1], rows[2], 64, 128, True)]
    want_a = sum(up((6 if d else 4) * no * C) + up(6 * C) for _, no, _, C, d in shapes)
    want_g = sum(up(L.mink_block_grad_scratch_floats(ni, no, cin, C, int(d))) + up(ni * cin) for ni, no, cin, C, d in shapes)
    assert a.value == want_a and g.value == want_g
    assert w.value == max(L.mink_block_workspace_bytes(ni, no, cin, C) for ni, no, cin, C, _ in shapes)
    # a block that strides past the last level given is refused
    assert L.mink_net_sizes(ctypes.byref(net), levels, 2, ctypes.byref(a), ctypes.byref(g), ctypes.byref(w)) != 0
    assert b"level" in L.mink_last_error()


# ---------------------------------------------------------------- the bindings are read from include/mink_hip.h (_lib.parse_header)
_SNIPPET = """
#ifndef SNIPPET_H
#define SNIPPET_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define X 4u
#define Y (-2) /* a negative code */
enum {
  MINK_T_A = 0,  /* 9 */
  MINK_T_b = 9,  // 3
  MINK_T_PARAMS = 12
};
const char *mink_name(void);
int mink_three(const float *x, /* [n][ld] */ int64_t n,
               uint64_t seed, uint64_t *keys, // one per row
               uint32_t *const *tables, float eps, double scale, uint32_t flags, int mode, int32_t K,
               const uint8_t *arg, void *stream);
typedef struct MinkInner {
  const float *gamma, *beta; /* [C] */
  int32_t K, cin;
  float eps;
} MinkInner;
typedef struct {
  MinkInner conv;
  MinkInner *blocks;
  int32_t offsets[81];
  const int32_t *nbr;
  int64_t n;
  void *compute, *branch;
} MinkOuter;
typedef void (*MinkTHook)(int32_t stage, int32_t backward);
int mink_set_t_hook(MinkTHook hook);
int64_t mink_sizes(const MinkOuter *net, int64_t *act_floats);
#ifdef __cplusplus
}
#endif
#endif /* SNIPPET_H */
"""


def test_reader_on_snippets():
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_uint32, c_uint64, c_void_p

    from nerf_downstream_amd import _lib

    sig, structs, hooks, consts = _lib.parse_header(_SNIPPET)
    assert consts == {"X": 4, "Y": -2, "MINK_T_A": 0, "MINK_T_b": 9, "MINK_T_PARAMS": 12}
    assert sig == {
        "mink_name": (c_char_p, []),
        "mink_three": (c_int, [c_void_p, c_int64, c_uint64, c_void_p, c_void_p, c_float, c_double, c_uint32, c_int, c_int32,
                               c_void_p, c_void_p]),
        "mink_set_t_hook": (c_int, [c_void_p]),
        "mink_sizes": (c_int64, [c_void_p, c_void_p]),
    }
    assert sorted(structs) == ["Inner", "Outer"]
    inner, outer = structs["Inner"], structs["Outer"]
    assert inner.__name__ == "Inner" and issubclass(outer, ctypes.Structure)
    assert inner._fields_ == [("gamma", c_void_p), ("beta", c_void_p), ("K", c_int32), ("cin", c_int32), ("eps", c_float)]
    assert outer._fields_ == [("conv", inner), ("blocks", POINTER(inner)), ("offsets", c_int32 * 81), ("nbr", c_void_p),
                              ("n", c_int64), ("compute", c_void_p), ("branch", c_void_p)]
    assert list(hooks) == ["MinkTHook"]
    assert hooks["MinkTHook"]._restype_ is None and hooks["MinkTHook"]._argtypes_ == (c_int32, c_int32)


@pytest.mark.parametrize("text, names", [
    ("int mink_f(const float *x, size_t n);", "size_t"),  # an unknown scalar type
    ("#define MINK_Z (1 << 3)", "1 << 3"),  # a constant that is an expression
    ("typedef struct { int32_t a : 3; } MinkBits;", "a : 3"),  # a bit-field
    ("int mink_g(int32_t n, void (*)(int32_t));", "mink_g"),  # an unnamed function-pointer parameter
])
def test_reader_raises_on_what_it_does_not_know(text, names):
    from nerf_downstream_amd import _lib

    with pytest.raises(_lib.HeaderError, match=re.escape(names)):
        _lib.parse_header(text)


_STRUCTS = ("KernelMapDesc", "ConvLayer", "NormLayer", "Exec", "Stem", "BasicBlock", "LevelMaps", "Net", "ClassPartitionDesc",
            "TimingEntry", "ConvLaunchInfo")


def test_struct_layout_against_the_c_compiler(tmp_path):
    """sizeof of every struct, offsetof and sizeof of every field, as the host C compiler lays include/mink_hip.h out, against
    the ctypes classes: the numbers come from gcc, not from the reader's reading of the types."""
    import subprocess

    from nerf_downstream_amd import _lib

    assert sorted(_lib.STRUCTS) == sorted(_STRUCTS)
    lines, want = [], []
    for name in _STRUCTS:
        cls = getattr(_lib, name)
        lines.append(f'  printf("%zu\\n", sizeof(Mink{name}));')
        want.append(ctypes.sizeof(cls))
        for field, _ in cls._fields_:
            lines.append(f'  printf("%zu %zu\\n", offsetof(Mink{name}, {field}), sizeof(((Mink{name} *)0)->{field}));')
            want.append((getattr(cls, field).offset, getattr(cls, field).size))
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include "mink_hip.h"\nint main(void) {\n' + "\n".join(lines) + "\n  return 0;\n}\n")
    exe = str(tmp_path / "layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, str(src)])
    out = subprocess.check_output([exe], text=True).splitlines()
    got = [tuple(map(int, row.split())) if " " in row else int(row) for row in out]
    assert len(want) == len(_STRUCTS) + sum(len(getattr(_lib, n)._fields_) for n in _STRUCTS) > 100
    assert got == want


def test_whole_header_is_read():
    from nerf_downstream_amd import _lib

    assert len(_lib.SIGNATURES) >= 141
    for name, (res, args) in _lib.SIGNATURES.items():
        assert res in (ctypes.c_int, ctypes.c_int32, ctypes.c_int64, ctypes.c_char_p), name
        assert isinstance(args, list), name
    assert len(_lib.SIGNATURES["mink_wsconv_fwd"][1]) == 19
    assert _lib.SIGNATURES["mink_set_stage_hook"] == (ctypes.c_int, [ctypes.c_void_p])
    assert _lib.STAGE_HOOK._argtypes_ == (ctypes.c_int32, ctypes.c_int32) and _lib.BLOCK_DONE_HOOK._argtypes_ == (ctypes.c_int32,)
    assert _lib.Net.blocks.size == ctypes.sizeof(ctypes.c_void_p) and dict(_lib.Net._fields_)["blocks"] is ctypes.POINTER(_lib.BasicBlock)
    for family, some in (("MINK_AUG_", ("A", "a", "DROPOUT", "PARAMS", "MAX_CHANNELS")),
                         ("MINK_SEGAUG_", ("A0", "CROP_U", "PARAMS", "MAX_ELASTIC")),
                         ("MINK_COLORAUG_", ("COUNT", "OP_STRIDE", "NORMALIZE")), ("MINK_VOXDS_", ("Q", "VOXEL", "IGNORE", "PARAMS")),
                         ("MINK_WSCONV_", ("CHUNK", "COUT_TILE", "WIDE_ROWS")), ("MINK_FPS_", ("THREADS", "DIST_REG_ROWS", "BAD_START")),
                         ("MINK_STATUS_", ("RANGE", "UNSORTED")), ("MINK_", ("OK", "EINVAL", "ELAUNCH", "ABI_VERSION"))):
        assert set(some) <= set(_lib.constants(family)), family
    assert _lib.CONSTANTS["MINK_EINVAL"] == -1 and _lib.CONSTANTS["MINK_STATUS_NOT_ASCENDING"] == 4
    assert _lib.constants("MINK_AUG_")["a"] == 9 and _lib.constants("MINK_AUG_")["A"] == 0


def test_header_sections_name_the_defining_file():
    """Text only: every prototype of mink_hip.h sits under a `/* ---- title (csrc/a.hip, csrc/b.hip)` line, and one of the files
    that title names defines it -- the entry-point name followed by `(` on an unindented line (a call is indented)."""
    text = open(os.path.join(ROOT, "include", "mink_hip.h")).read()
    titles = [(m.start(), m.group(1).strip(), re.findall(r"\bcsrc/\w+\.hip\b", m.group(1)))
              for m in re.finditer(r"^/\* -{4,}([^\n]*)", text, flags=re.M)]
    code = re.sub(r"/\*.*?\*/", lambda m: " " * len(m.group(0)), text, flags=re.S)  # (offsets kept)
    protos = [(m.start(), m.group(1)) for m in re.finditer(r"\b(mink_[a-z0-9_]+)\s*\(", code)]
    assert len(titles) >= 25 and sorted({n for _, n in protos}) == _declared()
    sources = {}
    for pos, name in protos:
        above = [t for t in titles if t[0] < pos]
        assert above, f"{name} is declared above the first section title"
        _, title, files = above[-1]
        assert files, f"{name}: its section {title!r} names no csrc file"
        for f in files:
            if f not in sources:
                sources[f] = open(os.path.join(ROOT, "nerf_downstream_amd", f)).read()
        defined = [f for f in files if re.search(rf"^[A-Za-z_][\w \*]*?\b{name}\(", sources[f], flags=re.M)]
        assert defined, f"{name} is declared under {title!r} but none of {files} defines it"


def test_library_of_another_abi_is_refused(monkeypatch):
    """lib() on a fresh module state, over a handle whose mink_abi_version answers 3: MinkHipError naming both numbers."""
    from nerf_downstream_amd import _lib

    stale = ctypes.CDLL(_lib.LIB_PATH)  # (a handle object of its own: the attribute set here is not seen by other handles)
    stale.mink_abi_version = ctypes.CFUNCTYPE(ctypes.c_int)(lambda: 3)
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib.ctypes, "CDLL", lambda path: stale)
    with pytest.raises(_lib.MinkHipError, match=r"ABI version 3\b.*declares 4\b.*make -C"):
        _lib.lib()
    assert _lib._lib is None
    monkeypatch.undo()
    assert _lib.lib().mink_abi_version() == 4
