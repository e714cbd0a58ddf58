"""-m gpu: the convolution kernels on both sides of the gates of their 32-bit addressing (tests/big_tables.py builds the tables,
the operands and the float64 reference; tests/test_big_tables_cpu.py holds those to account).

The fast kernels address their operands with 32-bit arithmetic -- buffer descriptors, `__umul24(row, pitch)`, row 0xFFFFFF for
"no neighbour" -- and the planners gate them by size (plan_gather / compact_operands in csrc/conv.hip, wgrad_plan in
csrc/conv_wgrad.hip, mink_stem_conv_bf16s_supported).  tests/test_conv_dispatch_cpu.py checks the gates on the host; here the
kernels RUN at them.  Cases come in pairs, one on each side of a gate, and each asks the library which launch it is about to
make (mink_conv_gather_gemm_launch_info / mink_conv_wgrad_launch_info) and asserts the family and template arguments first.

Large input side: a table of a few thousand rows (probe_table) names rows 0, 1, the rows around bits 22 / 23 / 24 of the index,
the rows on both sides of byte 2^31 and 2^32 of x, the last rows, and a few hundred random ones, in EVERY column, next to
missing neighbours.  Large output side: an x of a thousand rows, a table of -1 with neighbours inside a few row windows
(window_table: the first tile, the tiles where the byte offsets of y / dy and of the table cross 2^31 and 2^32, the ragged last
tile), y pre-filled with NaN: window rows against float64, every other row exactly the bias.

Bounds: none of its own.  fp32 forms: ATOL / RTOL of test_gpu_ops.py.  bf16 and split-bf16 forms: CONV_REL / CONV_MAX of
layerwise.py (the launch-form bounds of the layerwise suites), on operands that are bf16-representable, so that the float64
reference over the same values is what every math mode is asked to compute.  bf16 storage: layerwise.check_bf16_store.  Rows
without a neighbour, pad columns and everything outside a window: exact.  Every launch runs twice, bitwise equal.

Operands are filled on the device in chunks (fill_rows); pad columns of a pitched operand hold NaN; every test frees its
tensors before it returns and prints its peak allocation (run with -s to see the figures)."""
import contextlib
import gc

import pytest
import torch

import big_tables as BT
import layerwise as LW
from helpers import class_perm
from test_gpu_ops import ATOL, RTOL  # the fp32 convolution bounds of test_convolution: no new number here

pytestmark = pytest.mark.gpu

T24 = 1 << 24
B31, B32 = 1 << 31, 1 << 32
N_OUT = 2501      # rows of a probe table: 39 tiles of 64 + 5 rows, 19 tiles of 128 + 69
N_OUT_SK = 12101  # ... where the stream-K plan takes a launch (tests/test_conv_dispatch_cpu.py)
K27 = 27
LIBRARY_KEEPS = 256 << 20


# ------------------------------------------------------------------------------------------------------------ plumbing
def _dev():
    return torch.device("cuda", 0)


def _lib():
    from nerf_downstream_amd import _lib

    return _lib.lib(), _lib.constants("MINK_KERNEL_"), _lib.constants("MINK_EPILOGUE_")


def _stream():
    return torch.cuda.current_stream().cuda_stream


@contextlib.contextmanager
def _knobs(L, stagger=0, math=0, pipeline=0):
    old_math = L.mink_conv_set_math(math)
    old_pipe = L.mink_conv_set_pipeline(pipeline)
    L.mink_conv_set_stagger(stagger)
    try:
        yield
    finally:
        L.mink_conv_set_stagger(0)
        L.mink_conv_set_pipeline(old_pipe)
        L.mink_conv_set_math(old_math)


@pytest.fixture(autouse=True)
def _memory():
    """Peak allocation of the test (the figure of the summary); none of its tensors may stay behind -- LIBRARY_KEEPS allows for
    what torch's generators and its BLAS handle allocate on first use and keep (measured: 76 and 128 MB)."""
    gc.collect()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    yield
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    gc.collect()
    left = torch.cuda.memory_allocated() - before
    torch.cuda.empty_cache()
    print(f"    peak {peak:.2f} GB allocated")
    assert peak <= 16.0, f"{peak:.1f} GB live"
    assert left <= LIBRARY_KEEPS, f"{left} bytes stayed allocated"


def _inst(info, n):
    return (info.kernel,) + tuple(info.targ)[: n - 1]


_WORST = {}


def _judge(tag, got, ref, math=0):
    """`got` against the float64 `ref` under the bound of the form's arithmetic -> worst error / bound (printed, asserted)."""
    assert tuple(got.shape) == tuple(ref.shape), (tag, got.shape, ref.shape)
    if math == 0:
        worst = BT.worst_over_bound(got, ref, ATOL, RTOL)
    else:
        assert torch.isfinite(got).all(), tag
        rel, mx = LW.conv_errors(got, ref)
        worst = max(rel / LW.CONV_REL, mx / LW.CONV_MAX)
    _WORST[tag] = worst
    print(f"    {tag:100s} worst error / bound {worst:.3f}")
    assert worst <= 1.0, (tag, worst)
    return worst


def _probe_case(n_in, ldx, n_out=N_OUT, K=K27, seed=0, esz=4):
    """(table on the device, rows it names, table re-indexed into them, the rows that have no neighbour)."""
    rows = BT.probe_rows(n_in, ldx, esz, seed=seed)
    table = BT.probe_table(n_out, K, rows, 0.3, seed=seed).to(_dev())
    named, local = BT.gathered(table)
    assert named.numel() == len(rows) and int(named[-1]) == n_in - 1
    dead = (table < 0).all(dim=1)
    assert bool(dead.any())
    return table, named, local, dead


def _weights(K, cin, cout, seed, transposed=False):
    """Forward weights [K][cin][cout] (or the [K][cout][cin] block a w_transposed launch reads), bf16-representable."""
    g = torch.Generator(device=_dev()).manual_seed(seed)
    shape = (K, cout, cin) if transposed else (K, cin, cout)
    return (torch.randn(shape, generator=g, device=_dev()) * 0.1).bfloat16().float()


def _small(n, c, seed):
    g = torch.Generator(device=_dev()).manual_seed(seed)
    return torch.randn(n, c, generator=g, device=_dev()).bfloat16().float()


def _gather_gemm(L, x, n_in, w, table, cout, expect, wt=False, flip=False, perm=None, ksplit=1, bias=None, ldy=None, epilogue=None):
    """One mink_conv_gather_gemm launch into a NaN-filled y at pitch ldy, after asserting the instantiation the planner names
    for exactly this call; run twice, bitwise equal; the pad columns of y keep their NaN.  -> y[:, :cout]."""
    cin, ldx = x.shape[1], x.stride(0)
    n_out, K = table.shape
    ldy = ldy or cout + 4
    n_virtual = 0 if perm is None else perm.numel()
    rc, info = LW.ask_gather_launch(L, n_in, ldx, cin, wt, flip, n_out, K, perm is not None, n_virtual, ldy, cout, ksplit, bias=bias is not None)
    assert rc == 0, L.mink_last_error()
    assert _inst(info, len(expect)) == tuple(expect), (_inst(info, 7), expect)
    if epilogue is not None:
        assert info.epilogue == epilogue, (info.epilogue, epilogue)
    assert 1 <= info.slabs <= ksplit
    ws = torch.empty(ksplit * n_out * cout if ksplit > 1 else 4, device=x.device)  # (the call sizes it by the split asked for)
    outs = []
    for _ in range(2):
        y = torch.full((n_out, ldy), float("nan"), device=x.device)
        rc = L.mink_conv_gather_gemm(x.data_ptr(), n_in, ldx, cin, w.data_ptr(), int(wt), int(flip), table.data_ptr(), n_out, K,
                                     None if perm is None else perm.data_ptr(), n_virtual, y.data_ptr(), ldy, cout,
                                     None if bias is None else bias.data_ptr(), ksplit, ws.data_ptr() if ksplit > 1 else None,
                                     4 * ws.numel() if ksplit > 1 else 0, _stream())
        assert rc == 0, L.mink_last_error()
        outs.append(y)
    torch.cuda.synchronize()
    assert torch.equal(outs[0][:, :cout], outs[1][:, :cout]), "two runs differ"
    assert torch.isnan(outs[0][:, cout:]).all(), "a pad column of y was written"
    return outs[0][:, :cout]


def _wgrad(L, x, n_in, dy, table, expect, slabs=None):
    """One mink_conv_wgrad launch, the planner's instantiation asserted first; twice, bitwise equal.  -> dw [K][cin][cout]."""
    cin, ldx, cout, ldy = x.shape[1], x.stride(0), dy.shape[1], dy.stride(0)
    n_out, K = table.shape
    rc, info = LW.ask_wgrad_launch(L, n_in, ldx, cin, ldy, cout, n_out, K)
    assert rc == 0, L.mink_last_error()
    assert _inst(info, len(expect)) == tuple(expect), (_inst(info, 5), expect)
    if slabs is not None:
        assert info.slabs == slabs
    need = L.mink_conv_wgrad_workspace_bytes(n_out, K, cin, cout)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=x.device)
    outs = []
    for _ in range(2):
        dw = torch.full((K, cin, cout), float("nan"), device=x.device)
        rc = L.mink_conv_wgrad(x.data_ptr(), n_in, ldx, cin, dy.data_ptr(), ldy, cout, table.data_ptr(), n_out, K, dw.data_ptr(), ws.data_ptr(),
                               ws.numel(), _stream())
        assert rc == 0, L.mink_last_error()
        outs.append(dw)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1]), "two runs differ"
    return outs[0]


def _check_rows(tag, y, ref, dead, exact, math=0):
    """Rows with a neighbour within the bound, rows without exactly `exact` (the bias, or zero)."""
    _judge(tag, y, ref, math)
    assert torch.equal(y[dead], exact.expand(int(dead.sum()), -1)), f"{tag}: a row without neighbours is not exactly the bias"


# ---------------------------------------------------------------------------------------------- large input side: forward
@pytest.mark.parametrize("n_in", [T24 - 2, T24 - 1, T24 + 5])
def test_stem_forward_on_both_sides_of_the_flat_gate(n_in):
    """cin = 28 at pitch 32 (NaN in the pad columns), cout = 64, with bias.  n_in = 2^24 - 2: the flattened-K path
    gather_gemm2{FLAT = 28}, x two rows under 2^31 bytes, the sentinel row 0xFFFFFF one row behind the last; 2^24 - 1 and
    2^24 + 5: the general gather_gemm2 with 64-bit addresses.  Every math mode (each is an instantiation of its own)."""
    L, kind, _ = _lib()
    cin, cout = 28, 64
    table, named, local, dead = _probe_case(n_in, 32, seed=n_in % 97)
    x = BT.fill_rows(n_in, cin, 32, seed=1, device=_dev(), bf16=True)
    w, bias = _weights(K27, cin, cout, 2), _small(1, cout, 3)[0]
    ref, _ = BT.reference(x[named], local, w=w, bias=bias)
    flat = 28 if n_in < T24 - 1 else 0
    for math in (0, 1, 3):
        with _knobs(L, math=math):
            y = _gather_gemm(L, x, n_in, w, table, cout, (kind["GATHER2"], 0, 0, flat, math), bias=bias)
        _check_rows(f"fwd cin 28 n_in {n_in} gather_gemm2<FLAT={flat}, MATH={math}>", y, ref, dead, bias, math)
    del x, y, table


def test_scalar_forward_past_2_24_rows():
    """cin = 27 (no 16-byte rows): gather_gemm_kernel at n_in = 2^24 + 5, rows beyond 2^24 named in every column."""
    L, kind, _ = _lib()
    n_in, cin, cout = T24 + 5, 27, 64
    table, named, local, dead = _probe_case(n_in, cin, seed=11)
    x = BT.fill_rows(n_in, cin, cin, seed=4, device=_dev(), bf16=True)
    w = _weights(K27, cin, cout, 5)
    ref, _ = BT.reference(x[named], local, w=w)
    y = _gather_gemm(L, x, n_in, w, table, cout, (kind["GATHER_SCALAR"], 0))
    _check_rows("fwd cin 27 n_in 2^24+5 gather_gemm (scalar)", y, ref, dead, torch.zeros(cout, device=_dev()))
    del x, y, table


@pytest.mark.parametrize("n_in", [T24 - 1, T24 + 5])
def test_mid_layer_gathers_on_both_sides_of_the_compact_gate(n_in):
    """cin = cout = 64, forward and both data-gradient forms (w_transposed with flip_k; w_transposed through a class permutation).
    n_in = 2^24 - 1: 4 n_in ldx = 2^32 - 256, the row-compacted kernel (plain, class-permuted, three-stage, stream-K; split
    launches with the reduce epilogue) gathers rows whose 32-bit byte offsets lie between 2^31 and 2^32.  n_in = 2^24 + 5: past
    the gate, the dense gather_gemm2 (un-split and split, staged for the permuted form) gathers rows beyond byte 2^32.  Under
    bf16 / split-bf16 math the stride-1 forms are on the dense kernel on both sides, the permuted data gradient on the
    compact bf16 instantiation below the gate."""
    L, kind, epi = _lib()
    C, G2 = kind["COMPACT"], kind["GATHER2"]
    c = 64
    compact = 4 * n_in * c < B32
    assert compact == (n_in == T24 - 1)
    table, named, local, dead = _probe_case(n_in, c, seed=n_in % 89)
    perm = class_perm(torch.randint(0, 8, (N_OUT,), generator=torch.Generator().manual_seed(6))).to(_dev())
    x = BT.fill_rows(n_in, c, c, seed=7, device=_dev(), bf16=True)
    xs = x[named]
    w, wt = _weights(K27, c, c, 8), _weights(K27, c, c, 9, transposed=True)
    zero = torch.zeros(c, device=_dev())
    refs = {"fwd": BT.reference(xs, local, w=w)[0], "dgrad flip_k": BT.reference(xs, local, w=wt, w_transposed=True, flip_k=True)[0],
            "dgrad class-permuted": BT.reference(xs, local, w=wt, w_transposed=True)[0]}
    forms = {"fwd": dict(w=w), "dgrad flip_k": dict(w=wt, wt=True, flip=True), "dgrad class-permuted": dict(w=wt, wt=True, perm=perm)}

    def run(name, expect, math=0, pipeline=0, stagger=0, ksplit=1, epilogue=None, note=""):
        with _knobs(L, math=math, pipeline=pipeline, stagger=stagger):
            y = _gather_gemm(L, x, n_in, forms[name]["w"], table, c, expect, ksplit=ksplit, epilogue=epilogue,
                             **{k: v for k, v in forms[name].items() if k != "w"})
        _check_rows(f"{name} cin 64 n_in {n_in} {expect} ksplit {ksplit} math {math} {note}", y, refs[name], dead, zero, math)

    plan = L.mink_conv_plan(N_OUT, K27, c, c, 0)
    if compact:
        assert plan >= 3
        for name, t in (("fwd", 0), ("dgrad flip_k", 1)):
            for ks in sorted({3, plan}):
                run(name, (C, t, 0, 0, 0, 0, 0), ksplit=ks, epilogue=epi["SPLITK_REDUCE"])
            run(name, (C, t, 0, 0, 0, 1, 0), pipeline=1, ksplit=3, note="three-stage")
        for ks in (1, 2):
            run("dgrad class-permuted", (C, 1, 1, 0, 0, 0, 0), ksplit=ks, epilogue=epi["NONE"] if ks == 1 else epi["SPLITK_REDUCE"])
        run("dgrad class-permuted", (C, 1, 1, 0, 0, 1, 0), pipeline=2, note="three-stage")
        run("dgrad class-permuted", (C, 1, 1, 0, 1, 0, 0), math=1, note="bf16")
        # the dense kernel at the same size (set_stagger bit 30 / 31: the A/B switches): rows between byte 2^31 and 2^32
        run("fwd", (G2, 0, 0, 0, 0), stagger=1 << 30, note="dense by switch")
        run("dgrad class-permuted", (G2, 1, 1, 0, 0), stagger=-(1 << 31), note="staged by switch")
    else:
        for math in (0, 1, 3):
            run("fwd", (G2, 0, 0, 0, math), math=math)
            run("fwd", (G2, 0, 0, 0, math), math=math, ksplit=3, epilogue=epi["SPLITK_REDUCE"])
            run("dgrad flip_k", (G2, 1, 0, 0, math), math=math)
            run("dgrad class-permuted", (G2, 1, 1, 0, math), math=math)
    if compact:
        for math in (1, 3):  # reduced math keeps the stride-1 mid layers on the dense kernel, below the gate too
            run("fwd", (G2, 0, 0, 0, math), math=math)
            run("dgrad flip_k", (G2, 1, 0, 0, math), math=math, ksplit=3, epilogue=epi["SPLITK_REDUCE"])
    del table, named, local, dead, refs
    # stream-K needs runs of five offset-tiles: a table of 12,101 rows (ks = 7, as the dispatch test asks for it)
    if compact:
        table, named, local, dead = _probe_case(n_in, c, n_out=N_OUT_SK, seed=13)
        xs = x[named]
        for name, t, kw in (("fwd", 0, dict(w=w)), ("dgrad flip_k", 1, dict(w=wt, wt=True, flip=True))):
            ref = BT.reference(xs, local, w=kw["w"], w_transposed=bool(t), flip_k=bool(t))[0]
            with _knobs(L, pipeline=8):
                y = _gather_gemm(L, x, n_in, kw["w"], table, c, (C, t, 0, 0, 0, 0, 1), ksplit=7, epilogue=epi["SPLITK_REDUCE"],
                                 **{k: v for k, v in kw.items() if k != "w"})
            _check_rows(f"{name} cin 64 n_in {n_in} compact_gemm stream-K ksplit 7", y, ref, dead, zero)
        del table, named, local, dead, ref
    del x, xs


# --------------------------------------------------------------------------------------- large input side: weight gradient
FORCED = {1: (1 | (2 << 4)), 3: (2 | (2 << 4)), 9: (3 | (2 << 4))}  # set_stagger bits 12..: G and two row splits (the dispatch test's)

WGRAD_CASES = [
    # cin, ldx, n_in, BUF, what the case is
    (20, 20, T24 - 1, 1, "the last n_in the 24-bit row multiply takes"),
    (20, 20, T24, 0, "2^24 rows"),
    (20, 20, T24 + 5, 0, "past 2^24 rows"),
    (20, 36, 15_000_000, 0, "pitched x of 2.16e9 bytes, n_in < 2^24"),
    (96, 96, 5_592_404, 1, "the no-neighbour offset (2^31 - 384) directly behind the last row"),
    (96, 96, 5_592_405, 0, "x of 2^31 - 128 bytes: the wrapped no-neighbour offset would lie inside it"),
    (96, 96, T24 + 5, 0, "x of 6.4e9 bytes"),
    (64, 68, 986_894, 1, "ldx = 68: the no-neighbour offset wraps to 2^28 - 272, still at the end of x"),
    (64, 68, 1_200_000, 0, "ldx = 68, x of 3.3e8 bytes: the wrapped offset would lie inside it"),
]


@pytest.mark.parametrize("cin,ldx,n_in,buf,what", WGRAD_CASES, ids=[f"cin{c}-ld{l}-n{n}" for c, l, n, _, _ in WGRAD_CASES])
def test_tiled_weight_gradient_on_both_sides_of_the_buffer_gate(cin, ldx, n_in, buf, what):
    """wgrad_kernel{G, NARROW, VEC, BUF} at cout = 64 under the three offset groupings (forced, two row splits, slab reduce):
    BUF = 1 reads x, dy and the table through 32-bit buffer offsets with `__umul24(row, 4 ldx)` and row 0xFFFFFF for the padding
    pairs of a tile, BUF = 0 through 64-bit addresses.  The padding pairs multiply dY row 0 by what the no-neighbour offset reads:
    it must read zeros, i.e. lie beyond x -- for ldx > 64 the offset is the WRAPPED product (low 32 bits), which the gate has to
    compare with the size of x."""
    L, kind, epi = _lib()
    cout = 64
    table, named, local, dead = _probe_case(n_in, ldx, seed=(cin + n_in) % 83)
    x = BT.fill_rows(n_in, cin, ldx, seed=21, device=_dev(), bf16=True)
    dy = BT.fill_rows(N_OUT, cout, cout + 4, seed=22, device=_dev(), bf16=True)
    _, ref = BT.reference(x[named], local, dy=dy)
    for G, code in FORCED.items():
        with _knobs(L, stagger=(code << 12) | (1 << 10)):
            dw = _wgrad(L, x, n_in, dy, table, (kind["WGRAD"], G, int(cin <= 32), 1, buf), slabs=2)
        _judge(f"wgrad cin {cin} ldx {ldx} n_in {n_in} wgrad_kernel<G={G}, BUF={buf}> ({what})", dw, ref)
    del x, dy, dw, table


@pytest.mark.parametrize("n_in,w16", [(B31 // 256 - 1, True), (B31 // 256, False)])
def test_bf16_tiled_weight_gradient_just_under_its_gate(n_in, w16):
    """wgrad16_kernel (bf16 math, cin = cout = 64) exists only with buffer offsets: x of 2^31 - 256 bytes is the largest it takes,
    one row more falls to the exact-fp32 wgrad_kernel{BUF = 0}."""
    L, kind, _ = _lib()
    c = 64
    table, named, local, dead = _probe_case(n_in, c, seed=31)
    x = BT.fill_rows(n_in, c, c, seed=32, device=_dev(), bf16=True)
    dy = BT.fill_rows(N_OUT, c, c, seed=33, device=_dev(), bf16=True)
    _, ref = BT.reference(x[named], local, dy=dy)
    for G, code in ((1, 1 | (2 << 4)), (3, 2 | (2 << 4))):
        with _knobs(L, math=1, stagger=code << 12):
            dw = _wgrad(L, x, n_in, dy, table, (kind["WGRAD16"], G) if w16 else (kind["WGRAD"], G, 0, 1, 0), slabs=2)
        _judge(f"wgrad cin 64 n_in {n_in} {'wgrad16' if w16 else 'wgrad'}_kernel<G={G}> under bf16 math", dw, ref, math=1 if w16 else 0)
    del x, dy, dw, table


@pytest.mark.parametrize("n_in", [T24 - 1, T24])
def test_streaming_stem_weight_gradient_at_the_largest_input_it_admits(n_in):
    """The stem shape (cin = 28 at pitch 32, cout = 64) one row over the streaming threshold: n_in = 2^24 - 1 is the largest
    input stream_ok admits (fp32: wgrad_stream_kernel{FLAT}; bf16 math: wgrad_stream_bf16_kernel), 2^24 is tiled.  The fused
    entry answers _supported() by the same plan."""
    L, kind, _ = _lib()
    cin, cout, n_out = 28, 64, 43649
    streaming = n_in < T24
    table, named, local, dead = _probe_case(n_in, 32, n_out=n_out, seed=41)
    x = BT.fill_rows(n_in, cin, 32, seed=42, device=_dev(), bf16=True)
    dy = BT.fill_rows(n_out, cout, cout, seed=43, device=_dev(), bf16=True)
    _, ref = BT.reference(x[named], local, dy=dy)
    assert L.mink_conv_wgrad_bn_relu_pool_supported(n_in, 32, cin, n_out, K27, cout) == int(streaming)
    dw = _wgrad(L, x, n_in, dy, table, (kind["WGRAD_STREAM"], 4, 0, 1) if streaming else (kind["WGRAD"], 9, 1, 1, 0))
    _judge(f"wgrad stem n_in {n_in} {'wgrad_stream_kernel<FLAT>' if streaming else 'wgrad_kernel<G=9, BUF=0>'}", dw, ref)
    with _knobs(L, math=1):
        dw = _wgrad(L, x, n_in, dy, table, (kind["WGRAD_STREAM_BF16"], 0, 0) if streaming else (kind["WGRAD"], 9, 1, 1, 0))
    _judge(f"wgrad stem n_in {n_in} bf16 math {'wgrad_stream_bf16_kernel' if streaming else 'wgrad_kernel<G=9, BUF=0>'}", dw, ref,
           math=1 if streaming else 0)
    # the fused entry (dY recomputed from y, the pooled gradient and the batch statistics inside the operand load)
    n_pool = 5501
    rc, info = LW.ask_wgrad_launch(L, n_in, 32, cin, cout, cout, n_out, K27, fuse=1, n_pool=n_pool)
    if not streaming:
        assert rc == -1 and b"not supported by the streaming kernel" in L.mink_last_error()
    else:
        assert rc == 0 and _inst(info, 4) == (kind["WGRAD_STREAM"], 4, 1, 1), _inst(info, 5)
        g = torch.Generator(device=_dev()).manual_seed(44)
        y, gp = _small(n_out, cout, 45), _small(n_pool, cout, 46)
        i2o = torch.randint(0, n_pool, (n_out,), generator=g, device=_dev(), dtype=torch.int32)
        mean, beta, dga, dbe = (_small(1, cout, 47 + i)[0] * 0.3 for i in range(4))
        invstd, gamma = (1.0 + 0.1 * _small(1, cout, 51 + i)[0] for i in range(2))
        dy_f = LW.stem_wgrad_operand(gp, y, mean, invstd, gamma, beta, dga, dbe, i2o, n_out)
        # the fp32 bound is stated for sums of products of O(1) values: gamma * invstd ~ 1 keeps the recomputed dY (the masked pooled
        # gradient, scaled by it) at the scale of the dY the un-fused cases above draw
        assert 0.3 < float(dy_f.std()) <= 1.1, float(dy_f.std())
        _, ref_f = BT.reference(x[named], local, dy=dy_f)
        need = L.mink_conv_wgrad_workspace_bytes(n_out, K27, cin, cout)
        ws = torch.empty(max(need, 256), dtype=torch.uint8, device=_dev())
        outs = []
        for _ in range(2):
            dwf = torch.full((K27, cin, cout), float("nan"), device=_dev())
            rc = L.mink_conv_wgrad_bn_relu_pool(x.data_ptr(), n_in, 32, cin, y.data_ptr(), cout, gp.data_ptr(), n_pool, i2o.data_ptr(), mean.data_ptr(),
                                                invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), dga.data_ptr(), dbe.data_ptr(), table.data_ptr(),
                                                n_out, K27, dwf.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
            assert rc == 0, L.mink_last_error()
            outs.append(dwf)
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1])
        _judge(f"fused wgrad_bn_relu_pool stem n_in {n_in} wgrad_stream_kernel<FUSE, FLAT>", outs[0], ref_f)
        del y, gp, i2o, dy_f, outs, dwf, ws
    del x, dy, dw, table


def test_bf16_storage_stem_convolution_at_the_largest_input_it_supports():
    """mink_stem_conv_bf16s at n_in = 2^24 - 2 (xb [n][32] bf16, 64 bytes a row: the last row ends at 2^30 - 128); 2^24 - 1 rows
    are not supported."""
    L, _, _ = _lib()
    n_in, cin, cout = T24 - 2, 28, 64
    assert L.mink_stem_conv_bf16s_supported(n_in, N_OUT, K27, cin, cout) == 1
    assert L.mink_stem_conv_bf16s_supported(T24 - 1, N_OUT, K27, cin, cout) == 0
    assert L.mink_stem_conv_bf16s_supported(n_in, (B31 // 108) + 1, K27, cin, cout) == 0 and L.mink_stem_conv_bf16s_supported(n_in, B31 // 108, K27, cin, cout) == 1
    table, named, local, dead = _probe_case(n_in, 32, seed=51, esz=2)
    xb = torch.zeros(n_in, 32, dtype=torch.bfloat16, device=_dev())
    g = torch.Generator(device=_dev()).manual_seed(52)
    for a in range(0, n_in, 1 << 21):
        b = min(n_in, a + (1 << 21))
        xb[a:b, :cin] = torch.randn(b - a, cin, generator=g, device=_dev()).bfloat16()
    w = _weights(K27, cin, cout, 53)
    ref, _ = BT.reference(xb[named][:, :cin].float(), local, w=w)
    rows = L.mink_stem_conv_bf16s_stats_rows()
    outs = []
    for _ in range(2):
        yb = torch.full((N_OUT, cout), float("nan"), dtype=torch.bfloat16, device=_dev())
        stats = torch.zeros(rows, 2, cout, dtype=torch.float64, device=_dev())
        rc = L.mink_stem_conv_bf16s(xb.data_ptr(), n_in, w.data_ptr(), cin, table.data_ptr(), N_OUT, K27, yb.data_ptr(), cout, stats.data_ptr(),
                                    rows, _stream())
        assert rc == 0, L.mink_last_error()
        outs.append((yb, stats))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    yb, stats = outs[0]
    rec = LW.check_bf16_store("stem", "bf16s n_in 2^24-2", yb.float(), ref)[0]
    print("    " + rec.line())
    _WORST["stem_conv_bf16s n_in 2^24-2"] = rec.err / rec.bound
    assert rec.ok, rec.line()
    assert torch.equal(yb[dead].float(), torch.zeros(int(dead.sum()), cout, device=_dev()))
    assert torch.isfinite(stats).all()  # (the statistics partials are held to their bound by tests/test_gpu_ops.py; here: addressing)
    del xb, yb, stats, outs, table


# ------------------------------------------------------------------- large input side: the families with 64-bit addressing only
def test_big_kernel_volume_convolution_with_x_past_2_32_bytes():
    """mink_conv_bigk_gather_gemm / _wgrad (K = 125), cin = cout = 64, n_in = 2^24 + 5: probes beyond byte 2^32 in every column."""
    L, _, _ = _lib()
    n_in, c, K = T24 + 5, 64, 125
    table, named, local, dead = _probe_case(n_in, c, K=K, seed=61)
    x = BT.fill_rows(n_in, c, c, seed=62, device=_dev(), bf16=True)
    dy = BT.fill_rows(N_OUT, c, c + 4, seed=63, device=_dev(), bf16=True)
    w, bias = _weights(K, c, c, 64), _small(1, c, 65)[0]
    ref_y, ref_dw = BT.reference(x[named], local, w=w, dy=dy, bias=bias)
    need = L.mink_conv_bigk_wgrad_workspace_bytes(N_OUT, K, c, c)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=_dev())
    outs = []
    for _ in range(2):
        y = torch.full((N_OUT, c + 4), float("nan"), device=_dev())
        dw = torch.full((K, c, c), float("nan"), device=_dev())
        assert L.mink_conv_bigk_gather_gemm(x.data_ptr(), n_in, c, c, w.data_ptr(), 0, 0, table.data_ptr(), N_OUT, K, y.data_ptr(), c + 4, c,
                                            bias.data_ptr(), _stream()) == 0, L.mink_last_error()
        assert L.mink_conv_bigk_wgrad(x.data_ptr(), n_in, c, c, dy.data_ptr(), c + 4, c, table.data_ptr(), N_OUT, K, dw.data_ptr(), ws.data_ptr(),
                                      ws.numel(), _stream()) == 0, L.mink_last_error()
        outs.append((y, dw))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0][:, :c], outs[1][0][:, :c]) and torch.equal(outs[0][1], outs[1][1])
    y, dw = outs[0]
    assert torch.isnan(y[:, c:]).all()
    _check_rows("bigk fwd K 125 n_in 2^24+5", y[:, :c], ref_y, dead, bias)
    _judge("bigk wgrad K 125 n_in 2^24+5", dw, ref_dw)
    del x, dy, y, dw, outs, table


def test_grouped_convolution_with_x_past_2_32_bytes():
    """mink_gconv_fwd / _wgrad, two groups of 32 -> 32 channels (the matrix-core kernels), n_in = 2^24 + 5."""
    L, _, _ = _lib()
    n_in, G, cg = T24 + 5, 2, 32
    c = G * cg
    table, named, local, dead = _probe_case(n_in, c, seed=71)
    x = BT.fill_rows(n_in, c, c, seed=72, device=_dev(), bf16=True)
    dy = BT.fill_rows(N_OUT, c, c, seed=73, device=_dev(), bf16=True)
    g = torch.Generator(device=_dev()).manual_seed(74)
    w = (torch.randn(K27, G, cg, cg, generator=g, device=_dev()) * 0.1).bfloat16().float()
    xs = x[named]
    parts = [BT.reference(xs[:, i * cg:(i + 1) * cg], local, w=w[:, i], dy=dy[:, i * cg:(i + 1) * cg]) for i in range(G)]
    ref_y = torch.cat([p[0] for p in parts], dim=1)
    ref_dw = torch.stack([p[1] for p in parts], dim=1)
    need = L.mink_gconv_wgrad_workspace_bytes(N_OUT, K27, G, cg, cg)
    ws = torch.empty(max(need, 256), dtype=torch.uint8, device=_dev())
    outs = []
    for _ in range(2):
        y = torch.full((N_OUT, c), float("nan"), device=_dev())
        dw = torch.full((K27, G, cg, cg), float("nan"), device=_dev())
        assert L.mink_gconv_fwd(x.data_ptr(), n_in, c, w.data_ptr(), 0, 0, table.data_ptr(), N_OUT, K27, G, cg, cg, y.data_ptr(), c, _stream()) == 0, \
            L.mink_last_error()
        assert L.mink_gconv_wgrad(x.data_ptr(), n_in, c, dy.data_ptr(), c, table.data_ptr(), N_OUT, K27, G, cg, cg, dw.data_ptr(), ws.data_ptr(),
                                  ws.numel(), _stream()) == 0, L.mink_last_error()
        outs.append((y, dw))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    y, dw = outs[0]
    _check_rows("gconv fwd G 2 x 32 n_in 2^24+5", y, ref_y, dead, torch.zeros(c, device=_dev()))
    _judge("gconv wgrad G 2 x 32 n_in 2^24+5", dw, ref_dw)
    del x, dy, y, dw, outs, table, xs


def test_weight_sparse_convolution_with_x_past_2_32_bytes():
    """mink_wsconv_fwd, a kernel pruned to a tenth of its weights (one offset pruned away whole), n_in = 2^24 + 5 rows of 64."""
    from nerf_downstream_amd.minkowski.wsconv import pack_csr, wsconv_forward

    n_in, c = T24 + 5, 64
    table, named, local, dead = _probe_case(n_in, c, seed=75)
    x = BT.fill_rows(n_in, c, c, seed=76, device=_dev(), bf16=True)
    g = torch.Generator(device=_dev()).manual_seed(77)
    w = _weights(K27, c, c, 78) * (torch.rand(K27, c, c, generator=g, device=_dev()) < 0.1)
    w[5] = 0
    bias = _small(1, c, 79)[0]
    packed = pack_csr(w)
    assert len(packed.valid_kernel) == K27 - 1 and 0.05 < packed.density < 0.15
    ref, _ = BT.reference(x[named], local, w=w, bias=bias)
    y = wsconv_forward(x, packed, table, N_OUT, bias=bias)
    assert torch.equal(y, wsconv_forward(x, packed, table, N_OUT, bias=bias))
    _check_rows("wsconv fwd density 0.1 n_in 2^24+5", y, ref, dead, bias)
    del x, y, table, packed


def test_dense_gemm_and_row_scatter_past_2_32_bytes():
    """mink_dense_xwt and mink_rows_scatter_add with n = 2^24 + 5 rows of 64 floats: x, y, src and dst all pass 2^32 bytes.  The
    rows at both ends and on both sides of byte 2^31 and 2^32 against float64; ALL rows against torch on the device (fp32 GEMM
    within the fp32 bound; the scatter exactly, rows it does not reach untouched)."""
    L, _, _ = _lib()
    n, c = T24 + 5, 64
    dev = _dev()
    x = BT.fill_rows(n, c, c, seed=81, device=dev, bf16=True)
    w = _small(c, c, 82) * 0.1
    edge = torch.tensor(sorted({0, 1, n - 2, n - 1, *BT.crossing_rows(4 * c, n)}), device=dev)
    assert {(1 << 23) - 1, 1 << 23, T24 - 1, T24} <= set(edge.tolist())
    outs = []
    for _ in range(2):
        y = torch.full((n, c), float("nan"), device=dev)
        assert L.mink_dense_xwt(x.data_ptr(), w.data_ptr(), n, c, c, y.data_ptr(), _stream()) == 0, L.mink_last_error()
        outs.append(y)
    torch.cuda.synchronize()
    assert torch.equal(outs[0], outs[1])
    y = outs[0]
    del outs
    _judge("dense_xwt n 2^24+5, edge rows", y[edge], x[edge].double() @ w.double().t())
    worst = 0.0
    for a in range(0, n, 1 << 21):
        b = min(n, a + (1 << 21))
        worst = max(worst, BT.worst_over_bound(y[a:b], x[a:b] @ w.t(), ATOL, RTOL))
    print(f"    dense_xwt n 2^24+5, all rows against the fp32 GEMM of torch: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    # scatter: dst[idx[r]] += src[r]; idx = the reversal with every third row skipped, so both ends of src meet both ends of dst
    r = torch.arange(n, device=dev)
    idx = torch.where(r % 3 == 1, torch.full_like(r, -1), n - 1 - r).to(torch.int32)
    dst = y  # (any values: reuse the 4.3 GB)
    pick = torch.tensor(sorted({int(v) for e in edge.tolist() for v in (e, n - 1 - e)}), device=dev)
    before_pick = dst[pick].double()
    assert L.mink_rows_scatter_add(x.data_ptr(), idx.data_ptr(), n, c, dst.data_ptr(), _stream()) == 0, L.mink_last_error()
    torch.cuda.synchronize()
    src_of = n - 1 - pick  # the src row that lands on dst row `pick`
    hit = (src_of % 3 != 1)
    want = before_pick + x[src_of].double() * hit[:, None]
    assert torch.equal(dst[pick].double(), want.float().double()), "rows_scatter_add: an edge row differs (one fp32 add per element)"
    assert bool(hit.any()) and bool((~hit).any())
    # all rows: undo the scatter with torch and compare with the GEMM output it started from (exact up to one rounding per add)
    worst = 0.0
    for a in range(0, n, 1 << 21):
        b = min(n, a + (1 << 21))
        rows = torch.arange(a, b, device=dev)
        s = n - 1 - rows
        add = torch.where((s % 3 != 1)[:, None], x[s], torch.zeros((), device=dev))
        worst = max(worst, BT.worst_over_bound(dst[a:b], (x[a:b] @ w.t()) + add, ATOL, RTOL))
    print(f"    rows_scatter_add n 2^24+5, all rows: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    del x, y, dst, idx, r


# ----------------------------------------------------------------------------------------------------- large output side
def _window_case(n_out, K, n_in, ldy, seed):
    wins = BT.tile_windows(n_out, (4 * ldy, 4 * K), tile=128)
    table = BT.window_table(n_out, K, n_in, wins, seed=seed, device=_dev())
    rows = BT.window_rows(wins, device=_dev())
    return wins, table, rows


def _outside_is_exactly(y, rows, value, chunk=1 << 21):
    """Every row of y outside `rows` equals `value` bit for bit (on the device, in chunks)."""
    n = y.shape[0]
    inside = torch.zeros(n, dtype=torch.bool, device=y.device)
    inside[rows] = True
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        ok = (y[a:b] == value).all(dim=1) | inside[a:b]
        if not bool(ok.all()):
            bad = int(torch.nonzero(~ok)[0]) + a
            raise AssertionError(f"row {bad} outside every window is not exactly the bias: {y[bad, :4].tolist()}")


LARGE_OUT = [
    # cin, cout, n_out, flat, what
    (28, 64, T24 + 200, 28, "y crosses 2^31 and 2^32 bytes; flat stem path"),
    (64, 64, T24 + 200, 0, "y crosses 2^31 and 2^32 bytes; past the slab budget of the compacted kernel: dense, un-split"),
    (28, 16, B31 // 108 + 300, 28, "table crosses 2^31 bytes (row 19,884,107); flat stem path, offsets up to 2^32"),
    (28, 16, B32 // 108 + 300, 0, "table crosses 2^32 bytes (row 39,768,215): past the flat path's descriptor, general path"),
]


@pytest.mark.parametrize("cin,cout,n_out,flat,what", LARGE_OUT, ids=[f"cin{a}-cout{b}-n{n}" for a, b, n, _, _ in LARGE_OUT])
def test_unsplit_forward_and_weight_gradient_with_many_output_rows(cin, cout, n_out, flat, what):
    """Un-split forward with bias into a NaN-filled y, then the weight gradient with the same table (dy zero outside the
    windows).  The flat path reads the table through a 32-bit descriptor: 4 n_out K must stay below 2^32, which n_out K < 2^31
    does not give -- the last case is past that and must take the general path."""
    L, kind, epi = _lib()
    n_in, ldx = 1000, 32 if cin == 28 else cin
    assert n_out * K27 < B31 and n_out % 128
    wins, table, rows = _window_case(n_out, K27, n_in, cout, seed=n_out % 79)
    crossed = [lim for lim in (B31, B32) for pitch in (4 * cout, 4 * K27) if pitch * n_out > lim]
    assert crossed and len(wins) >= 3, (wins, crossed)  # first tile, last tile, and at least one tile at a crossing
    x = BT.fill_rows(n_in, cin, ldx, seed=91, device=_dev(), bf16=True)
    w, bias = _weights(K27, cin, cout, 92), _small(1, cout, 93)[0]
    sub = table[rows]
    ref, _ = BT.reference(x, sub.long(), w=w, bias=bias)
    y = _gather_gemm(L, x, n_in, w, table, cout, (kind["GATHER2"], 0, 0, flat, 0), bias=bias, ldy=cout, epilogue=epi["NONE"])
    tag = f"fwd cin {cin} cout {cout} n_out {n_out} gather_gemm2<FLAT={flat}>"
    _check_rows(tag + " window rows", y[rows], ref, (sub < 0).all(dim=1), bias)
    _outside_is_exactly(y, rows, bias)
    del y
    # weight gradient: dy zero outside the windows, so float64 needs the window rows alone
    dy = torch.zeros(n_out, cout, device=_dev())
    dyw = _small(rows.numel(), cout, 94)
    dy[rows] = dyw
    _, ref_dw = BT.reference(x, sub.long(), dy=dyw)
    rc, info = LW.ask_wgrad_launch(L, n_in, ldx, cin, cout, cout, n_out, K27)
    assert rc == 0
    buf = int(4 * n_out * cout < B31 and 4 * n_out * K27 < B31)
    stream = cin == 28 and buf  # (stream_ok asks the same of dy and the table)
    expect = (kind["WGRAD_STREAM"], 4, 0, 1) if stream else (kind["WGRAD"], 9, int(cin <= 32), 1, buf)
    dw = _wgrad(L, x, n_in, dy, table, expect)
    _judge(f"wgrad cin {cin} cout {cout} n_out {n_out} {expect}", dw, ref_dw)
    del x, dy, dw, table, rows, sub


WGRAD_OUT = [
    # cin, cout, n_out, BUF / streaming, what
    (64, 64, (1 << 23) - 100, 1, "dy of 2^31 - 25,600 bytes"),
    (64, 64, (1 << 23) + 100, 0, "dy past 2^31 bytes"),
    (64, 16, B31 // 108 - 107, 1, "table of 2^31 - 11,600 bytes"),
    (64, 16, B31 // 108 + 300, 0, "table past 2^31 bytes"),
    (28, 16, B31 // 108 - 107, 1, "stem shape, table just under 2^31 bytes: the largest n_out the streaming kernel admits"),
]


@pytest.mark.parametrize("cin,cout,n_out,buf,what", WGRAD_OUT, ids=[f"cin{a}-cout{b}-n{n}" for a, b, n, _, _ in WGRAD_OUT])
def test_weight_gradient_on_both_sides_of_the_dy_and_table_byte_gates(cin, cout, n_out, buf, what):
    """The db / nb < 2^31 parts of buf_ok (and of stream_ok): wgrad_kernel{BUF} at cin = 64, the streaming kernel at the stem
    shape, with the last tile's dy and table rows right under, or past, byte 2^31."""
    L, kind, _ = _lib()
    n_in, ldx = 1000, 32 if cin == 28 else cin
    assert n_out % 128 and buf == int(4 * n_out * cout < B31 and 4 * n_out * K27 < B31)
    wins, table, rows = _window_case(n_out, K27, n_in, cout, seed=n_out % 73)
    x = BT.fill_rows(n_in, cin, ldx, seed=95, device=_dev(), bf16=True)
    dy = torch.zeros(n_out, cout, device=_dev())
    dyw = _small(rows.numel(), cout, 96)
    dy[rows] = dyw
    _, ref_dw = BT.reference(x, table[rows].long(), dy=dyw)
    expect = (kind["WGRAD_STREAM"], 4, 0, 1) if cin == 28 and buf else (kind["WGRAD"], 9, int(cin <= 32), 1, buf)
    dw = _wgrad(L, x, n_in, dy, table, expect)
    _judge(f"wgrad cin {cin} cout {cout} n_out {n_out} {expect} ({what})", dw, ref_dw)
    del x, dy, dw, table, rows


# ------------------------------------------------------------------------------------------------------------- refusals
def test_tables_of_2_31_entries_are_refused_before_any_launch():
    """n_out K = 2^31 (K = 8, n_out = 2^28) and the first n_out past it for K = 125: refused by the scalars, outputs untouched.
    The launch query, which shares the refusals with the call and launches nothing, is asked first."""
    L, _, _ = _lib()
    dev = _dev()
    n_out = 1 << 28
    rc, _ = LW.ask_gather_launch(L, 1000, 64, 64, False, False, n_out, 8, False, 0, 64, 64, 1)
    assert rc == -1 and b"table too large" in L.mink_last_error()
    rc, _ = LW.ask_gather_launch(L, 1000, 64, 64, False, False, n_out - 1, 8, False, 0, 64, 64, 1)
    assert rc == 0  # one row fewer is planned
    x, w = _small(1000, 64, 1), _weights(8, 64, 64, 2)
    nbr = torch.full((64, 8), -1, dtype=torch.int32, device=dev)
    y = torch.full((64, 64), float("nan"), device=dev)
    rc = L.mink_conv_gather_gemm(x.data_ptr(), 1000, 64, 64, w.data_ptr(), 0, 0, nbr.data_ptr(), n_out, 8, None, 0, y.data_ptr(), 64, 64, None, 1,
                                 None, 0, _stream())
    assert rc == -1 and b"table too large" in L.mink_last_error()
    n_big = -(-B31 // 125)
    assert (n_big - 1) * 125 < B31 <= n_big * 125
    wb = _weights(125, 64, 64, 3)
    nbr_b = torch.full((64, 125), -1, dtype=torch.int32, device=dev)
    rc = L.mink_conv_bigk_gather_gemm(x.data_ptr(), 1000, 64, 64, wb.data_ptr(), 0, 0, nbr_b.data_ptr(), n_big, 125, y.data_ptr(), 64, 64, None, _stream())
    assert rc == -1 and b"overflows int32 indexing" in L.mink_last_error()
    dw = torch.full((125, 64, 64), float("nan"), device=dev)
    ws = torch.empty(256, dtype=torch.uint8, device=dev)
    rc = L.mink_conv_bigk_wgrad(x.data_ptr(), 1000, 64, 64, y.data_ptr(), 64, 64, nbr_b.data_ptr(), n_big, 125, dw.data_ptr(), ws.data_ptr(), 256, _stream())
    assert rc == -1 and b"overflows int32 indexing" in L.mink_last_error()
    coords = torch.zeros(64, 4, dtype=torch.int32, device=dev)
    rc = L.mink_kernel_map_cube(coords.data_ptr(), 64, coords.data_ptr(), n_big, 5, 1, nbr_b.data_ptr(), None, ws.data_ptr(), 256, _stream())
    assert rc == -1 and b"overflows int32 indexing" in L.mink_last_error(), "kernel_map_cube took a table of 2^31 entries"
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(dw).all() and bool((nbr == -1).all()) and bool((nbr_b == -1).all())
