"""-m gpu: no kernel of the training step writes outside the buffers it is given, skips an element it promised, or lets an
out-of-extent or pad-column read into a result.

Every entry point is called through the C ABI (nerf_downstream_amd._lib.lib(): the Python wrappers allocate for themselves)
with every output, workspace and statistics buffer a guarded.Guarded of EXACTLY the size include/mink_hip.h or the matching
*_workspace_bytes() names, and every input a Guarded.input (NaN bands, NaN pad columns).  After the call: check() on every
buffer, then the value check -- every written element finite and within the bound the existing test of the same entry point
uses, of a float64 reference computed from the logical extents only (on the CPU; the reduced-math forms, like
test_gpu_reduced_math, with torch on the GPU from contiguous copies of the logical operands, never from the guarded buffers):
  fp32 convolution forms            test_gpu_ops._chain_tolerance
  bf16 / bf16x3 convolution forms   layerwise.form_reference, bounds of test_gpu_reduced_math
  weight gradients                  2e-5 of max |dW| (test_gpu_ops test_stem_wgrad_streaming / test_mid_layer_weight_gradient_..)
  batch-norm family, head, pools    the allclose limits of test_gpu_ops / test_gpu_compat
Each case names the launch form it is meant for and asserts that the dispatcher's rules (restated in layerwise.gather_launch_form /
conv_form / wgrad_plan, and asked of mink_conv_plan / mink_conv_wgrad_workspace_bytes / _supported where the library
answers) take it there; the convolution cases also assert that the library's own plan for the very call they make
(mink_conv_gather_gemm_launch_info / mink_conv_wgrad_launch_info) is that form.  Nothing here is meant to fault: no buffer is smaller than the library asks for."""
import contextlib
import ctypes

import pytest
import torch

import layerwise as LW
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu

BM, BN, BK, CKP = 128, 64, 32, 9  # conv_common.h: dense row tile, column tile, reduction chunk, offsets per compacted workgroup
MATH_NAME = {0: "fp32", 1: "bf16", 3: "bf16x3"}


def _dev():
    return torch.device("cuda", 0)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(g):
    return None if g is None else g.ptr


def _gin(t, ld=None, pad=None, name="input"):
    return Guarded.input(t.to(_dev()), ld=ld, pad=pad, name=name)


def _gout(shape, dtype=torch.float32, name="output", **kw):
    return Guarded(shape, dtype, _dev(), name=name, **kw)


def _ws(nbytes, name="workspace"):
    """A workspace of exactly `nbytes` (None for 0): the call may write any of it, and nothing around it."""
    return Guarded(int(nbytes), torch.uint8, _dev(), written="any", name=name) if nbytes else None


def _lib():
    from nerf_downstream_amd._lib import check, lib

    return lib(), check


def _done(*bufs):
    torch.cuda.synchronize()
    check_all(*bufs)


@contextlib.contextmanager
def _knobs(L, stagger=0, math=0, pipeline=0, fold=None, small=None):
    """Set the library's switches for one case and put every one back."""
    old_math = L.mink_conv_set_math(math)
    old_pipe = L.mink_conv_set_pipeline(pipeline)
    old_fold = L.mink_bn_set_fold(fold) if fold is not None else None
    old_small = L.mink_bn_set_small(small) if small is not None else None
    L.mink_conv_set_stagger(stagger)
    try:
        yield
    finally:
        L.mink_conv_set_stagger(0)  # (the call returns the low byte only: 0 is the state every test starts from)
        L.mink_conv_set_pipeline(old_pipe)
        L.mink_conv_set_math(old_math)
        if old_fold is not None:
            L.mink_bn_set_fold(old_fold)
        if old_small is not None:
            L.mink_bn_set_small(old_small)


def _cdiv(a, b):
    return -(-a // b)


def _table(n_out, K, n_in, g):
    """About 45 % of the entries -1, one offset nobody has, one that a whole 64-row tile lacks."""
    nbr = torch.randint(0, n_in, (n_out, K), generator=g, dtype=torch.int32)
    nbr[torch.rand(n_out, K, generator=g) < 0.45] = -1
    if K > 1:
        nbr[:, K // 2 - 1] = -1
    if n_out > 128:
        nbr[64:128, min(1, K - 1)] = -1
    return nbr


def _gather64(x, B, nbr):
    """float64 sum_k x[nbr[:, k]] @ B[k] on the CPU."""
    out = torch.zeros(nbr.shape[0], B.shape[2], dtype=torch.float64)
    for k in range(nbr.shape[1]):
        sel = nbr[:, k] >= 0
        out[sel] += x[nbr[sel, k].long()].double() @ B[k].double()
    return out


def _class_perm(L, check, n, g):
    """mink_class_partition of n random rows at tensor stride 2 (pad 128): the permutation, -1 padded, as a guarded int32 buffer."""
    coords = torch.zeros(n, 4, dtype=torch.int32)
    coords[:, 1:] = torch.randint(0, 40, (n, 3), generator=g, dtype=torch.int32) * 2
    cg = _gin(coords, name="coords")
    rows = L.mink_class_partition_rows(n, 128)
    perm = _gout((rows,), torch.int32, name="row_perm")
    ws = _ws(L.mink_class_partition_workspace_bytes(n), "class_partition workspace")
    check(L.mink_class_partition(cg.ptr, n, 2, 128, perm.ptr, _ptr(ws), ws.nbytes if ws else 0, _st()))
    _done(cg, perm, ws)
    p = perm.t.cpu()
    live = p[p >= 0].long()
    assert int((p < 0).sum()) > 0 and torch.equal(torch.sort(live).values, torch.arange(n)), "class partition: not a -1 padded permutation"
    return p


# ------------------------------------------------------------------------------------------------ gather-GEMM launch forms
def _gemm(n_out, K, cin, cout, form, ldx=None, ldy=None, wt=False, flip=False, perm=False, acc=False, bias=False, ksplit=1,
          math=0, pipe=0, api="gemm", stagger=0, x_pad=None):
    return dict(n_out=n_out, K=K, cin=cin, cout=cout, form=form, ldx=ldx or cin, ldy=ldy or cout, wt=wt, flip=flip, perm=perm, acc=acc,
                bias=bias, ksplit=ksplit, math=math, pipe=pipe, api=api, stagger=stagger, x_pad=x_pad)


def _gemm_id(c):
    s = f"{c['api']}-{c['form'].replace(' ', '_')}-n{c['n_out']}-K{c['K']}-{c['cin']}x{c['cout']}-ldx{c['ldx']}-ldy{c['ldy']}-z{c['ksplit']}"
    for k in ("wt", "flip", "perm", "acc", "bias"):
        s += f"-{k}" if c[k] else ""
    return s + (f"-math{c['math']}" if c["math"] else "") + (f"-pipe{c['pipe']}" if c["pipe"] else "")


GEMM_CASES = []
# scalar form (gather_gemm_kernel): 27 channels / a row stride that is no multiple of 4
for _n in (1, 130):
    for _ldx in (27, 30):
        GEMM_CASES.append(_gemm(_n, 27, 27, 7, "scalar gather_gemm", ldx=_ldx, ldy=12, bias=_ldx == 30))
GEMM_CASES.append(_gemm(130, 27, 27, 7, "scalar gather_gemm", ldx=30, ldy=12, ksplit=3))
# flat stem form
for _n in (129, 257):
    for _ldx, _ldy, _b in ((28, 64, False), (32, 68, True), (32, 64, False), (28, 68, True)):
        GEMM_CASES.append(_gemm(_n, 27, 28, 64, "flat gather_gemm2 (cin 28)", ldx=_ldx, ldy=_ldy, bias=_b))
# dense gather_gemm2: column-tile tail (96 = 64 + 32), K 27 and 8, un-split and split over 3 / 27 slabs
for _K in (27, 8):
    for _z in (1, 3, 27):
        if _z <= _K:
            GEMM_CASES.append(_gemm(257, _K, 32, 96, "dense gather_gemm2", ldy=100, ksplit=_z, bias=_z != 3))
            GEMM_CASES.append(_gemm(257, _K, 32, 96, "dense gather_gemm2 (transposed weights)", ldy=100, ksplit=_z, wt=True, flip=True))
# transposed weights through a class permutation: staged form, and the accumulate form (rows the permutation skips keep their values)
GEMM_CASES += [
    _gemm(257, 27, 32, 96, "staged gather_gemm2 (transposed weights)", ldy=100, wt=True, perm=True),
    _gemm(257, 8, 32, 96, "staged gather_gemm2 (transposed weights)", ldy=100, wt=True, perm=True, ksplit=3),
    _gemm(257, 8, 32, 96, "staged gather_gemm2", ldy=100, perm=True),
    _gemm(257, 1, 128, 64, "staged gather_gemm2 (transposed weights) accumulate", ldy=68, wt=True, perm=True, acc=True),
    _gemm(130, 8, 32, 96, "staged gather_gemm2 (transposed weights) accumulate", ldy=100, wt=True, perm=True, acc=True),
]
# row-compacted form: ragged row counts, K 9 un-split and K 27 at every legal split, both weight layouts
for _cin, _cout in ((64, 64), (96, 128)):
    for _n in (1, 63, 65, 130):
        _wt = _n in (63, 130)
        GEMM_CASES.append(_gemm(_n, 9, _cin, _cout, "row-compacted", ldy=_cout + (4 if _n != 65 else 0), bias=True, wt=_wt, flip=_wt))
        for _z in sorted({_cdiv(27, kper) for kper in range(1, 10)}):
            GEMM_CASES.append(_gemm(_n, 27, _cin, _cout, "row-compacted", ldy=_cout + (4 if _z % 2 else 0), ksplit=_z, wt=not _wt, flip=not _wt))
# class-permuted compacted form: un-split and split over two channel chunks; three-stage pipelines; stream-K
GEMM_CASES += [
    _gemm(130, 27, 64, 64, "class-permuted compact", ldy=68, wt=True, perm=True),
    _gemm(300, 27, 64, 64, "class-permuted compact", wt=True, perm=True, ksplit=2),
    _gemm(300, 8, 96, 128, "class-permuted compact", ldy=132, perm=True, ksplit=2),
    _gemm(130, 27, 64, 64, "row-compacted three-stage", ldy=68, ksplit=3, pipe=1),
    _gemm(65, 9, 96, 128, "row-compacted three-stage", bias=True, wt=True, flip=True, pipe=1),
    _gemm(300, 27, 64, 64, "class-permuted compact three-stage", ldy=68, wt=True, perm=True, ksplit=2, pipe=2),
    _gemm(12101, 27, 64, 64, "stream-K", ksplit=7, pipe=8),
    _gemm(12101, 27, 64, 64, "stream-K", ldy=68, ksplit=9, pipe=8, wt=True, flip=True),
]
# reduced math: the dense forms and the class-permuted bf16 form
for _m in (1, 3):
    _t = " bf16" if _m == 1 else " bf16x3"
    for _K, _z in ((27, 1), (27, 3), (8, 1)):
        GEMM_CASES.append(_gemm(257, _K, 32, 96, "dense gather_gemm2" + _t, ldy=100, ksplit=_z, math=_m, bias=_z == 1))
        GEMM_CASES.append(_gemm(257, _K, 32, 96, "dense gather_gemm2 (transposed weights)" + _t, ldy=100, ksplit=_z, math=_m, wt=True, flip=True))
    GEMM_CASES.append(_gemm(257, 27, 28, 64, "flat gather_gemm2 (cin 28)" + _t, ldx=32, ldy=68, math=_m))
GEMM_CASES.append(_gemm(300, 27, 64, 64, "class-permuted compact bf16", ldy=68, wt=True, perm=True, math=1))
# statistics epilogues: direct in both kernels, and the split reduce
GEMM_CASES += [
    _gemm(257, 27, 32, 96, "dense gather_gemm2", ldy=100, bias=True, api="stats"),
    _gemm(1100, 27, 28, 64, "flat gather_gemm2 (cin 28)", ldx=32, ldy=68, api="stats"),
    _gemm(130, 9, 64, 64, "row-compacted", ldy=68, bias=True, api="stats"),
    _gemm(700, 8, 96, 128, "row-compacted", api="stats"),
    _gemm(257, 27, 32, 96, "dense gather_gemm2", ldy=100, ksplit=3, bias=True, api="stats"),
    _gemm(130, 27, 64, 64, "row-compacted", ldy=68, ksplit=7, api="stats"),
    _gemm(1, 27, 64, 64, "row-compacted", ksplit=3, api="stats"),
]
# slabs left to the caller
GEMM_CASES += [
    _gemm(130, 27, 64, 64, "row-compacted", ldy=68, ksplit=7, api="slabs"),
    _gemm(63, 9, 64, 64, "row-compacted", ldy=68, api="slabs"),
    _gemm(257, 27, 32, 96, "dense gather_gemm2 (transposed weights)", ldy=100, ksplit=3, wt=True, flip=True, api="slabs"),
    _gemm(300, 27, 64, 64, "class-permuted compact", wt=True, perm=True, ksplit=2, api="slabs"),
    _gemm(12101, 27, 64, 64, "stream-K", ksplit=9, pipe=8, api="slabs"),
]


@pytest.mark.parametrize("c", GEMM_CASES, ids=_gemm_id)
def test_gather_gemm_stays_inside_its_buffers(c):
    """mink_conv_gather_gemm / _stats / _slabs, launch form by launch form."""
    import test_gpu_ops as OPS
    import test_gpu_reduced_math as RM

    L, check = _lib()
    n_out, K, cin, cout, ldx, ldy, wt, flip, math, ks = (c[k] for k in ("n_out", "K", "cin", "cout", "ldx", "ldy", "wt", "flip", "math", "ksplit"))
    g = torch.Generator().manual_seed(n_out * 131 + K * 7 + cin + cout + ks)
    n_in = n_out + 17
    nbr = _table(n_out, K, n_in, g)
    x = torch.randn(n_in, cin, generator=g)
    B = torch.randn(K, cin, cout, generator=g) * 0.1  # B[k]: what table column k is multiplied with
    w = B.flip(0) if flip else B
    w = w.transpose(1, 2).contiguous() if wt else w.contiguous()
    bias = torch.randn(cout, generator=g) if c["bias"] else None
    form, zs = LW.gather_launch_form(n_out, K, cin, cout, ldx, ldy, wt, flip, c["perm"], c["acc"], ks, MATH_NAME[math], c["pipe"])
    assert form == c["form"], f"this shape reaches {form!r}, the case is meant for {c['form']!r}"
    perm = None
    visited = torch.ones(n_out, dtype=torch.bool)
    if c["perm"]:
        perm = _class_perm(L, check, n_out, g)
        if c["acc"]:  # an accumulating launch may skip rows: every third one here
            perm[(perm >= 0) & (perm % 3 == 0)] = -1
            visited = torch.arange(n_out) % 3 != 0
    init = torch.randn(n_out, cout, generator=g) if c["acc"] else None

    xg, wg, ng = _gin(x, ld=ldx, pad=c["x_pad"], name="x"), _gin(w, name="w"), _gin(nbr, name="nbr")
    bg = _gin(bias, name="bias") if bias is not None else None
    pg = _gin(perm, name="row_perm") if perm is not None else None
    yg = _gout((n_out, ldy), cols=cout, init=init, written=visited[:, None].expand(n_out, cout), name="y")
    slab = _gout((ks, n_out, cout), name="split-K slabs") if ks > 1 else None
    bufs = [xg, wg, ng, bg, pg, yg, slab]
    with _knobs(L, stagger=c["stagger"], math=math, pipeline=c["pipe"]):
        if form.startswith("row-compacted") or form == "stream-K":
            plan = L.mink_conv_plan(n_out, K, cin, cout, 0)
            assert plan * CKP >= K, "the planner must hand this shape to the compacted kernel"
            if form == "stream-K":
                assert plan > 1 and ks in (plan, plan + 2), f"stream-K plans {plan} slabs: the cases are the plan's count and two above, not {ks}"
        if form.startswith("class-permuted compact"):
            assert 1 <= L.mink_conv_plan(perm.numel(), K, cin, cout, 1) <= max(cin // BK, 1)
        common = (xg.ptr, n_in, ldx, cin, wg.ptr)
        tail = (_ptr(slab), slab.nbytes if slab else 0)
        # the library's own answer for the call below (the planner the launch runs) is the form in the case id
        rc, info = LW.ask_gather_launch(L, n_in, ldx, cin, wt, flip, n_out, K, perm is not None, perm.numel() if perm is not None else 0, ldy,
                                        cout, ks, acc=c["acc"], bias=bg is not None and c["api"] != "slabs", stats=c["api"] == "stats",
                                        slabs=c["api"] == "slabs", xw_aligned=(xg.ptr | wg.ptr) % 16 == 0,
                                        y_aligned=(yg.ptr | (_ptr(slab) or 0) | (_ptr(bg) or 0 if c["api"] != "slabs" else 0)) % 16 == 0)
        check(rc)
        assert (LW.launch_form_name(info, cin, c["acc"]), info.slabs) == (c["form"], zs), (LW.launch_form_name(info, cin, c["acc"]), info.slabs)
        if c["api"] == "stats":
            sw = _ws(L.mink_conv_stats_workspace_bytes(n_out, cout), "stats_ws")
            so = _gout((512, 2, cout), torch.float64, name="stats_out")
            rows = ctypes.c_int32(-1)
            check(L.mink_conv_gather_gemm_stats(*common, ng.ptr, n_out, K, yg.ptr, ldy, cout, _ptr(bg), ks, *tail, so.ptr, ctypes.byref(rows),
                                                sw.ptr, sw.nbytes, _st()))
            bufs += [sw, so]
        elif c["api"] == "slabs":
            nsl = ctypes.c_int32(-1)
            check(L.mink_conv_gather_gemm_slabs(*common, int(wt), int(flip), ng.ptr, n_out, K, _ptr(pg), perm.numel() if perm is not None else 0,
                                                yg.ptr, ldy, cout, ks, *tail, ctypes.byref(nsl), _st()))
        else:
            check(L.mink_conv_gather_gemm(*common, int(wt), int(flip) | (2 if c["acc"] else 0), ng.ptr, n_out, K, _ptr(pg),
                                          perm.numel() if perm is not None else 0, yg.ptr, ldy, cout, _ptr(bg), ks, *tail, _st()))
        torch.cuda.synchronize()
    # where the call wrote
    if slab is not None:  # every slab the launch planned is written in full (the reduce reads them all), the others not at all
        m = torch.zeros(ks, n_out, cout, dtype=torch.bool)
        m[:zs] = True
        slab.set_written(m)
    if c["api"] == "slabs":
        assert nsl.value == zs, (nsl.value, zs)
        if zs > 1:
            yg.set_written(False)  # the partial sums stay in the workspace: y is not touched
    if c["api"] == "stats":
        want_rows = min(512, _cdiv(_cdiv(n_out, 64 if form.startswith("row-compacted") else BM), 8)) if zs == 1 else \
            max(1, min(512, _cdiv(n_out, (256 // (cout // 4)) * 4)))
        assert rows.value == want_rows, (rows.value, want_rows)
        m = torch.zeros(512, 2, cout, dtype=torch.bool)
        m[: rows.value] = True
        so.set_written(m)
    _done(*bufs)
    # what it wrote
    if c["api"] == "slabs" and zs > 1:
        got = slab.t[:zs].double().sum(0).cpu()
        assert_finite(slab.t[:zs], "slabs")
    else:
        got = yg.logical().cpu().double()
        assert_finite(yg.logical()[visited.to(_dev())], "y")
    xd, Bd, nd = x.to(_dev()), B.to(_dev()), nbr.to(_dev())
    extra = (bias.double() if bias is not None else 0.0)
    if math == 0:
        ref = _gather64(x, B, nbr) + extra
        if init is not None:
            ref = torch.where(visited[:, None], ref + init.double(), init.double())
        scale = float(ref.abs().max()) + 1e-30
        tol = OPS._chain_tolerance(xd, Bd, nd, _gather64(x, B, nbr), scale)
        err = float((got - ref).abs().max()) / scale
        assert err < tol, (form, err, tol)
    else:
        conv_cin, conv_cout = (cout, cin) if wt else (cin, cout)
        cf = LW.conv_form("dgrad" if wt else "fwd", K, conv_cin, conv_cout, MATH_NAME[math], n_out=n_out, ldx=ldx, row_perm=c["perm"],
                          ksplit=ks, shortcut_dense=False)
        assert cf.rounded, form
        kind = "bf16x3" if cf.split else "bf16"
        names = ("dy", "w") if wt else ("x", "w")
        ref = LW.form_reference(lambda **o: RM._gather64(o[names[0]], o[names[1]], nd), {names[0]: xd, names[1]: Bd}, cf).cpu() + extra
        seq = RM._gather_seq32(RM._pairs(xd, Bd, kind), nd).cpu().double() + extra
        rel_s, max_s = RM._errs(seq, ref)
        rel, mx = RM._errs(got, ref)
        assert rel <= max(RM.REL_FLOOR, 2.0 * rel_s) and mx <= max(RM.MAX_FLOOR, 2.0 * max_s), (form, rel, rel_s, mx, max_s)
    if c["api"] == "stats":  # the written rows are the column sums of the y the call wrote
        yd = yg.logical().double()
        s = so.t[: rows.value].sum(0)
        assert_finite(so.t[: rows.value], "stats_out")
        e0 = float(((s[0] - yd.sum(0)).abs() / yd.abs().sum(0).clamp_min(1e-30)).max())
        e1 = float(((s[1] - (yd * yd).sum(0)).abs() / (yd * yd).sum(0).clamp_min(1e-30)).max())
        assert max(e0, e1) <= 1e-5, (form, e0, e1)  # fp32 sums of y's own values, per partial row (test_gpu_reduced_math)


# ------------------------------------------------------------------------------------------------ weight gradients
def _wgrad64(x, dy, nbr):
    """float64 dW[k] = x[nbr[:, k]]^T dy on the CPU."""
    K = nbr.shape[1]
    out = torch.zeros(K, x.shape[1], dy.shape[1], dtype=torch.float64)
    for k in range(K):
        sel = nbr[:, k] >= 0
        out[k] = x[nbr[sel, k].long()].double().T @ dy[sel].double()
    return out


def _wg(n_out, K, cin, cout, form, ldx=None, ldy=None, force=0, math=0, stagger=0):
    return dict(n_out=n_out, K=K, cin=cin, cout=cout, form=form, ldx=ldx or cin + 4, ldy=ldy or cout + 4, force=force, math=math, stagger=stagger)


def _wg_id(c):
    return (f"{c['form'].replace(' ', '_')}-n{c['n_out']}-K{c['K']}-{c['cin']}x{c['cout']}-ldx{c['ldx']}-ldy{c['ldy']}"
            + (f"-force{c['force']:#x}" if c["force"] else "") + (f"-math{c['math']}" if c["math"] else ""))


WGRAD_CASES = []
# tiled fp32: one split (straight into dw) and several (slabs + reduce); ldx > cin, ldy > cout (27 -> 31 / 7 -> 11: the scalar loads)
for _n in (100, 300):
    for _cin, _cout in ((27, 7), (20, 36), (96, 64)):
        for _K in (1, 8, 27):
            _plan = LW.wgrad_plan(_n, _K, _cin, _cout)
            WGRAD_CASES.append(_wg(_n, _K, _cin, _cout, f"wgrad fp32 G{_plan[0]}" + (" split" if _plan[1] > 1 else "")))
# forced plans (the encodings of test_gpu_reduced_math.WGRAD_CASES): G = 3 and 9, one and several row splits
WGRAD_CASES += [
    _wg(1000, 27, 64, 128, "wgrad fp32 G3", force=2 | (1 << 4)),
    _wg(1000, 27, 128, 128, "wgrad fp32 G3 split", force=2 | (4 << 4), ldx=128, ldy=128),
    _wg(1000, 8, 64, 64, "wgrad fp32 G3", force=2 | (1 << 4)),
    _wg(1000, 27, 64, 64, "wgrad fp32 G9 split", force=3 | (2 << 4)),
    _wg(300, 27, 96, 64, "wgrad fp32 G9", force=3 | (1 << 4)),
    _wg(1000, 27, 64, 64, "wgrad fp32 G1", force=1 | (1 << 4)),
]
# the streaming stem kernel at its natural threshold (tests/test_capi.py: 43,649 rows is the first count that takes it)
WGRAD_CASES += [
    _wg(43649, 27, 28, 64, "wgrad_stream G9 split", ldx=32, ldy=64),
    _wg(43649, 27, 32, 64, "wgrad_stream G9 split", ldx=32, ldy=68),
    _wg(43649, 27, 16, 64, "wgrad_stream G9 split", ldx=20, ldy=64),
]
# ... and forced at 2,200 rows: 17 splits asked -> 16, 256 rows each -> 9 with rows, rounded up to 16: seven empty trailing splits
WGRAD_CASES += [
    _wg(2200, 27, 28, 64, "wgrad_stream G9 split", ldx=32, ldy=68, force=3 | (17 << 4)),
    _wg(2200, 27, 20, 36, "wgrad_stream G9 split", ldx=24, ldy=36, force=3 | (17 << 4)),
]
# bf16 math: the streaming bf16 kernel and wgrad16<1> / <3>
WGRAD_CASES += [
    _wg(2200, 27, 28, 64, "wgrad_stream_bf16 G9 split", ldx=32, ldy=68, force=3 | (17 << 4), math=1),
    _wg(43649, 27, 28, 64, "wgrad_stream_bf16 G9 split", ldx=32, ldy=64, math=1),
    _wg(300, 27, 64, 64, "wgrad16<1> G1 split", ldx=68, ldy=68, force=1 | (3 << 4), math=1),
    _wg(100, 8, 64, 128, "wgrad16<1> G1", ldx=64, ldy=132, force=1 | (1 << 4), math=1),
    _wg(300, 27, 128, 64, "wgrad16<3> G3 split", ldx=132, ldy=64, force=2 | (2 << 4), math=1),
    _wg(1000, 8, 64, 64, "wgrad16<3> G3", ldx=68, ldy=68, force=2 | (1 << 4), math=1),
]


@pytest.mark.parametrize("c", WGRAD_CASES, ids=_wg_id)
def test_weight_gradient_stays_inside_its_buffers(c):
    """mink_conv_wgrad: dw exactly K x cin x cout floats, the workspace exactly mink_conv_wgrad_workspace_bytes() as asked AFTER the
    knobs are set; every slab of a split plan is written in full (empty trailing splits store zeros), dw in full."""
    L, check = _lib()
    n_out, K, cin, cout, ldx, ldy, force, math = (c[k] for k in ("n_out", "K", "cin", "cout", "ldx", "ldy", "force", "math"))
    g = torch.Generator().manual_seed(n_out + 17 * K + cin * 3 + cout)
    n_in = n_out + 17
    nbr = _table(n_out, K, n_in, g)
    x, dy = torch.randn(n_in, cin, generator=g), torch.randn(n_out, cout, generator=g)
    cf = LW.conv_form("wgrad", K, cin, cout, MATH_NAME[math], n_out=n_out, ldx=ldx, ldy=ldy, force_g=force)
    assert cf.form == c["form"], f"this shape reaches {cf.form!r}, the case is meant for {c['form']!r}"
    G, nsplit = LW.wgrad_plan(n_out, K, cin, cout, force)
    xg, dg, ng = _gin(x, ld=ldx, name="x"), _gin(dy, ld=ldy, name="dy"), _gin(nbr, name="nbr")
    dw = _gout((K, cin, cout), name="dw")
    with _knobs(L, stagger=(force << 12) | c["stagger"], math=math):
        need = L.mink_conv_wgrad_workspace_bytes(n_out, K, cin, cout)
        assert need == (4 * nsplit * K * cin * cout if nsplit > 1 else 0), (need, nsplit)
        if "stream" in cf.form and not force:
            assert L.mink_conv_wgrad_bn_relu_pool_supported(n_in, ldx, cin, n_out, K, cout) == 1
            assert L.mink_conv_wgrad_bn_relu_pool_supported(n_in, ldx, cin, n_out - 1, K, cout) == 0  # the threshold itself
        slabs = _gout((nsplit, K, cin, cout), name="row-split slabs") if need else None
        rc, info = LW.ask_wgrad_launch(L, n_in, ldx, cin, ldy, cout, n_out, K, aligned=(xg.ptr | dg.ptr) % 16 == 0)
        check(rc)
        assert (LW.wgrad_form_name(info), info.slabs) == (c["form"], nsplit)  # the library's own answer for the call below
        check(L.mink_conv_wgrad(xg.ptr, n_in, ldx, cin, dg.ptr, ldy, cout, ng.ptr, n_out, K, dw.ptr, _ptr(slabs), need, _st()))
        torch.cuda.synchronize()
    _done(xg, dg, ng, dw, slabs)
    assert_finite(dw.t, "dw")
    if slabs is not None:
        assert_finite(slabs.t, "slabs")
    ops = LW.apply_rounding({"x": x, "dy": dy}, cf.rounded)
    ref = _wgrad64(ops["x"], ops["dy"], nbr)
    scale = float(ref.abs().max()) + 1e-30
    err = float((dw.t.cpu().double() - ref).abs().max()) / scale
    assert err <= 2e-5, (cf.form, err)  # fp32 sums of <= n_out products (test_gpu_ops: test_stem_wgrad_streaming, wgrad16)


def _fused_operands(n_out, cin, cout, g, b16):
    n_in, n_pool = n_out + 17, n_out // 5 + 3
    nbr = _table(n_out, 27, n_in, g)
    x = torch.randn(n_in, cin, generator=g)
    y = torch.randn(n_out, cout, generator=g) * 1.5 + 0.2
    if b16:
        x, y = LW.bf16_rne(x), LW.bf16_rne(y)
    in2out = torch.randint(0, n_pool, (n_out,), generator=g, dtype=torch.int32)
    dyp = torch.randn(n_pool, cout, generator=g)
    mean, var = y.mean(0), y.var(0, unbiased=False)
    invstd = (var + 1e-5).rsqrt()
    gamma, beta = torch.rand(cout, generator=g) + 0.5, torch.rand(cout, generator=g) - 0.5
    dgamma, dbeta = torch.randn(cout, generator=g) * 30, torch.randn(cout, generator=g) * 30
    return n_in, n_pool, nbr, x, y, in2out, dyp, mean, invstd, gamma, beta, dgamma, dbeta


@pytest.mark.parametrize("cin,ldx,cout,kind,form", [
    (28, 32, 64, "fp32", "wgrad_stream<FUSE, FLAT>"), (16, 16, 64, "fp32", "wgrad_stream<FUSE>"),
    (28, 32, 64, "bf16", "wgrad_stream_bf16<FUSE>"),
    (28, 32, 64, "b16", "wgrad_stream_b16t"), (28, 32, 32, "b16", "wgrad_stream_bf16<FUSE, B16>")])
def test_fused_stem_weight_gradient_stays_inside_its_buffers(cin, ldx, cout, kind, form):
    """mink_conv_wgrad_bn_relu_pool (fp32 and bf16 math) and mink_conv_wgrad_bn_relu_pool_b16 (both kernels) at the first row count
    the streaming kernel takes: dY is recomputed from (y, pooled gradient, statistics) in the operand load
    (layerwise.stem_wgrad_operand restates it in fp32) and never written."""
    L, check = _lib()
    n_out, K = 43649, 27
    b16 = kind == "b16"
    math = 0 if kind == "fp32" else 1
    g = torch.Generator().manual_seed(cin * 5 + cout + len(kind))
    n_in, n_pool, nbr, x, y, in2out, dyp, mean, invstd, gamma, beta, dgamma, dbeta = _fused_operands(n_out, cin, cout, g, b16)
    # (which kernel: wgrad_plan in csrc/conv_wgrad.hip -- flat when 512 < K cin <= 768, ldx <= 32, cin >= 16; b16t when cout == 64)
    flat = 512 < K * cin <= 768 and ldx <= 32 and cin >= 16
    want = {"fp32": "wgrad_stream<FUSE" + (", FLAT>" if flat else ">"), "bf16": "wgrad_stream_bf16<FUSE>",
            "b16": "wgrad_stream_b16t" if cout == 64 else "wgrad_stream_bf16<FUSE, B16>"}[kind]
    assert want == form
    if b16:  # bf16 storage: x [n_in][cin] at row pitch 32 (NaN in the pad columns, as for every input), y [n_out][cout]
        xg, yg = _gin(x.bfloat16(), ld=32, name="xb"), _gin(y.bfloat16(), name="yb")
    else:
        xg, yg = _gin(x, ld=ldx, name="x"), _gin(y, name="y")
    ins = [_gin(t, name=nm) for t, nm in ((dyp, "dy_pool"), (in2out, "in2out"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma"),
                                         (beta, "beta"), (dgamma, "dgamma"), (dbeta, "dbeta"), (nbr, "nbr"))]
    dpg, iog, mg, isg, gag, beg, dgg, dbg, ng = ins
    dw = _gout((K, cin, cout), name="dw")
    with _knobs(L, math=math):
        assert L.mink_conv_wgrad_bn_relu_pool_supported(n_in, ldx, cin, n_out, K, cout) == 1
        need = L.mink_conv_wgrad_workspace_bytes(n_out, K, cin, cout)
        _, nsplit = LW.wgrad_plan(n_out, K, cin, cout)
        assert nsplit > 1 and need == 4 * nsplit * K * cin * cout
        slabs = _gout((nsplit, K, cin, cout), name="row-split slabs")
        rc, info = LW.ask_wgrad_launch(L, n_in, 32 if b16 else ldx, cin, cout, cout, n_out, K, fuse=2 if b16 else 1, n_pool=n_pool,
                                       aligned=(xg.ptr | yg.ptr) % 16 == 0)
        check(rc)
        assert (LW.wgrad_form_name(info, instantiation=True), info.slabs) == (form, nsplit)  # the library's own answer for the call below
        stats = (mg.ptr, isg.ptr, gag.ptr, beg.ptr, dgg.ptr, dbg.ptr, ng.ptr, n_out, K, dw.ptr, slabs.ptr, need, _st())
        if b16:
            check(L.mink_conv_wgrad_bn_relu_pool_b16(xg.ptr, n_in, cin, yg.ptr, cout, dpg.ptr, n_pool, iog.ptr, *stats))
        else:
            check(L.mink_conv_wgrad_bn_relu_pool(xg.ptr, n_in, ldx, cin, yg.ptr, cout, dpg.ptr, n_pool, iog.ptr, *stats))
        torch.cuda.synchronize()
    _done(xg, yg, *ins, dw, slabs)
    assert_finite(dw.t, "dw")
    v = LW.stem_wgrad_operand(dyp, y, mean, invstd, gamma, beta, dgamma, dbeta, in2out, n_out)
    ops = LW.apply_rounding({"x": x, "dy": v}, frozenset({"x", "dy"}) if math else frozenset())
    ref = _wgrad64(ops["x"], ops["dy"], nbr)
    scale = float(ref.abs().max()) + 1e-30
    err = float((dw.t.cpu().double() - ref).abs().max()) / scale
    assert err <= 2e-5, (form, err)  # (test_gpu_ops.test_fused_stem_conv_bn_relu_pool: 2e-5 of max |dW|)


# ------------------------------------------------------------------------------------------------ batch-norm family
EPS, MOM = 1e-5, 0.1
BN_GRID = [(n, C) for n in (1, 63, 1025, 3001) for C in (4, 48, 64, 1536, 2048)]


def _bn_options(i):
    """relu, residual, dresidual -- walked over the (n, C) grid so that every value of each meets small and large shapes."""
    return i % 2 == 0, i % 3 != 2, i % 4 != 3


assert {_bn_options(i)[k] for i in range(len(BN_GRID)) for k in (0,)} == {True, False}
assert {_bn_options(i)[1:] for i in range(len(BN_GRID))} == {(True, True), (True, False), (False, True), (False, False)}


def _bn_data(n, C, seed, res):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    r = torch.randn(n, C, generator=g) if res else None
    return g, x, gamma, beta, r


def _bn_fwd64(x, gamma, beta, r, relu):
    x = x.double()
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    invstd = (var + EPS).rsqrt()
    z = (x - mean) * invstd * gamma.double() + beta.double()
    if r is not None:
        z = z + r.double()
    return mean, var, invstd, (z.clamp_min(0) if relu else z)


def _bn_bwd64(gy, x, y, mean, invstd, gamma, relu):
    """dx, masked gradient, dgamma, dbeta in float64 from the statistics and the ReLU decisions (y > 0) the kernel is given."""
    n = x.shape[0]
    gm = gy.double() * (y > 0).double() if relu else gy.double()
    xhat = (x.double() - mean.double()) * invstd.double()
    dbeta, dgamma = gm.sum(0), (gm * xhat).sum(0)
    dx = gamma.double() * invstd.double() * (gm - dbeta / n - xhat * dgamma / n)
    return dx, gm, dgamma, dbeta


def _close(got, want, atol, rtol, name):
    assert_finite(got, name)
    got, want = got.detach().cpu().double(), want.double()
    assert torch.allclose(got, want, atol=atol, rtol=rtol), (name, float((got - want).abs().max()))


def _check_stats(n, mean, invstd, rm, rv, m64, v64, is64, tag, x, gamma, beta):
    """Statistics a kernel wrote, at the limits test_gpu_ops.test_batch_norm holds the forward pass to: the mean, the running
    statistics, and the normalised values these statistics give (invstd has no limit of its own there)."""
    _close(mean.t, m64, 1e-5, 0.0, tag + " mean")
    assert_finite(invstd.t, tag + " invstd")
    x64 = x.double()
    z = (x64 - mean.t.cpu().double()) * invstd.t.cpu().double() * gamma.double() + beta.double()
    _close(z, (x64 - m64) * is64 * gamma.double() + beta.double(), 1e-5, 1e-5, tag + " normalised with mean / invstd")
    if n > 1:  # (one row: torch refuses, the unbiased variance has no value)
        _close(rm.t, MOM * m64, 1e-6, 0.0, tag + " running_mean")
        _close(rv.t, (1 - MOM) + MOM * v64 * n / (n - 1), 1e-5, 0.0, tag + " running_var")


def _running(C):
    return _gout((C,), init=torch.zeros(C), name="running_mean"), _gout((C,), init=torch.ones(C), name="running_var")


@pytest.mark.parametrize("i", range(len(BN_GRID)), ids=[f"n{n}-C{C}" for n, C in BN_GRID])
def test_batch_norm_forward_stays_inside_its_buffers(i):
    """mink_bn_stats, _apply, _fwd, _apply_from_partials (fold off and forced), _reduce mode 0 + _stats_from_sums: workspace exactly
    mink_bn_workspace_bytes(n, C), mean / invstd / running statistics exactly C floats."""
    L, check = _lib()
    n, C = BN_GRID[i]
    relu, res, _ = _bn_options(i)
    g, x, gamma, beta, r = _bn_data(n, C, 100 + i, res)
    m64, v64, is64, out64 = _bn_fwd64(x, gamma, beta, r, relu)
    wsb = L.mink_bn_workspace_bytes(n, C)
    xg, gg, bg = _gin(x, name="x"), _gin(gamma, name="gamma"), _gin(beta, name="beta")
    rg = _gin(r, name="residual") if res else None
    ins = [xg, gg, bg, rg]
    # mink_bn_stats
    mean, invstd, (rm, rv), ws = _gout((C,), name="mean"), _gout((C,), name="invstd"), _running(C), _ws(wsb)
    check(L.mink_bn_stats(xg.ptr, n, C, EPS, MOM, mean.ptr, invstd.ptr, rm.ptr, rv.ptr, ws.ptr, wsb, _st()))
    _done(*ins, mean, invstd, rm, rv, ws)
    _check_stats(n, mean, invstd, rm, rv, m64, v64, is64, "bn_stats", x, gamma, beta)
    # mink_bn_apply with float64's own statistics
    mi, ii = _gin(m64.float(), name="mean"), _gin(is64.float(), name="invstd")
    y = _gout((n, C), name="y")
    check(L.mink_bn_apply(xg.ptr, n, C, mi.ptr, ii.ptr, gg.ptr, bg.ptr, _ptr(rg), int(relu), y.ptr, _st()))
    _done(*ins, mi, ii, y)
    _close(y.t, out64, 1e-5, 1e-5, "bn_apply y")
    # mink_bn_fwd
    y, mean, invstd, (rm, rv), ws = _gout((n, C), name="y"), _gout((C,), name="mean"), _gout((C,), name="invstd"), _running(C), _ws(wsb)
    check(L.mink_bn_fwd(xg.ptr, n, C, EPS, MOM, gg.ptr, bg.ptr, _ptr(rg), int(relu), y.ptr, mean.ptr, invstd.ptr, rm.ptr, rv.ptr, ws.ptr, wsb, _st()))
    _done(*ins, y, mean, invstd, rm, rv, ws)
    _close(y.t, out64, 1e-5, 1e-5, "bn_fwd y")
    _check_stats(n, mean, invstd, rm, rv, m64, v64, is64, "bn_fwd", x, gamma, beta)
    # mink_bn_apply_from_partials: genuine partials of x over interleaved rows; two launches, and the finalize folded into the apply pass
    rows = min(n, 67)
    part = torch.stack([torch.stack([x[q::rows].double().sum(0), (x[q::rows].double() ** 2).sum(0)]) for q in range(rows)])
    pg = _gin(part, name="partials")
    for fold in (0, 1128):
        with _knobs(L, fold=fold):
            y, mean, invstd, (rm, rv) = _gout((n, C), name="y"), _gout((C,), name="mean"), _gout((C,), name="invstd"), _running(C)
            check(L.mink_bn_apply_from_partials(xg.ptr, n, C, pg.ptr, rows, EPS, MOM, gg.ptr, bg.ptr, _ptr(rg), int(relu), y.ptr, mean.ptr,
                                                invstd.ptr, rm.ptr, rv.ptr, _st()))
            _done(*ins, pg, y, mean, invstd, rm, rv)
        _close(y.t, out64, 2e-5, 1e-5, f"bn_apply_from_partials fold {fold} y")  # (test_batch_norm_finalize_inside_the_apply_pass_is_bitwise)
        _check_stats(n, mean, invstd, rm, rv, m64, v64, is64, f"bn_apply_from_partials fold {fold}", x, gamma, beta)
    # mink_bn_reduce mode 0 -> mink_bn_stats_from_sums (the split form of the synchronised batch norm)
    sums, ws = _gout((2 * C,), torch.float64, name="sums"), _ws(wsb)
    check(L.mink_bn_reduce(0, xg.ptr, None, None, n, C, None, None, sums.ptr, ws.ptr, wsb, _st()))
    _done(*ins, sums, ws)
    x64 = x.double()
    _close(sums.t, torch.cat([x64.sum(0), (x64 * x64).sum(0)]), 2e-3, 1e-4, "bn_reduce sums")  # (column sums: the limits of dgamma / dbeta)
    sg, ng = _gin(torch.cat([x64.sum(0), (x64 * x64).sum(0)]), name="sums"), _gin(torch.tensor([float(n)], dtype=torch.float64), name="n_total")
    mean, invstd, (rm, rv) = _gout((C,), name="mean"), _gout((C,), name="invstd"), _running(C)
    check(L.mink_bn_stats_from_sums(sg.ptr, ng.ptr, C, EPS, MOM, mean.ptr, invstd.ptr, rm.ptr, rv.ptr, _st()))
    _done(sg, ng, mean, invstd, rm, rv)
    _check_stats(n, mean, invstd, rm, rv, m64, v64, is64, "bn_stats_from_sums", x, gamma, beta)


@pytest.mark.parametrize("i", range(len(BN_GRID)), ids=[f"n{n}-C{C}" for n, C in BN_GRID])
def test_batch_norm_backward_stays_inside_its_buffers(i):
    """mink_bn_bwd (fold off and forced), _bwd_slabs (C <= 1024), _reduce mode 1 + _bwd_from_sums: dgamma / dbeta exactly C floats,
    scratch2c exactly 2 C, dresidual present and NULL."""
    L, check = _lib()
    n, C = BN_GRID[i]
    relu, res, dres = _bn_options(i)
    g, x, gamma, beta, r = _bn_data(n, C, 300 + i, res)
    m64, v64, is64, out64 = _bn_fwd64(x, gamma, beta, r, relu)
    mean, invstd, y = m64.float(), is64.float(), out64.float()
    gy = torch.randn(n, C, generator=g)
    dx64, gm64, dga64, dbe64 = _bn_bwd64(gy, x, y, mean, invstd, gamma, relu)
    wsb = L.mink_bn_workspace_bytes(n, C)
    dyg, xg, yg, mg, ig, gg = (_gin(t, name=nm) for t, nm in ((gy, "dy"), (x, "x"), (y, "y"), (mean, "mean"), (invstd, "invstd"), (gamma, "gamma")))
    ins = [dyg, xg, yg, mg, ig, gg]

    def outs():
        return (_gout((n, C), name="dx"), _gout((n, C), name="dresidual") if dres else None, _gout((C,), name="dgamma"),
                _gout((C,), name="dbeta"))

    def judge(dx, dr, dga, dbe, tag):
        _close(dx.t, dx64, 1e-5, 1e-4, tag + " dx")
        _close(dga.t, dga64, 2e-3, 1e-4, tag + " dgamma")
        _close(dbe.t, dbe64, 2e-3, 1e-4, tag + " dbeta")
        if dr is not None:
            _close(dr.t, gm64, 1e-6, 0.0, tag + " dresidual")

    for fold in (0, 1128):
        with _knobs(L, fold=fold):
            dx, dr, dga, dbe = outs()
            ws = _ws(wsb)
            check(L.mink_bn_bwd(dyg.ptr, xg.ptr, yg.ptr if relu else None, n, C, mg.ptr, ig.ptr, gg.ptr, int(relu), dx.ptr, _ptr(dr), dga.ptr,
                                dbe.ptr, ws.ptr, wsb, _st()))
            _done(*ins, dx, dr, dga, dbe, ws)
        judge(dx, dr, dga, dbe, f"bn_bwd fold {fold}")
    if C <= 1024:  # the incoming gradient as three split-K slabs plus (where there is a residual branch) an addend
        parts = torch.randn(3, n, C, generator=g)
        addend = torch.randn(n, C, generator=g) if res else None
        total = parts.double().sum(0) + (addend.double() if res else 0.0)
        sl, ad = _gin(parts, name="dy_slabs"), (_gin(addend, name="addend") if res else None)
        dx, dr, dga, dbe = outs()
        dsum, ws = _gout((n, C), name="dy_sum"), _ws(wsb)
        check(L.mink_bn_bwd_slabs(sl.ptr, 3, _ptr(ad), dsum.ptr, xg.ptr, yg.ptr if relu else None, n, C, mg.ptr, ig.ptr, gg.ptr, int(relu), dx.ptr,
                                  _ptr(dr), dga.ptr, dbe.ptr, ws.ptr, wsb, _st()))
        _done(*ins, sl, ad, dx, dr, dga, dbe, dsum, ws)
        _close(dsum.t, total, 1e-5, 0.0, "bn_bwd_slabs dy_sum")  # (test_one_launch_batch_norm_of_few_row_layers: the slab sum)
        d2, g2, a2, b2 = _bn_bwd64(dsum.t.cpu(), x, y, mean, invstd, gamma, relu)
        _close(dx.t, d2, 1e-5, 1e-4, "bn_bwd_slabs dx")
        _close(dga.t, a2, 2e-3, 1e-4, "bn_bwd_slabs dgamma")
        _close(dbe.t, b2, 2e-3, 1e-4, "bn_bwd_slabs dbeta")
        if dr is not None:
            _close(dr.t, g2, 1e-6, 0.0, "bn_bwd_slabs dresidual")
    # mink_bn_reduce mode 1 -> mink_bn_bwd_from_sums
    sums, ws = _gout((2 * C,), torch.float64, name="sums"), _ws(wsb)
    check(L.mink_bn_reduce(1, dyg.ptr, xg.ptr, yg.ptr if relu else None, n, C, mg.ptr, ig.ptr, sums.ptr, ws.ptr, wsb, _st()))
    _done(*ins, sums, ws)
    _close(sums.t[:C], dbe64, 2e-3, 1e-4, "bn_reduce sum g")
    _close(sums.t[C:], dga64, 2e-3, 1e-4, "bn_reduce sum g xhat")
    sg, ng = _gin(torch.cat([dbe64, dga64]), name="sums"), _gin(torch.tensor([float(n)], dtype=torch.float64), name="n_total")
    dx, dr, _, _ = outs()
    scratch = _ws(8 * C, "scratch2c")
    check(L.mink_bn_bwd_from_sums(dyg.ptr, xg.ptr, yg.ptr if relu else None, n, C, sg.ptr, ng.ptr, mg.ptr, ig.ptr, gg.ptr, int(relu), dx.ptr,
                                  _ptr(dr), scratch.ptr, _st()))
    _done(*ins, sg, ng, dx, dr, scratch)
    _close(dx.t, dx64, 1e-5, 1e-4, "bn_bwd_from_sums dx")
    if dr is not None:
        _close(dr.t, gm64, 1e-6, 0.0, "bn_bwd_from_sums dresidual")


@pytest.mark.parametrize("n,C,nslab,relu,res,width", [
    (1, 16, 0, True, False, 1), (1, 1024, 3, False, True, 1), (777, 48, 14, True, True, 1), (777, 16, 3, False, False, 1),
    (1024, 1024, 0, True, True, 1), (1024, 48, 3, True, False, 1), (1024, 16, 14, False, True, 1),
    (777, 48, 3, True, True, 16), (1024, 1024, 3, True, False, 8), (1, 16, 14, False, True, 16)])
def test_one_launch_batch_norm_stays_inside_its_buffers(n, C, nslab, relu, res, width):
    """mink_bn_small_fwd / _bwd: slabs summed into y (or y as given), statistics, norm, residual, ReLU in one launch each way.
    width: mink_bn_set_small -- 1 = channels per workgroup by the channel count (8 below 1,024 channels, else 16), 8 / 16 forced."""
    L, check = _lib()
    with _knobs(L, small=width):
        assert L.mink_bn_small_rows() == 1024
        _one_launch_batch_norm(L, check, n, C, nslab, relu, res)


def _one_launch_batch_norm(L, check, n, C, nslab, relu, res):
    g, x, gamma, beta, r = _bn_data(n, C, n + C + nslab, res)
    parts = torch.randn(max(nslab, 1), n, C, generator=g) * 1.5 + 0.2
    ysum = parts[:nslab].double().sum(0).float() if nslab else parts[0]
    m64, v64, is64, out64 = _bn_fwd64(ysum, gamma, beta, r, relu)
    gg, bg, rg = _gin(gamma, name="gamma"), _gin(beta, name="beta"), (_gin(r, name="residual") if res else None)
    sl = _gin(parts[:nslab], name="slabs") if nslab else None
    y = _gout((n, C), name="y") if nslab else _gin(parts[0], name="y")
    out, mean, invstd, (rm, rv) = _gout((n, C), name="out"), _gout((C,), name="mean"), _gout((C,), name="invstd"), _running(C)
    check(L.mink_bn_small_fwd(_ptr(sl), nslab, n, C, y.ptr, EPS, MOM, gg.ptr, bg.ptr, _ptr(rg), int(relu), out.ptr, mean.ptr, invstd.ptr,
                              rm.ptr, rv.ptr, _st()))
    _done(gg, bg, rg, sl, y, out, mean, invstd, rm, rv)
    _close(y.t, parts[:nslab].double().sum(0) if nslab else parts[0], 1e-5, 1e-6, "bn_small_fwd y")
    _close(out.t, out64, 2e-5, 1e-5, "bn_small_fwd out")
    _close(mean.t, m64, 1e-5, 0.0, "bn_small_fwd mean")
    assert_finite(invstd.t, "invstd")
    if n > 1:
        _close(rm.t, MOM * m64, 1e-6, 0.0, "bn_small_fwd running_mean")
        _close(rv.t, (1 - MOM) + MOM * v64 * n / (n - 1), 1e-5, 0.0, "bn_small_fwd running_var")
    # backward, the incoming gradient as slabs (+ an addend where there is a residual branch)
    meanf, invf, yf = m64.float(), is64.float(), out64.float()
    gparts = torch.randn(max(nslab, 1), n, C, generator=g)
    addend = torch.randn(n, C, generator=g) if (res and nslab) else None
    gtot = (gparts[:nslab].double().sum(0) if nslab else gparts[0].double()) + (addend.double() if addend is not None else 0.0)
    dyg = _gin(gparts[:nslab] if nslab else gparts[0], name="dy")
    ad = _gin(addend, name="addend") if addend is not None else None
    xg, yg, mg, ig = _gin(ysum, name="x"), _gin(yf, name="y"), _gin(meanf, name="mean"), _gin(invf, name="invstd")
    dsum = _gout((n, C), name="dy_sum") if nslab else None
    dx, dr, dga, dbe = _gout((n, C), name="dx"), (_gout((n, C), name="dresidual") if res else None), _gout((C,), name="dgamma"), _gout((C,), name="dbeta")
    check(L.mink_bn_small_bwd(dyg.ptr, nslab, _ptr(ad), _ptr(dsum), xg.ptr, yg.ptr if relu else None, n, C, mg.ptr, ig.ptr, gg.ptr, int(relu),
                              dx.ptr, _ptr(dr), dga.ptr, dbe.ptr, _st()))
    _done(dyg, ad, xg, yg, mg, ig, gg, dsum, dx, dr, dga, dbe)
    if nslab:
        _close(dsum.t, gtot, 1e-5, 0.0, "bn_small_bwd dy_sum")
    d2, g2, a2, b2 = _bn_bwd64(dsum.t.cpu() if nslab else gparts[0], ysum, yf, meanf, invf, gamma, relu)
    assert_finite(dx.t, "dx")
    scale = float(d2.abs().max()) + 1e-12
    assert float((dx.t.cpu().double() - d2).abs().max()) < 2e-4 * max(scale, 1.0)
    if n > 1:
        _close(dga.t, a2, 2e-3, 1e-4, "bn_small_bwd dgamma")
    _close(dbe.t, b2, 2e-3, 1e-4, "bn_small_bwd dbeta")
    if dr is not None:
        _close(dr.t, g2, 1e-6, 0.0, "bn_small_bwd dresidual")


@pytest.mark.parametrize("n_out,C,dx_null", [(1, 4, False), (63, 48, True), (1025, 64, False), (400, 1024, True)])
def test_fused_bn_relu_pool_stays_inside_its_buffers(n_out, C, dx_null):
    """mink_bn_relu_pool_fwd / _bwd: y_pool = SumPool(relu(BN(x))) over the 2^3 children table; backward with dx and with dx = NULL
    (parameter gradients only).  The ReLU decisions are recomputed from x, so x is kept clear of z = 0."""
    L, check = _lib()
    g = torch.Generator().manual_seed(n_out + C)
    n, K = 8 * n_out - 5 if n_out > 1 else 3, 8
    in2out = (torch.arange(n) // 8).to(torch.int32)
    in2out = torch.minimum(in2out, torch.tensor(n_out - 1, dtype=torch.int32))
    nbr = torch.full((n_out, K), -1, dtype=torch.int32)
    for o in range(n_out):
        kids = torch.nonzero(in2out == o).flatten()[:K]
        nbr[o, torch.randperm(K, generator=g)[: len(kids)]] = kids.to(torch.int32)
    in2out = torch.full((n,), -1, dtype=torch.int32)
    for k in range(K):
        sel = nbr[:, k] >= 0
        in2out[nbr[sel, k].long()] = torch.nonzero(sel).flatten().to(torch.int32)
    assert int(in2out.min()) >= 0
    x = torch.randn(n, C, generator=g) * 2 + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    for _ in range(4):  # move the few elements whose pre-activation is within rounding of zero away from it
        m64, _, is64, z = _bn_fwd64(x, gamma, beta, None, False)
        near = z.abs() < 1e-3
        if not bool(near.any()):
            break
        x[near] += 0.05
    meanf, invf = m64.float(), is64.float()
    z = (x.double() - meanf.double()) * invf.double() * gamma.double() + beta.double()
    assert float(z.abs().min()) > 1e-4
    a = z.clamp_min(0)
    xg, mg, ig, gg, bg, ng, iog = (_gin(t, name=nm) for t, nm in ((x, "x"), (meanf, "mean"), (invf, "invstd"), (gamma, "gamma"), (beta, "beta"),
                                                                   (nbr, "nbr"), (in2out, "in2out")))
    y = _gout((n_out, C), name="y")
    check(L.mink_bn_relu_pool_fwd(xg.ptr, C, mg.ptr, ig.ptr, gg.ptr, bg.ptr, ng.ptr, n_out, K, y.ptr, _st()))
    _done(xg, mg, ig, gg, bg, ng, y)
    _close(y.t, LW.sum_pool(a, in2out, n_out), 1e-5, 1e-5, "bn_relu_pool_fwd y")  # (test_fused_bn_relu_sumpool)
    gp = torch.randn(n_out, C, generator=g)
    gy = gp[in2out.long()]
    dx64, _, dga64, dbe64 = _bn_bwd64(gy, x, a, meanf, invf, gamma, True)
    wsb = L.mink_bn_workspace_bytes(n, C)
    dpg, ws = _gin(gp, name="dy_pool"), _ws(wsb)
    dx = None if dx_null else _gout((n, C), name="dx")
    dga, dbe = _gout((C,), name="dgamma"), _gout((C,), name="dbeta")
    check(L.mink_bn_relu_pool_bwd(dpg.ptr, xg.ptr, n, C, mg.ptr, ig.ptr, gg.ptr, bg.ptr, iog.ptr, _ptr(dx), dga.ptr, dbe.ptr, ws.ptr, wsb, _st()))
    _done(dpg, xg, mg, ig, gg, bg, iog, dx, dga, dbe, ws)
    if dx is not None:
        _close(dx.t, dx64, 1e-5, 1e-4, "bn_relu_pool_bwd dx")
    _close(dga.t, dga64, 1e-3, 1e-4, "bn_relu_pool_bwd dgamma")
    _close(dbe.t, dbe64, 1e-3, 1e-4, "bn_relu_pool_bwd dbeta")


# ------------------------------------------------------------------------------------------------ the rest of the step
@pytest.mark.parametrize("n_out,C,ldx", [(1, 4, 8), (130, 48, 52), (257, 64, 64)])
def test_sum_pool_stays_inside_its_buffers(n_out, C, ldx):
    """mink_pool_sum_fwd (row pitch ldx > C) and _bwd."""
    L, check = _lib()
    g = torch.Generator().manual_seed(n_out + C)
    n, K = 5 * n_out + 3, 8
    in2out = torch.randint(0, n_out, (n,), generator=g, dtype=torch.int32)
    nbr = torch.full((n_out, K), -1, dtype=torch.int32)
    fill = torch.zeros(n_out, dtype=torch.long)
    for i in range(n):  # every input row is the child of at most one window, windows hold at most K
        o = int(in2out[i])
        if fill[o] < K:
            nbr[o, fill[o]] = i
            fill[o] += 1
    x = torch.randn(n, C, generator=g)
    ref = torch.zeros(n_out, C, dtype=torch.float64)
    for k in range(K):
        sel = nbr[:, k] >= 0
        ref[sel] += x[nbr[sel, k].long()].double()
    xg, ng, y = _gin(x, ld=ldx, name="x"), _gin(nbr, name="nbr"), _gout((n_out, C), name="y")
    check(L.mink_pool_sum_fwd(xg.ptr, ldx, C, ng.ptr, n_out, K, y.ptr, _st()))
    _done(xg, ng, y)
    _close(y.t, ref, 1e-5, 0.0, "pool_sum_fwd y")  # (test_relu_add_pool_globalavg)
    dy = torch.randn(n_out, C, generator=g)
    dg, ig, dx = _gin(dy, name="dy"), _gin(in2out, name="in2out"), _gout((n, C), name="dx")
    check(L.mink_pool_sum_bwd(dg.ptr, C, ig.ptr, n, dx.ptr, _st()))
    _done(dg, ig, dx)
    assert torch.equal(dx.t.cpu(), dy[in2out.long()])  # a copy


@pytest.mark.parametrize("n_out,C", [(1, 4), (130, 48), (257, 64)])
def test_max_pool_stays_inside_its_buffers(n_out, C):
    """mink_pool_max_fwd / _bwd (overlapping windows, the int32 `arg`)."""
    L, check = _lib()
    g = torch.Generator().manual_seed(n_out * 3 + C)
    n_in, K = n_out + 17, 9
    nbr = torch.randint(0, n_in, (n_out, K), generator=g, dtype=torch.int32)
    nbr[torch.rand(n_out, K, generator=g) < 0.45] = -1
    nbr[:, 0] = torch.randint(0, n_in, (n_out,), generator=g, dtype=torch.int32)  # (no empty window: its value is -inf)
    x = torch.randn(n_in, C, generator=g)
    cand = torch.where((nbr >= 0)[:, :, None], x[nbr.clamp_min(0).long()], torch.tensor(float("-inf")))
    ref, kbest = cand.max(1)
    xg, ng = _gin(x, name="x"), _gin(nbr, name="nbr")
    y, arg = _gout((n_out, C), name="y"), _gout((n_out, C), torch.int32, name="arg")
    check(L.mink_pool_max_fwd(xg.ptr, C, ng.ptr, n_out, K, y.ptr, arg.ptr, _st()))
    _done(xg, ng, y, arg)
    assert torch.equal(y.t.cpu(), ref)
    a = arg.t.cpu().long()
    assert int(a.min()) >= 0 and int(a.max()) < n_in and torch.equal(torch.gather(x, 0, a), ref)  # every arg names a row holding the maximum
    # backward through the transposed table: dx[i][c] = sum of dy[o][c] over the windows o of row i whose arg is i
    nbr_t = torch.full((n_in, K), -1, dtype=torch.int32)
    for k in range(K):
        sel = nbr[:, k] >= 0
        # (a row may sit in the same column of several windows: keep one table entry per (row, column), drop the others from arg's reach)
        nbr_t[nbr[sel, k].long(), k] = torch.nonzero(sel).flatten().to(torch.int32)
    dy = torch.randn(n_out, C, generator=g)
    ref_dx = torch.zeros(n_in, C, dtype=torch.float64)
    for k in range(K):
        o = nbr_t[:, k].long()
        ok = o >= 0
        hit = ok[:, None] & (a[o.clamp_min(0)] == torch.arange(n_in)[:, None])
        ref_dx += torch.where(hit, dy[o.clamp_min(0)].double(), torch.zeros((), dtype=torch.float64))
    dg, ag, tg, dx = _gin(dy, name="dy"), _gin(arg.t.cpu(), name="arg"), _gin(nbr_t, name="nbr_t"), _gout((n_in, C), name="dx")
    check(L.mink_pool_max_bwd(dg.ptr, ag.ptr, C, tg.ptr, n_in, K, dx.ptr, _st()))
    _done(dg, ag, tg, dx)
    _close(dx.t, ref_dx, 1e-6, 0.0, "pool_max_bwd dx")


@pytest.mark.parametrize("B,C,ncls", [(1, 4, 1), (3, 96, 130), (2, 2048, 51)])
def test_classifier_head_stays_inside_its_buffers(B, C, ncls):
    """mink_global_avg_fwd / _bwd and mink_head_forward / _backward with an empty sample; dx and dbias present and NULL."""
    L, check = _lib()
    g = torch.Generator().manual_seed(B * 100 + C + ncls)
    counts = torch.randint(1, 40, (B,), generator=g)
    if B > 1:
        counts[1] = 0
    boff = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).to(torch.int32)
    n = int(boff[-1])
    x = torch.randn(n, C, generator=g)
    w, bias = torch.randn(C, ncls, generator=g) * 0.05, torch.randn(ncls, generator=g) * 0.1
    pooled64 = torch.stack([x[boff[b]:boff[b + 1]].double().mean(0) if counts[b] > 0 else torch.zeros(C, dtype=torch.float64) for b in range(B)])
    xg, og, wg, bg = _gin(x, name="x"), _gin(boff, name="batch_offsets"), _gin(w, name="w"), _gin(bias, name="bias")
    ya = _gout((B, C), name="y")
    check(L.mink_global_avg_fwd(xg.ptr, C, og.ptr, B, ya.ptr, _st()))
    _done(xg, og, ya)
    _close(ya.t, pooled64, 1e-5, 0.0, "global_avg_fwd")
    dyb = torch.randn(B, C, generator=g)
    dg, dxa = _gin(dyb, name="dy"), _gout((n, C), name="dx")
    check(L.mink_global_avg_bwd(dg.ptr, C, og.ptr, B, n, dxa.ptr, _st()))
    _done(dg, og, dxa)
    rows_b = torch.repeat_interleave(torch.arange(B), counts)
    _close(dxa.t, dyb.double()[rows_b] / counts.double()[rows_b][:, None], 1e-6, 0.0, "global_avg_bwd")
    for with_bias in (True, False):
        pooled, logits = _gout((B, C), name="pooled"), _gout((B, ncls), name="logits")
        check(L.mink_head_forward(xg.ptr, og.ptr, B, C, wg.ptr, bg.ptr if with_bias else None, ncls, pooled.ptr, logits.ptr, _st()))
        _done(xg, og, wg, bg, pooled, logits)
        _close(pooled.t, pooled64, 1e-5, 0.0, "head pooled")
        l64 = pooled64 @ w.double() + (bias.double() if with_bias else 0.0)
        assert_finite(logits.t, "logits")
        assert float((logits.t.cpu().double() - l64).abs().max()) < 1e-5  # (test_classifier_head_matches_torch)
    dl = torch.randn(B, ncls, generator=g)
    dlg, pg = _gin(dl, name="dlogits"), _gin(pooled64.float(), name="pooled")
    dw64 = pooled64.float().double().t() @ dl.double()
    dx64 = (dl.double() @ w.double().t())[rows_b] / counts.double()[rows_b][:, None]
    for full in (True, False):
        dw, db, dx = _gout((C, ncls), name="dw"), (_gout((ncls,), name="dbias") if full else None), (_gout((n, C), name="dx") if full else None)
        check(L.mink_head_backward(dlg.ptr, pg.ptr, wg.ptr, og.ptr, B, C, ncls, dw.ptr, _ptr(db), _ptr(dx), _st()))
        _done(dlg, pg, wg, og, dw, db, dx)
        for got, want, name in ((dw, dw64, "dw"), (db, dl.double().sum(0), "db"), (dx, dx64, "dx")):
            if got is not None:
                assert_finite(got.t, name)
                err = float((got.t.cpu().double() - want).norm() / want.norm().clamp_min(1e-30))
                assert err < 1e-5, (name, err)


@pytest.mark.parametrize("B,ncls", [(1, 1), (5, 65), (257, 130), (5, 1), (1, 130), (257, 65)])
def test_softmax_cross_entropy_stays_inside_its_buffers(B, ncls):
    import torch.nn.functional as F

    L, check = _lib()
    g = torch.Generator().manual_seed(B + ncls)
    logits = torch.randn(B, ncls, generator=g) * 3
    labels = torch.randint(0, ncls, (B,), generator=g)
    lg, yg = _gin(logits, name="logits"), _gin(labels, name="labels")
    prob, loss = _gout((B, ncls), name="prob"), _gout((1,), name="loss")
    check(L.mink_softmax_ce_forward(lg.ptr, yg.ptr, B, ncls, prob.ptr, loss.ptr, _st()))
    _done(lg, yg, prob, loss)
    l64 = logits.double().requires_grad_()
    loss64 = F.cross_entropy(l64, labels)
    (3.0 * loss64).backward()
    _close(prob.t, torch.softmax(logits.double(), 1), 1e-6, 1e-5, "prob")
    assert abs(float(loss.t) - float(loss64)) < 1e-5  # (test_classifier_head_matches_torch)
    gl = _gin(torch.tensor([3.0]), name="grad_loss")
    pg, dl = _gin(torch.softmax(logits.double(), 1).float(), name="prob"), _gout((B, ncls), name="dlogits")
    check(L.mink_softmax_ce_backward(pg.ptr, yg.ptr, gl.ptr, B, ncls, dl.ptr, _st()))
    _done(pg, yg, gl, dl)
    assert_finite(dl.t, "dlogits")
    assert float((dl.t.cpu().double() - l64.grad).norm()) <= 1e-5 * float(l64.grad.norm()) + 1e-12


@pytest.mark.parametrize("n", [1, 65, 129])
@pytest.mark.parametrize("N,Kd", [(7, 4), (96, 64), (7, 64), (96, 4)])
def test_dense_xwt_stays_inside_its_buffers(n, N, Kd):
    L, check = _lib()
    g = torch.Generator().manual_seed(n + N + Kd)
    x, w = torch.randn(n, Kd, generator=g), torch.randn(N, Kd, generator=g) * 0.1
    xg, wg, y = _gin(x, name="x"), _gin(w, name="w"), _gout((n, N), name="y")
    check(L.mink_dense_xwt(xg.ptr, wg.ptr, n, Kd, N, y.ptr, _st()))
    _done(xg, wg, y)
    ref = x.double() @ w.double().t()
    assert_finite(y.t, "y")
    assert float((y.t.cpu().double() - ref).abs().max()) < 1e-5 * max(1.0, float(ref.abs().max()))  # (test_shortcut_data_gradient_pieces)


@pytest.mark.parametrize("n,C", [(1, 4), (37, 12), (513, 64)])
def test_rows_scatter_add_leaves_the_other_rows_alone(n, C):
    L, check = _lib()
    g = torch.Generator().manual_seed(n + C)
    n_dst = 3 * n + 5
    src, dst0 = torch.randn(n, C, generator=g), torch.randn(n_dst, C, generator=g)
    idx = torch.full((n,), -1, dtype=torch.int32)
    sel = torch.randperm(n, generator=g)[: (n + 1) // 2]
    idx[sel] = torch.randperm(n_dst, generator=g)[: sel.numel()].to(torch.int32)
    hit = torch.zeros(n_dst, dtype=torch.bool)
    hit[idx[sel].long()] = True
    sg, ig = _gin(src, name="src"), _gin(idx, name="idx")
    dst = _gout((n_dst, C), init=dst0, written=hit[:, None].expand(n_dst, C), name="dst")
    check(L.mink_rows_scatter_add(sg.ptr, ig.ptr, n, C, dst.ptr, _st()))
    _done(sg, ig, dst)
    want = dst0.clone()
    want[idx[sel].long()] += src[sel]
    assert torch.equal(dst.t.cpu(), want)  # (test_shortcut_data_gradient_pieces: exact)


@pytest.mark.parametrize("n_out,C,ldx", [(1, 3, 5), (65, 28, 32), (300, 64, 64)])
def test_segment_mean_and_sum_stay_inside_their_buffers(n_out, C, ldx):
    L, check = _lib()
    g = torch.Generator().manual_seed(n_out + C)
    cnt = torch.randint(1, 5, (n_out,), generator=g)
    seg = torch.cat([torch.zeros(1, dtype=torch.long), cnt.cumsum(0)]).to(torch.int32)
    n = int(seg[-1]) + 3  # (three rows no segment owns)
    members = torch.randperm(n, generator=g)[: int(seg[-1])].to(torch.int32)
    x = torch.randn(n, C, generator=g)
    owner = torch.repeat_interleave(torch.arange(n_out), cnt)
    s64 = torch.zeros(n_out, C, dtype=torch.float64).index_add_(0, owner, x[members.long()].double())
    xg, mg, sg = _gin(x, ld=ldx, name="x"), _gin(members, name="members"), _gin(seg, name="seg")
    for fn, ref, name in ((L.mink_segment_mean, s64 / cnt.double()[:, None], "segment_mean"), (L.mink_segment_sum, s64, "segment_sum")):
        y = _gout((n_out, C), name="y")
        check(fn(xg.ptr, ldx, C, mg.ptr, sg.ptr, n_out, y.ptr, _st()))
        _done(xg, mg, sg, y)
        _close(y.t, ref, 1e-6, 1e-6, name)  # (test_field_to_sparse_average: atol 1e-6 on O(1) means of <= 4 rows)


@pytest.mark.parametrize("count", [1, 3, 5, 1027])
def test_elementwise_kernels_stay_inside_their_buffers(count):
    """mink_eltwise (all three modes), mink_activation (leaky ReLU, PReLU with one and 24 slopes; forward and backward) at counts
    that are not multiples of the vector width, and mink_sgd_step."""
    L, check = _lib()
    g = torch.Generator().manual_seed(count)
    a, b = torch.randn(count, generator=g), torch.randn(count, generator=g)
    ag, bg = _gin(a, name="a"), _gin(b, name="b")
    for mode, ref in ((0, a.clamp_min(0)), (1, torch.where(b > 0, a, torch.zeros(()))), (2, a + b)):
        y = _gout((count,), name="y")
        check(L.mink_eltwise(ag.ptr, None if mode == 0 else bg.ptr, count, mode, y.ptr, _st()))
        _done(ag, bg, y)
        assert torch.equal(y.t.cpu(), ref), mode
    for C in (1, 24):
        rows = count
        x, gy = torch.randn(rows, C, generator=g), torch.randn(rows, C, generator=g)
        slope = torch.rand(C, generator=g) * 0.5
        xg, gg, sg = _gin(x, name="x"), _gin(gy, name="gy"), _gin(slope, name="slope")
        for kind, sl in ((1, None), (6, slope)):
            neg = 0.1 if sl is None else sl[None, :]
            for back in (False, True):
                out = _gout((rows, C), name="out")
                check(L.mink_activation(xg.ptr, gg.ptr if back else None, sg.ptr if kind == 6 else None, C, rows * C, kind, 0.1, out.ptr, _st()))
                _done(xg, gg, sg, out)
                d = torch.where(x > 0, torch.ones(()), neg * torch.ones_like(x))
                ref = gy * d if back else x * d
                _close(out.t, ref, 1e-6, 0.0, f"activation kind {kind}")  # (test_prelu_and_instance_norm_match_torch)
    n = (count + 3) // 4 * 4  # (flat buffers are padded to a multiple of four floats)
    w, gr, m = torch.randn(n, generator=g), torch.randn(n, generator=g), torch.randn(n, generator=g)
    for zero in (0, 1):
        wg, grg, mg = (_gout((n,), init=t, name=nm) for t, nm in ((w, "w"), (gr, "g"), (m, "m")))
        if not zero:
            grg.set_written(False)
        check(L.mink_sgd_step(wg.ptr, grg.ptr, mg.ptr, n, 0.1, 0.9, 1e-4, zero, _st()))
        _done(wg, grg, mg)
        g2 = gr.double() + 1e-4 * w.double()
        m2 = 0.9 * m.double() + g2
        for got, want, name in ((mg, m2, "m"), (wg, w.double() - 0.1 * m2, "w")):  # (test_flat_sgd_is_torch_sgd: one rounding per product and sum)
            assert_finite(got.t, name)
            assert float((got.t.cpu().double() - want).abs().max()) <= 1e-6 * float(want.abs().max()) + 1e-7, name
        assert torch.equal(grg.t.cpu(), torch.zeros(n) if zero else gr)
