"""Negative controls of tests/layerwise.py (no GPU): on a small synthetic scene with oracle-built tables, the CPU oracle's own
fp32 operators play the kernel.  The clean run passes every comparator at the bounds test_gpu_layerwise.py uses; each planted
fault -- the kinds of error a kernel at bench shapes could make -- is flagged by the check that is meant to catch it."""
import numpy as np
import pytest
import torch

import layerwise as LW
from helpers import batch_scenes


class Scene:
    """Level ts 1 (n rows) and ts 2, their tables (3^3 stride 1, 3^3 and 1^3 stride 2, transposed, class partition), and
    seeded fp32 operands with 16 channels."""

    def __init__(self):
        from oracle import maps

        maps.build()
        coords, _ = batch_scenes([3, 4], grid=14, cin=4)
        q = maps.quantize(coords.numpy())
        c1 = q[maps.unique(q)[0]]
        c2, i2o = maps.stride_map(c1, 2)
        self.n, self.n2 = c1.shape[0], c2.shape[0]
        self.nbr = maps.kernel_map_table(c1, c1, maps.kernel_offsets(3, 1))
        self.nbr_s = maps.kernel_map_table(c1, c2, maps.kernel_offsets(3, 1))
        self.nbr_d = maps.kernel_map_table(c1, c2, maps.kernel_offsets(1, 1))
        self.nbr_t = maps.transpose_table(self.nbr_s, self.n)
        self.perm = maps.class_partition(c1, 1, 16)
        self.i2o = i2o
        g = torch.Generator().manual_seed(5)
        self.x = torch.randn(self.n, 16, generator=g)
        self.w = torch.randn(27, 16, 16, generator=g) / 20
        self.wd = torch.randn(1, 16, 16, generator=g) / 4
        self.gy = torch.randn(self.n, 16, generator=g)
        self.gy2 = torch.randn(self.n2, 16, generator=g)
        self.gamma = 1 + 0.1 * torch.randn(16, generator=g)
        self.beta = 0.1 * torch.randn(16, generator=g)


@pytest.fixture(scope="module")
def sc():
    return Scene()


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def table(op, K, math):
    """The rounding table of a 64-wide Mink-ResNet14 mid layer (the block convolutions, a K = 1 strided shortcut) -- applied to
    this scene's 16-wide operands: these tests judge the comparators, tests/test_reduced_math_cpu.py the table itself."""
    return LW.rounded_operands(op, K, 64, 64, math, n_out=1000, row_perm=K == 1)


def oracle_conv(x, w, nbr, gy, rounded=None, rnd=LW.bf16_rne):
    """The oracle's fp32 convolution (oracle.me_cpu._ConvFn) as the "kernel": -> (y, dx, dw).  `rounded` = {op: operands}:
    what it rounds (with `rnd`) before its fp32 products, through oracle.me_cpu.OPERAND_HOOK."""
    from oracle import me_cpu as OME

    names = {"fwd_x": ("fwd", "x"), "fwd_w": ("fwd", "w"), "dgrad_g": ("dgrad", "dy"), "dgrad_w": ("dgrad", "w"),
             "wgrad_x": ("wgrad", "x"), "wgrad_g": ("wgrad", "dy")}

    def hook(t, role, shape):
        if role in names and names[role][1] in (rounded or {}).get(names[role][0], ()):
            return rnd(t)
        return t

    xr, wr = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
    OME.OPERAND_HOOK = hook if rounded else None
    try:
        y = OME._ConvFn.apply(xr, wr, nbr)
        y.backward(gy)
    finally:
        OME.OPERAND_HOOK = None
    return y.detach(), xr.grad, wr.grad


def conv_checks(sc, y, dx, dw, math="fp32", nbr=None, w=None):
    """Forward, data gradient and weight gradient of the stride-1 convolution against float64 on the declared rounding."""
    nbr_t = T(sc.nbr if nbr is None else nbr)
    w = sc.w if w is None else w
    recs = []
    for op, got, fn, ops in [
        ("fwd", y, lambda x, w: LW.conv_fwd(x, w, nbr_t), {"x": sc.x, "w": w}),
        ("dgrad", dx, lambda dy, w: LW.conv_dgrad(dy, w, nbr_t, sc.n), {"dy": sc.gy, "w": w}),
        ("wgrad", dw, lambda x, dy: LW.conv_wgrad(x, dy, nbr_t), {"x": sc.x, "dy": sc.gy}),
    ]:
        r = table(op, 27, math)
        other = frozenset() if r else frozenset(ops)
        recs += LW.check_conv("L", op, got, fn(**LW.apply_rounding(ops, r)), r, fn(**LW.apply_rounding(ops, other)))
    return recs


def failed(recs):
    return {r.op for r in recs if not r.ok}


@pytest.mark.parametrize("math", ["fp32", "bf16"])
def test_clean_convolution_passes(sc, math):
    rounded = {op: table(op, 27, math) for op in ("fwd", "dgrad", "wgrad")}
    y, dx, dw = oracle_conv(sc.x, sc.w, sc.nbr, sc.gy, rounded if math != "fp32" else None)
    recs = conv_checks(sc, y, dx, dw, math)
    assert not failed(recs), [r.line() for r in recs]
    # the rounding references are far enough apart for "declared vs other" to be asserted, not skipped
    assert all("too close" not in r.note for r in recs), [r.line() for r in recs]


def test_clean_reference_forms_agree(sc):
    """The kernels' gather forms of the data gradient (flip_k through the forward table; transposed table visited in class
    order) are the scatter through the forward table, and the oracle's strided data gradient matches them."""
    gy = sc.gy.double()
    a = LW.conv_dgrad(gy, sc.w, T(sc.nbr), sc.n)
    b = LW.conv_dgrad_gather(gy, sc.w, T(sc.nbr), flip_k=True)
    assert LW.conv_errors(b, a)[0] < 1e-13
    gy2 = sc.gy2.double()
    a = LW.conv_dgrad(gy2, sc.w, T(sc.nbr_s), sc.n)
    b = LW.conv_dgrad_gather(gy2, sc.w, T(sc.nbr_t), perm=T(sc.perm))
    assert LW.conv_errors(b, a)[0] < 1e-13
    _, dx, _ = oracle_conv(sc.x, sc.w, sc.nbr_s, sc.gy2)
    assert not failed(LW.check_conv("L", "strided dgrad", dx, a))


def _bn_kernel(y, gamma, beta, unbiased=False, relu=True, eps=1e-5):
    """fp32 training-mode batch norm as a kernel computes it: (mean, invstd, out, autograd backward closure)."""
    mean = y.mean(0)
    var = y.var(0, unbiased=unbiased)
    invstd = (var + eps).rsqrt()
    z = (y - mean) * invstd * gamma + beta
    return mean, invstd, (z.clamp_min(0) if relu else z)


def test_clean_norm_passes(sc):
    y = sc.x @ sc.w[13] + 0.3
    mean, invstd, h = _bn_kernel(y, sc.gamma, sc.beta)
    recs = LW.check_stats("L", "norm", mean, invstd, y)
    recs += LW.check_relu_out("L", "norm+relu", h, LW.bn_fwd(y, sc.gamma, sc.beta))
    # backward: fp32 autograd of the same operator, under its own ReLU decisions
    yr, ga, be = (t.clone().requires_grad_(True) for t in (y, sc.gamma, sc.beta))
    _, _, hh = _bn_kernel(yr, ga, be)
    hh.backward(sc.gy)
    recs += LW.check_bn_bwd("L", "norm bwd", yr.grad, ga.grad, be.grad, sc.gy, y, sc.gamma, sc.beta, h > 0)
    # pooling after the ReLU (the stem) and a bf16-stored value
    pooled = torch.zeros(sc.n2, 16).index_add_(0, T(sc.i2o).long(), h)
    ref = LW.sum_pool(LW.bn_fwd(y, sc.gamma, sc.beta).clamp_min(0), T(sc.i2o), sc.n2)
    recs += LW.check_scaled("L", "pool", pooled, ref, float(ref.abs().max()))
    recs += LW.check_bf16_store("L", "store", LW.bf16_rne(y), y.double())
    assert not failed(recs), [r.line() for r in recs]


# ---------------------------------------------------------------------------------------------------------- planted faults
def test_dropped_neighbour_is_flagged(sc):
    nbr = sc.nbr.copy()
    r = int(np.argmax((nbr >= 0).sum(1)))  # a row with every neighbour
    nbr[r, 4] = -1
    y, dx, dw = oracle_conv(sc.x, sc.w, nbr, sc.gy)
    assert {"fwd", "dgrad", "wgrad"} <= failed(conv_checks(sc, y, dx, dw))


def test_flipped_offset_weight_is_flagged(sc):
    w = sc.w.clone()
    w[3], w[23] = sc.w[23], sc.w[3]  # offset 3 read as K-1-3 (and back)
    y, dx, dw = oracle_conv(sc.x, w, sc.nbr, sc.gy)
    assert {"fwd", "dgrad"} <= failed(conv_checks(sc, y, dx, dw))  # (dW does not read the weights)


def test_missing_splitk_slab_is_flagged(sc):
    nbr = sc.nbr.copy()
    nbr[: sc.n // 8, 9:18] = -1  # slab 1 of 3 (offsets 9..17) lost for the first row tile
    y, _, _ = oracle_conv(sc.x, sc.w, nbr, sc.gy)
    _, dx, dw = oracle_conv(sc.x, sc.w, sc.nbr, sc.gy)
    assert "fwd" in failed(conv_checks(sc, y, dx, dw))


def test_bf16_truncation_is_flagged(sc):
    rounded = {op: table(op, 27, "bf16") for op in ("fwd", "dgrad", "wgrad")}
    y, dx, dw = oracle_conv(sc.x, sc.w, sc.nbr, sc.gy, rounded, rnd=LW.bf16_trunc)
    assert {"fwd", "dgrad", "wgrad"} <= failed(conv_checks(sc, y, dx, dw, "bf16"))


def test_rounding_table_mismatch_is_flagged(sc):
    # the kernel runs in exact fp32 where the table says it rounds ...
    y, dx, dw = oracle_conv(sc.x, sc.w, sc.nbr, sc.gy)
    f = failed(conv_checks(sc, y, dx, dw, "bf16"))
    assert {"fwd", "fwd vs other", "dgrad vs other", "wgrad vs other"} <= f
    # ... or rounds where the table says it does not (the 1x1x1 shortcut's data gradient is exact fp32)
    gd = LW.bf16_rne(sc.gy2) @ LW.bf16_rne(sc.wd[0]).t()
    ops = {"dy": sc.gy2, "w": sc.wd}
    r = table("dgrad", 1, "bf16")
    assert r == frozenset()
    fn = lambda dy, w: dy @ w[0].t()  # noqa: E731
    recs = LW.check_conv("L", "down dgrad", gd, fn(**LW.apply_rounding(ops, r)), r, fn(**LW.apply_rounding(ops, {"dy", "w"})))
    assert {"down dgrad", "down dgrad vs other"} <= failed(recs)


def test_unbiased_variance_is_flagged(sc):
    y = sc.x @ sc.w[13] + 0.3
    mean, invstd, h = _bn_kernel(y, sc.gamma, sc.beta, unbiased=True)
    assert "norm invstd" in failed(LW.check_stats("L", "norm", mean, invstd, y))
    assert "norm+relu" in failed(LW.check_relu_out("L", "norm+relu", h, LW.bn_fwd(y, sc.gamma, sc.beta)))


def test_flipped_relu_branch_is_flagged(sc):
    y = sc.x @ sc.w[13] + 0.3
    _, _, h = _bn_kernel(y, sc.gamma, sc.beta)
    h = h.clone()
    h.view(-1)[int(h.argmax())] = 0.0  # the largest activation's branch taken the wrong way
    recs = LW.check_relu_out("L", "norm+relu", h, LW.bn_fwd(y, sc.gamma, sc.beta))
    assert "norm+relu flips" in failed(recs)
    # and a backward under a wrong mask element where |z| is large
    z = LW.bn_fwd(y, sc.gamma, sc.beta)
    yr, ga, be = (t.clone().requires_grad_(True) for t in (y, sc.gamma, sc.beta))
    _, _, hh = _bn_kernel(yr, ga, be)
    hh.backward(sc.gy * (h > 0))
    assert failed(LW.check_bn_bwd("L", "norm bwd", yr.grad, ga.grad, be.grad, sc.gy, y, sc.gamma, sc.beta, z > 0))


def test_class_permutation_off_by_one_is_flagged(sc):
    gy2 = sc.gy2.double()
    ref = LW.conv_dgrad(gy2, sc.w, T(sc.nbr_s), sc.n)
    good = LW.conv_dgrad_gather(gy2, sc.w, T(sc.nbr_t), perm=T(sc.perm)).float()
    p = T(sc.perm)
    p = p[p >= 0].long()
    bad = torch.empty_like(good)
    bad[p] = good[p.roll(-1)]  # slot j of the class order writes row perm[j] with what belongs to perm[j + 1]
    assert not failed(LW.check_conv("L", "strided dgrad", good, ref))
    assert "strided dgrad" in failed(LW.check_conv("L", "strided dgrad", bad, ref))
