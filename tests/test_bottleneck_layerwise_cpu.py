"""Negative controls of the Bottleneck, running-statistics and eval-mode checks of tests/test_gpu_bottleneck_layerwise.py (no
GPU): on a small two-level scene with oracle-built tables (1^3 stride 2 for the shortcut) the CPU oracle's fp32 operators and
torch's own fp32 batch norm play the kernels.  The clean run passes every comparator; each planted fault -- the kinds of error
a batch-norm, pointwise or residual kernel of these networks could make -- is flagged by the check meant to catch it."""
import pytest
import torch

import layerwise as LW
from helpers import batch_scenes
from test_layerwise_cpu import T, failed, oracle_conv

EPS, MOM = 1e-5, 0.1


class Scene:
    """Levels ts 1 (n rows) and ts 2, the 1x1 stride-2 shortcut table, and seeded fp32 operands."""

    def __init__(self):
        from oracle import maps

        maps.build()
        coords, _ = batch_scenes([5, 6], grid=14, cin=4)
        q = maps.quantize(coords.numpy())
        c1 = q[maps.unique(q)[0]]
        c2, _ = maps.stride_map(c1, 2)
        self.n, self.n2 = c1.shape[0], c2.shape[0]
        self.nbr_d = maps.kernel_map_table(c1, c2, maps.kernel_offsets(1, 1))  # [n2, 1]
        g = torch.Generator().manual_seed(11)
        self.x = torch.randn(self.n, 24, generator=g)  # block input, 24 channels
        self.wp = torch.randn(24, 40, generator=g) / 5  # conv1 (1x1): 24 -> 40 (cin != cout)
        self.wd = torch.randn(1, 24, 32, generator=g) / 5  # shortcut (1x1, stride 2): 24 -> 32
        self.gy = torch.randn(self.n, 40, generator=g)
        self.gy2 = torch.randn(self.n2, 32, generator=g)
        self.y = 0.3 * torch.randn(self.n, 32, generator=g) + 0.1  # what a norm normalises
        self.res = torch.randn(self.n, 32, generator=g)
        self.y2k = 0.5 * torch.randn(300, 2048, generator=g) + torch.linspace(-1, 1, 2048)  # a 2048-channel norm's input


@pytest.fixture(scope="module")
def sc():
    return Scene()


def _bn(C, seed=91):
    """An nn.BatchNorm1d with running statistics far from (0, 1) (layerwise.far_running_stats, as the GPU test seeds them)."""
    bn = torch.nn.BatchNorm1d(C, eps=EPS, momentum=MOM)
    LW.far_running_stats(bn, seed)
    return bn


def _conv(layer, op, got, fn, ops):
    """check_conv on fp32 math, every operand rounded to bf16 as the discriminator (as the GPU test does)."""
    return LW.check_conv(layer, op, got, fn(**LW.apply_rounding(ops, frozenset())), frozenset(), fn(**LW.apply_rounding(ops, set(ops))))


# ---------------------------------------------------------------------------------------------------------- running statistics
def _train_pass(bn, y):
    """One training pass of torch's fp32 batch norm (the kernel's stand-in): -> (the snapshot before it, its output)."""
    before = LW.running_snapshot(bn)[bn]
    bn.train()
    with torch.no_grad():
        out = bn(y)
    return before, out


def _running(bn, before, y):
    return failed(LW.check_running("norm", before, bn, y))


def test_clean_running_statistics_pass(sc):
    bn = _bn(32)
    before, _ = _train_pass(bn, sc.y)
    assert not _running(bn, before, sc.y)
    # two passes, one counter step each
    first = LW.running_snapshot(bn)[bn]
    _train_pass(bn, sc.y)
    assert not failed(LW.check_running("norm", first, bn, sc.y))
    assert int(bn.num_batches_tracked) == int(before[3]) + 2


def _planted_update(bn, before, y, biased=False, swap=False, skip=False, steps=1):
    _, r0, v0, t0 = before
    n = y.shape[0]
    mean, var = y.double().mean(0), y.double().var(0, unbiased=False)
    if not biased:
        var = var * n / (n - 1)
    keep, mom = (MOM, 1 - MOM) if swap else (1 - MOM, MOM)
    with torch.no_grad():
        if not skip:
            bn.running_mean.copy_((keep * r0.double() + mom * mean).float())
            bn.running_var.copy_((keep * v0.double() + mom * var).float())
        bn.num_batches_tracked.copy_(t0 + steps)


def test_running_var_with_the_biased_variance_is_flagged(sc):
    bn = _bn(32)
    before = LW.running_snapshot(bn)[bn]
    _planted_update(bn, before, sc.y)
    assert not _running(bn, before, sc.y)  # (the planted update itself, unbiased, passes)
    _planted_update(bn, before, sc.y, biased=True)
    assert _running(bn, before, sc.y) == {"running var"}


def test_biased_variance_is_flagged_where_the_running_var_dwarfs_the_batchs():
    """Bench shapes: a low-variance norm (var(y) ~ 0.03, a 3^3 convolution's output at this repository's init) at n = 512 rows
    (layer 4) after two passes from running_var = 1 (~0.82): the biased variance moves the update by 0.1 var / 511, under
    1e-5 of running_var but 20 times NORM_BOUND var(y)."""
    g = torch.Generator().manual_seed(12)
    y = 0.17 * torch.randn(512, 64, generator=g) + 0.05
    bn = torch.nn.BatchNorm1d(64, eps=EPS, momentum=MOM)
    with torch.no_grad():
        bn.running_var.fill_(0.82), bn.running_mean.fill_(0.03)
    before, _ = _train_pass(bn, y)  # torch's own fp32 update
    assert not _running(bn, before, y)
    _planted_update(bn, before, y)
    assert not _running(bn, before, y)
    _planted_update(bn, before, y, biased=True)
    assert _running(bn, before, y) == {"running var"}


def test_swapped_momentum_is_flagged(sc):
    bn = _bn(32)
    before = LW.running_snapshot(bn)[bn]
    _planted_update(bn, before, sc.y, swap=True)
    assert {"running mean", "running var"} <= _running(bn, before, sc.y)


def test_skipped_running_update_is_flagged(sc):
    bn = _bn(32)
    before = LW.running_snapshot(bn)[bn]
    _planted_update(bn, before, sc.y, skip=True)
    assert {"running mean", "running var"} <= _running(bn, before, sc.y)
    _planted_update(bn, before, sc.y, steps=0)  # statistics moved, the counter did not
    assert _running(bn, before, sc.y) == {"batches tracked"}


# ---------------------------------------------------------------------------------------------------------- eval mode
def _eval_checks(bn, y, got, relu=True):
    z = LW.bn_eval_fwd(y, bn.running_mean, bn.running_var, bn.weight.detach(), bn.bias.detach(), eps=bn.eps)
    return LW.check_relu_out("norm", "eval norm+relu fwd", got, z) if relu else LW.check_scaled("norm", "eval norm fwd", got, z, float(z.abs().max()))


def _eval_kernel(bn, y, training=False, eps=EPS):
    """torch's fp32 batch norm on the running statistics (or, planted, on the batch's / without eps)."""
    with torch.no_grad():
        if eps == 0.0:  # (torch refuses eps = 0: the same affine map by hand, in fp32)
            return (y - bn.running_mean) * bn.running_var.rsqrt() * bn.weight + bn.bias
        return torch.nn.functional.batch_norm(y, bn.running_mean.clone(), bn.running_var.clone(), bn.weight, bn.bias, training,
                                              0.0, eps)


def test_clean_eval_norm_passes_and_keeps_the_running_statistics(sc):
    bn = _bn(32)
    bn.eval()
    before = LW.running_snapshot(bn)
    with torch.no_grad():
        out = bn(sc.y).clamp_min(0)
    assert not failed(_eval_checks(bn, sc.y, out))
    assert not failed(LW.check_running_unchanged(before, bn))
    bn.train()
    with torch.no_grad():
        bn(sc.y)
    assert failed(LW.check_running_unchanged(before, bn)) == {"running stats kept"}


def test_eval_with_batch_statistics_is_flagged(sc):
    bn = _bn(32)
    assert "eval norm fwd" in failed(_eval_checks(bn, sc.y, _eval_kernel(bn, sc.y, training=True), relu=False))
    assert "eval norm+relu fwd" in failed(_eval_checks(bn, sc.y, _eval_kernel(bn, sc.y, training=True).clamp_min(0)))


def test_eval_without_eps_is_flagged(sc):
    bn = _bn(32)
    assert not failed(_eval_checks(bn, sc.y, _eval_kernel(bn, sc.y), relu=False))
    assert "eval norm fwd" in failed(_eval_checks(bn, sc.y, _eval_kernel(bn, sc.y, eps=0.0), relu=False))


# ---------------------------------------------------------------------------------------------------------- pointwise / blocks
def _pointwise_checks(sc, y, dw):
    return (_conv("conv1", "pointwise fwd", y, lambda x, w: LW.pointwise_fwd(x, w), {"x": sc.x, "w": sc.wp})
            + _conv("conv1", "pointwise wgrad", dw, lambda x, dy: LW.pointwise_wgrad(x, dy), {"x": sc.x, "dy": sc.gy}))


def test_clean_pointwise_passes(sc):
    assert not failed(_pointwise_checks(sc, sc.x @ sc.wp, sc.x.t() @ sc.gy))


def test_transposed_pointwise_weight_is_flagged(sc):
    """[cin, cout] weights read as if stored [cout, cin] (and the weight gradient written that way)."""
    cin, cout = sc.wp.shape
    assert cin != cout
    wt = sc.wp.reshape(cout, cin).t()
    gw = (sc.gy.t() @ sc.x).reshape(cin, cout)
    assert {"pointwise fwd", "pointwise wgrad"} <= failed(_pointwise_checks(sc, sc.x @ wt, gw))


def _block_input_grad(sc, with_shortcut=True):
    """The gradient of a strided Bottleneck's input: conv1's (1x1) data gradient + the 1x1 stride-2 shortcut's, scattered onto
    the rows it reaches -- the kernel's sum, and the float64 sum of the two shares."""
    _, dx_sc, _ = oracle_conv(sc.x, sc.wd, sc.nbr_d, sc.gy2)
    got = sc.gy @ sc.wp.t() + (dx_sc if with_shortcut else 0)
    ref = LW.pointwise_dgrad(sc.gy, sc.wp) + LW.conv_dgrad(sc.gy2, sc.wd, T(sc.nbr_d), sc.n)
    return LW.check_conv("block", "grad = conv1 dgrad + downsample dgrad", got, ref)


def test_block_input_gradient_missing_the_shortcut_share_is_flagged(sc):
    assert not failed(_block_input_grad(sc))
    assert "grad = conv1 dgrad + downsample dgrad" in failed(_block_input_grad(sc, with_shortcut=False))


def _norm3(sc, got):
    bn = _bn(32)
    return LW.check_relu_out("norm3", "norm+res+relu fwd", got, LW.bn_fwd(sc.y, bn.weight.detach(), bn.bias.detach(), sc.res)), bn


def test_residual_added_before_norm3_is_flagged(sc):
    _, bn = _norm3(sc, torch.zeros(sc.n, 32))
    bn.train()
    with torch.no_grad():
        right = (bn(sc.y) + sc.res).clamp_min(0)
        wrong = bn(sc.y + sc.res).clamp_min(0)
    assert not failed(_norm3(sc, right)[0])
    assert "norm+res+relu fwd" in failed(_norm3(sc, wrong)[0])


def test_second_slab_of_a_2048_channel_norm_with_the_first_slabs_statistics_is_flagged(sc):
    y = sc.y2k
    mean = y.mean(0)
    invstd = (y.var(0, unbiased=False) + EPS).rsqrt()
    assert not failed(LW.check_stats("layer4", "norm", mean, invstd, y))
    bad_m, bad_is = mean.clone(), invstd.clone()
    bad_m[1024:], bad_is[1024:] = mean[:1024], invstd[:1024]
    assert {"norm mean", "norm invstd"} <= failed(LW.check_stats("layer4", "norm", bad_m, bad_is, y))
    gamma, beta = torch.ones(2048), torch.zeros(2048)
    z = LW.bn_fwd(y, gamma, beta)
    got = (y - bad_m) * bad_is
    assert "norm fwd" in failed(LW.check_scaled("layer4", "norm fwd", got, z, float(z.abs().max())))
