"""Negative controls of the segmentation references of tests/layerwise.py (no GPU), which tests/test_gpu_seg_layerwise.py
holds Res16UNet to: on a small two-level scene with oracle-built tables (3^3 stride 1, 2^3 stride 2, its transpose, the
class partition) the CPU oracle's own fp32 operators play the kernel.  The clean run passes every comparator; each planted
fault -- the kinds of error a kernel, a planner or a map builder of the segmentation network could make -- is flagged by the
check that is meant to catch it."""
import numpy as np
import pytest
import torch

import layerwise as LW
from helpers import batch_scenes
from test_layerwise_cpu import T, failed, oracle_conv


class Scene:
    """Levels ts 1 (n rows, with duplicate field rows) and ts 2, their tables, and seeded fp32 operands."""

    def __init__(self):
        from oracle import maps

        maps.build()
        coords, _ = batch_scenes([3, 4], grid=14, cin=4)
        g = torch.Generator().manual_seed(7)
        dup = torch.randint(0, coords.shape[0], (coords.shape[0] // 4,), generator=g)
        self.fcoords = torch.cat([coords, coords[dup]]) + torch.cat([torch.zeros(coords.shape[0] + dup.numel(), 1),
                                                                     0.9 * torch.rand(coords.shape[0] + dup.numel(), 3, generator=g)], 1)
        q = maps.quantize(self.fcoords.numpy())
        ui, inv = maps.unique(q)
        c1 = q[ui]
        c2, _ = maps.stride_map(c1, 2)
        self.n, self.n2 = c1.shape[0], c2.shape[0]
        self.inv = inv
        self.nbr = maps.kernel_map_table(c1, c1, maps.kernel_offsets(3, 1))
        self.nbr2 = maps.kernel_map_table(c1, c2, maps.kernel_offsets(2, 1))  # fine -> coarse, [n2, 8]
        self.nbr2_t = maps.transpose_table(self.nbr2, self.n)  # [n, 8]: one live offset per fine row
        self.perm = maps.class_partition(c1, 1, 16)
        self.f = torch.randn(self.fcoords.shape[0], 3, generator=g)  # field features (3 colours)
        self.x = torch.randn(self.n, 16, generator=g)
        self.x2 = torch.randn(self.n2, 24, generator=g)
        self.w = torch.randn(27, 16, 16, generator=g) / 20
        self.w3 = torch.randn(27, 3, 16, generator=g) / 5
        self.wd = torch.randn(8, 16, 24, generator=g) / 10  # down: 16 -> 24
        self.wt = torch.randn(8, 24, 16, generator=g) / 10  # up: 24 -> 16
        self.wp = torch.randn(32, 20, generator=g) / 6  # 1x1: 32 -> 20, with bias
        self.bias = torch.randn(1, 20, generator=g) / 6
        self.gy = torch.randn(self.n, 16, generator=g)
        self.gy2 = torch.randn(self.n2, 24, generator=g)
        self.gl = torch.randn(self.fcoords.shape[0], 20, generator=g)
        self.gamma = 1 + 0.1 * torch.randn(16, generator=g)
        self.beta = 0.1 * torch.randn(16, generator=g)


@pytest.fixture(scope="module")
def sc():
    return Scene()


def _conv(layer, op, got, fn, ops):
    """check_conv on fp32 math, every operand rounded to bf16 as the discriminator (as the GPU test does)."""
    return LW.check_conv(layer, op, got, fn(**LW.apply_rounding(ops, frozenset())), frozenset(), fn(**LW.apply_rounding(ops, set(ops))))


def tconv_checks(sc, y, dx, dw, nbr2=None, w=None):
    nbr2 = T(sc.nbr2 if nbr2 is None else nbr2)
    w = sc.wt if w is None else w
    return (_conv("up", "tconv fwd", y, lambda x, w: LW.tconv_fwd(x, w, nbr2, sc.n), {"x": sc.x2, "w": w})
            + _conv("up", "tconv dgrad", dx, lambda dy, w: LW.tconv_dgrad(dy, w, nbr2), {"dy": sc.gy, "w": w})
            + _conv("up", "tconv wgrad", dw, lambda x, dy: LW.tconv_wgrad(x, dy, nbr2), {"x": sc.x2, "dy": sc.gy}))


def down_checks(sc, y, dx, dw):
    nbr2 = T(sc.nbr2)
    return (_conv("down", "conv fwd", y, lambda x, w: LW.conv_fwd(x, w, nbr2), {"x": sc.x, "w": sc.wd})
            + _conv("down", "dgrad", dx, lambda dy, w: LW.conv_dgrad(dy, w, nbr2, sc.n), {"dy": sc.gy2, "w": sc.wd})
            + _conv("down", "conv wgrad", dw, lambda x, dy: LW.conv_wgrad(x, dy, nbr2), {"x": sc.x, "dy": sc.gy2}))


def oracle_tconv(sc, w=None, nbr2_t=None):
    """The oracle's transposed convolution (me_cpu.MinkowskiConvolutionTranspose: its convolution through the transposed
    table) as the kernel."""
    return oracle_conv(sc.x2, sc.wt if w is None else w, sc.nbr2_t if nbr2_t is None else nbr2_t, sc.gy)


def _pointwise_kernel(sc, x, bias=True):
    xr, wr, br = x.clone().requires_grad_(True), sc.wp.clone().requires_grad_(True), sc.bias.clone().requires_grad_(True)
    y = xr @ wr + (br if bias else 0)
    y.backward(sc.gl[: x.shape[0]])
    return y.detach(), xr.grad, wr.grad, torch.zeros_like(sc.bias) if br.grad is None else br.grad


def _pointwise_checks(sc, x, y, dx, dw, db):
    g = sc.gl[: x.shape[0]]
    ref = LW.bias_grad(g)
    return (_conv("final", "pointwise fwd + bias", y, lambda x, w: LW.pointwise_fwd(x, w, sc.bias), {"x": x, "w": sc.wp})
            + _conv("final", "pointwise dgrad", dx, lambda dy, w: LW.pointwise_dgrad(dy, w), {"dy": g, "w": sc.wp})
            + _conv("final", "pointwise wgrad", dw, lambda x, dy: LW.pointwise_wgrad(x, dy), {"x": x, "dy": g})
            + LW.check_scaled("final", "bias grad", db, ref, LW.reduction_scale(g)))


def _oracle_field(sc):
    from oracle import me_cpu as OME

    return OME.TensorField(coordinates=sc.fcoords, features=sc.f)


# ---------------------------------------------------------------------------------------------------------- clean run
def test_clean_segmentation_operators_pass(sc):
    recs = tconv_checks(sc, *oracle_tconv(sc))
    recs += down_checks(sc, *oracle_conv(sc.x, sc.wd, sc.nbr2, sc.gy2))
    # the strided data gradient in the kernels' form: transposed table in class order
    a = LW.conv_dgrad(sc.gy2.double(), sc.wd, T(sc.nbr2), sc.n)
    assert LW.conv_errors(LW.conv_dgrad_gather(sc.gy2.double(), sc.wd, T(sc.nbr2_t), perm=T(sc.perm)), a)[0] < 1e-13
    # 1x1 classifier with bias
    xp = torch.cat([sc.x, sc.x * 0.5], 1)
    recs += _pointwise_checks(sc, xp, *_pointwise_kernel(sc, xp))
    # cat, .sparse(), slice()
    h = torch.randn(sc.n, 8)
    recs += LW.check_scaled("b8", "cat fwd", torch.cat([sc.x, h], 1), LW.cat_fwd(sc.x, h), 1.0, bound=0.0)
    ga, gb = LW.cat_bwd(torch.cat([sc.gy, sc.gy[:, :8]], 1), (16, 8))
    recs += LW.check_scaled("b8", "cat bwd", torch.cat([ga, gb], 1), torch.cat([sc.gy, sc.gy[:, :8]], 1).double(), 1.0, bound=0.0)
    tf = _oracle_field(sc)
    xs = tf.sparse()
    assert xs.F.shape[0] == sc.n < sc.fcoords.shape[0]
    ref = LW.sparse_mean(sc.f, T(sc.inv), sc.n)
    recs += LW.check_scaled("field", ".sparse() fwd", xs.F, ref, float(ref.abs().max()))
    y = torch.randn(sc.n, 20)
    inv = T(sc.inv).long()
    recs += LW.check_scaled("field", "slice() fwd", y[inv], LW.slice_fwd(y, T(sc.inv)), 1.0, bound=0.0)
    yr = y.clone().requires_grad_(True)
    yr[inv].backward(sc.gl)
    ref = LW.slice_bwd(sc.gl, T(sc.inv), sc.n)
    recs += LW.check_scaled("field", "slice() bwd", yr.grad, ref, float(ref.abs().max()))
    # the padded stem: input of 3 channels, one zero column added for the kernel, its weight gradient sliced back
    x3 = sc.f[: sc.n]
    x4, w4 = torch.nn.functional.pad(x3, (0, 1)), torch.nn.functional.pad(sc.w3, (0, 0, 0, 1))
    _, _, dw4 = oracle_conv(x4, w4, sc.nbr, sc.gy)
    recs += _conv("stem", "conv wgrad", dw4[:, :3], lambda x, dy: LW.conv_wgrad(x, dy, T(sc.nbr)), {"x": x3, "dy": sc.gy})
    # composite: a block input's gradient = conv1's data gradient + the residual's share
    res = torch.randn(sc.n, 16)
    _, dx, _ = oracle_conv(sc.x, sc.w, sc.nbr, sc.gy)
    recs += LW.check_conv("b1", "grad = conv1 dgrad + residual", dx + res,
                          LW.conv_dgrad(sc.gy, sc.w, T(sc.nbr), sc.n) + res.double())
    # eval-mode norm (running statistics) and the loss gradient
    y = sc.x @ sc.w[13]
    rm, rv = 0.1 * torch.randn(16), 0.5 + torch.rand(16)
    z = (y - rm) / torch.sqrt(rv + 1e-5) * sc.gamma + sc.beta
    recs += LW.check_relu_out("b1", "norm+relu fwd (eval)", z.clamp_min(0), LW.bn_eval_fwd(y, rm, rv, sc.gamma, sc.beta))
    logits = torch.randn(sc.fcoords.shape[0], 20).requires_grad_(True)
    labels = torch.randint(0, 20, (logits.shape[0],))
    labels[::7] = -100
    torch.nn.functional.cross_entropy(logits, labels, ignore_index=-100).backward()
    ref = LW.cross_entropy_grad(logits.detach(), labels)
    recs += LW.check_scaled("loss", "cross entropy dlogits", logits.grad, ref, float(ref.abs().max()))
    assert not failed(recs), [r.line() for r in recs if not r.ok]
    assert all("too close" not in r.note for r in recs), [r.line() for r in recs if "too close" in r.note]


def test_reference_forms_of_the_transposed_convolution_agree(sc):
    """tconv_* (scatter / gather through the fine -> coarse table) are the ordinary convolution through the transposed table,
    and tconv_dgrad is the data gradient of the fine -> coarse convolution with the weights read as [K, cout, cin]."""
    x2, gy = sc.x2.double(), sc.gy.double()
    a = LW.tconv_fwd(x2, sc.wt, T(sc.nbr2), sc.n)
    assert LW.conv_errors(LW.conv_fwd(x2, sc.wt, T(sc.nbr2_t)), a)[0] < 1e-13
    b = LW.tconv_dgrad(gy, sc.wt, T(sc.nbr2))
    assert LW.conv_errors(LW.conv_dgrad(gy, sc.wt, T(sc.nbr2_t), sc.n2), b)[0] < 1e-13
    c = LW.tconv_wgrad(x2, gy, T(sc.nbr2))
    assert LW.conv_errors(LW.conv_wgrad(x2, gy, T(sc.nbr2_t)), c)[0] < 1e-13
    assert ((sc.nbr2_t >= 0).sum(1) == 1).all()  # kernel size == stride: one parent per fine row


# ---------------------------------------------------------------------------------------------------------- planted faults
def test_mirrored_transposed_offsets_are_flagged(sc):
    y, dx, dw = oracle_tconv(sc, w=sc.wt.flip(0))  # table column k multiplied by the weights of offset 7 - k ...
    f = failed(tconv_checks(sc, y, dx, dw.flip(0)))  # ... and its pairs' weight gradient written there
    assert {"tconv fwd", "tconv dgrad", "tconv wgrad"} <= f


def test_permutation_class_shifted_by_one_row_is_flagged(sc):
    """The transposed forward written in class order (slot j of the permutation -> row perm[j]): one class's slots shifted
    by one row."""
    y, dx, dw = oracle_tconv(sc)
    p = T(sc.perm).long()
    cls = [p[j : j + 16] for j in range(0, p.numel(), 16)]
    seg = next(c[c >= 0] for c in cls if int((c >= 0).sum()) > 4)
    bad = y.clone()
    bad[seg] = y[seg.roll(-1)]
    assert not failed(tconv_checks(sc, y, dx, dw))
    assert "tconv fwd" in failed(tconv_checks(sc, bad, dx, dw))


def test_dropped_offset_of_a_stride2_table_is_flagged(sc):
    nbr2 = sc.nbr2.copy()
    r = int(np.argmax((nbr2 >= 0).sum(1)))
    k = int(np.nonzero(nbr2[r] >= 0)[0][0])
    nbr2[r, k] = -1
    assert {"conv fwd", "dgrad", "conv wgrad"} <= failed(down_checks(sc, *oracle_conv(sc.x, sc.wd, nbr2, sc.gy2)))
    # ... and the transposed convolution through the transposed table of the damaged one
    from oracle import maps

    y, dx, dw = oracle_tconv(sc, nbr2_t=maps.transpose_table(nbr2, sc.n))
    assert {"tconv fwd", "tconv dgrad", "tconv wgrad"} <= failed(tconv_checks(sc, y, dx, dw))


def test_swapped_cat_halves_are_flagged(sc):
    h = torch.randn(sc.n, 16)
    assert "cat fwd" in failed(LW.check_scaled("b8", "cat fwd", torch.cat([h, sc.x], 1), LW.cat_fwd(sc.x, h), 1.0, bound=0.0))
    ga, gb = LW.cat_bwd(torch.cat([sc.gy, sc.gy * 2], 1), (16, 16))
    assert failed(LW.check_scaled("b8", "cat bwd", gb, (sc.gy * 2).double(), 1.0, bound=0.0)) == set()
    assert "cat bwd" in failed(LW.check_scaled("b8", "cat bwd", ga, (sc.gy * 2).double(), 1.0, bound=0.0))


def test_dropped_bias_is_flagged(sc):
    xp = torch.cat([sc.x, sc.x * 0.5], 1)
    y, dx, dw, db = _pointwise_kernel(sc, xp, bias=False)
    assert "pointwise fwd + bias" in failed(_pointwise_checks(sc, xp, y, dx, dw, db))
    assert "bias grad" in failed(_pointwise_checks(sc, xp, y, dx, dw, torch.zeros_like(sc.bias)))


def test_slice_off_by_one_row_is_flagged(sc):
    y = torch.randn(sc.n, 20)
    inv = T(sc.inv).long()
    assert "slice() fwd" in failed(LW.check_scaled("field", "slice() fwd", y[(inv + 1) % sc.n], LW.slice_fwd(y, T(sc.inv)), 1.0,
                                                   bound=0.0))
    got = torch.zeros(sc.n, 20).index_add_(0, (inv + 1) % sc.n, sc.gl)
    ref = LW.slice_bwd(sc.gl, T(sc.inv), sc.n)
    assert "slice() bwd" in failed(LW.check_scaled("field", "slice() bwd", got, ref, float(ref.abs().max())))


def test_padded_stem_channel_kept_is_flagged(sc):
    x3 = sc.f[: sc.n]
    x4, w4 = torch.nn.functional.pad(x3, (0, 1)), torch.nn.functional.pad(sc.w3, (0, 0, 0, 1))
    _, _, dw4 = oracle_conv(x4, w4, sc.nbr, sc.gy)
    recs = _conv("stem", "conv wgrad", dw4, lambda x, dy: LW.conv_wgrad(x, dy, T(sc.nbr)), {"x": x3, "dy": sc.gy})
    assert "conv wgrad" in failed(recs) and "shape" in recs[0].note


def test_composite_missing_its_residual_share_is_flagged(sc):
    res = torch.randn(sc.n, 16)
    _, dx, _ = oracle_conv(sc.x, sc.w, sc.nbr, sc.gy)
    ref = LW.conv_dgrad(sc.gy, sc.w, T(sc.nbr), sc.n) + res.double()
    assert "grad = conv1 dgrad + residual" in failed(LW.check_conv("b1", "grad = conv1 dgrad + residual", dx, ref))


def test_sparse_without_averaging_is_flagged(sc):
    """.sparse() that keeps the first row of each voxel instead of the mean of its rows."""
    from oracle import maps

    ui, _ = maps.unique(maps.quantize(sc.fcoords.numpy()))
    ref = LW.sparse_mean(sc.f, T(sc.inv), sc.n)
    assert ".sparse() fwd" in failed(LW.check_scaled("field", ".sparse() fwd", sc.f[T(ui).long()], ref, float(ref.abs().max())))


def test_room_scene_is_sampled_on_surfaces():
    """pc_restate.room_scene at ScanNet density: ~10^5 voxels of 2 cm, several live 3^3 offsets per voxel (a volume-filled
    scene of the same size has ~1), every raw label in 0..40."""
    from oracle import maps
    from pc_restate import room_scene

    xyz, rgb, lab = room_scene(np.random.default_rng(0), 300_000)
    assert xyz.shape == (300_000, 3) and rgb.shape == (300_000, 3) and lab.shape == (300_000,)
    assert rgb.min() >= 0 and rgb.max() <= 255 and lab.min() >= 0 and lab.max() <= 40
    q = np.floor(xyz / 0.02).astype(np.int32)
    c = np.concatenate([np.zeros((len(q), 1), np.int32), q], 1)
    ui, _ = maps.unique(c)
    live = (maps.kernel_map_table(c[ui], c[ui], maps.kernel_offsets(3, 1)) >= 0).sum(1).mean()
    print(f"room_scene: {len(ui)} voxels of 2 cm, {live:.2f} live offsets per voxel at tensor stride 1")
    assert 50_000 < len(ui) < 300_000 and live > 4.0
