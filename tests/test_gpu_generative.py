"""-m gpu: the generative layers (csrc/generate.hip, minkowski/generative.py) against tests/gen_restate.py and the CPU oracle:
children, the generative convolution forward and backward, pruning, convolutions and pooling downstream of both, occupancy,
and CompletionNet as a whole."""
import numpy as np
import pytest
import torch

import gen_restate as R
from helpers import batch_scenes

pytestmark = pytest.mark.gpu

POINTWISE_ROWS = 4096  # the row threshold of the pointwise path (minkowski/modules.py: use_mm)


def _ME():
    from nerf_downstream_amd import minkowski as ME

    return ME


def _derived(coords, feats, ts, B):
    """A HIP SparseTensor whose map is the int32 rows `coords` at tensor stride ts."""
    ME = _ME()
    m = ME.CoordinateManager.from_coordinates(torch.from_numpy(np.ascontiguousarray(coords, np.int32)).cuda(), ts, B)
    return ME.SparseTensor(feats, ME.CoordinateMapKey(ts), m)


# ------------------------------------------------------------------------------------------------------------------- children
@pytest.mark.parametrize("B", [2, 3])
@pytest.mark.parametrize("ts", [2, 4, 16])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_children(n, ts, B):
    ME = _ME()
    parents = R.random_parents(np.random.default_rng(100 * n + ts + B), n, ts, B, top=True)
    assert parents[:, 1:].min() < 0 and parents[-1, 1] + ts // 2 <= 32767 < parents[-1, 1] + ts  # negative rows; the top of the key range
    x = _derived(parents, torch.ones(n, 1, device="cuda"), ts, B)
    assert x.coordinate_manager.batch_size() == B and torch.equal(x.C.cpu(), torch.from_numpy(parents))
    up = ME.MinkowskiGenerativeConvolutionTranspose(1, 1).cuda()
    y = up(x)
    want = R.children(parents, ts)
    m = y.coordinate_manager
    assert y.tensor_stride == [ts // 2] * 3 and m is not x.coordinate_manager
    assert torch.equal(y.C.cpu(), torch.from_numpy(want))
    assert m.size(y.coordinate_map_key) == 8 * n == len(y) and m.batch_size() == B
    assert m.batch_offsets(y.coordinate_map_key).cpu().tolist() == R.batch_offsets(want, B).tolist()


# ------------------------------------------------------------------------------------------------- the generative convolution
def _grad_close(h, r, what):
    scale = float(r.abs().max())
    assert torch.allclose(h.cpu().double(), r, atol=2e-5 * max(scale, 1.0), rtol=1e-4), (what, float((h.cpu().double() - r).abs().max()))


@pytest.mark.parametrize("n", [1, 65, 300, POINTWISE_ROWS - 1, POINTWISE_ROWS])
@pytest.mark.parametrize("cin,cout", [(1, 3), (5, 7), (32, 16)])
def test_generative_convolution(cin, cout, n):
    ME = _ME()
    torch.manual_seed(n + cin)
    parents = R.random_parents(np.random.default_rng(n + cout), n, 2, 2, lo=-8, hi=8)
    kids = R.children(parents, 2)
    gen = ME.MinkowskiGenerativeConvolutionTranspose(cin, cout, bias=True).cuda()
    xf = torch.randn(n, cin)
    g = torch.randn(8 * n, cout)
    # float64 restatement
    rx, rw, rb = xf.double().requires_grad_(True), gen.kernel.detach().cpu().double().requires_grad_(True), gen.bias.detach().cpu().double().requires_grad_(True)
    ref = R.gen_product(rx, rw, rb)
    ref.backward(g.double())
    # the generative layer
    hx = xf.cuda().requires_grad_(True)
    y = gen(_derived(parents, hx, 2, 2))
    assert torch.equal(y.C.cpu(), torch.from_numpy(kids))
    y.F.backward(g.cuda())
    assert torch.allclose(y.F.detach().cpu().double(), ref.detach(), atol=2e-5, rtol=1e-5)
    assert torch.allclose(hx.grad.cpu().double(), rx.grad, atol=2e-5, rtol=1e-4)
    _grad_close(gen.kernel.grad, rw.grad, "kernel")
    assert torch.allclose(gen.bias.grad.cpu().double(), rb.grad, atol=1e-4, rtol=1e-5)
    # the existing transposed convolution with the same weights, on a manager built from the field of all children
    up = ME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=2, stride=2, bias=True, dimension=3).cuda()
    up.load_state_dict(gen.state_dict())
    fine = ME.TensorField(coordinates=torch.from_numpy(kids).float().cuda(), features=torch.zeros(8 * n, 1, device="cuda")).sparse()
    m = fine.coordinate_manager
    coarse_key = m.stride(fine.coordinate_map_key, 2)
    assert torch.equal(fine.C.cpu(), torch.from_numpy(kids)) and torch.equal(m.get_coordinates(coarse_key).cpu(), torch.from_numpy(parents))
    tx = xf.cuda().requires_grad_(True)
    z = up(ME.SparseTensor(tx, coarse_key, m))
    z.F.backward(g.cuda())
    assert torch.allclose(y.F.detach(), z.F.detach(), atol=2e-5, rtol=1e-5)
    assert torch.allclose(hx.grad, tx.grad, atol=2e-5, rtol=1e-4)
    _grad_close(gen.kernel.grad, up.kernel.grad.cpu().double(), "kernel vs transposed convolution")
    assert torch.allclose(gen.bias.grad, up.bias.grad, atol=1e-4, rtol=1e-5)


@pytest.mark.parametrize("mode", ["bf16", "bf16x3"])
def test_generative_convolution_is_fp32_in_every_math_mode(mode):
    """Above the pointwise path's row threshold, with channel counts the bf16 weight-gradient kernel would take (multiples of 32):
    the fp32 bounds hold under set_conv_math(mode), and the mode is what it was afterwards."""
    ME = _ME()
    n, cin, cout = POINTWISE_ROWS, 32, 16
    torch.manual_seed(7)
    parents = R.random_parents(np.random.default_rng(7), n, 2, 2, lo=-8, hi=8)
    gen = ME.MinkowskiGenerativeConvolutionTranspose(cin, cout).cuda()
    xf, g = torch.randn(n, cin), torch.randn(8 * n, cout)
    rx, rw = xf.double().requires_grad_(True), gen.kernel.detach().cpu().double().requires_grad_(True)
    ref = R.gen_product(rx, rw)
    ref.backward(g.double())
    old = ME.set_conv_math(mode)
    try:
        hx = xf.cuda().requires_grad_(True)
        y = gen(_derived(parents, hx, 2, 2))
        y.F.backward(g.cuda())
        torch.cuda.synchronize()
        from nerf_downstream_amd.minkowski import functional as Fn

        assert Fn.conv_math() == mode
    finally:
        ME.set_conv_math(old)
    assert torch.allclose(y.F.detach().cpu().double(), ref.detach(), atol=2e-5, rtol=1e-5)
    assert torch.allclose(hx.grad.cpu().double(), rx.grad, atol=2e-5, rtol=1e-4)
    _grad_close(gen.kernel.grad, rw.grad, "kernel")


def test_generative_convolution_refuses_an_odd_tensor_stride():
    ME = _ME()
    x = ME.SparseTensor(torch.ones(2, 1, device="cuda"), coordinates=torch.tensor([[0, 1, 2, 3], [0, 2, 2, 3]], dtype=torch.int32).cuda())
    with pytest.raises(ValueError, match="even tensor stride"):
        ME.MinkowskiGenerativeConvolutionTranspose(1, 1).cuda()(x)


# -------------------------------------------------------------------------------------------------------------------- pruning
def _prune_block():
    from nerf_downstream_amd._lib import CONSTANTS

    return CONSTANTS["MINK_PRUNE_BLOCK"]


def _mask(kind, coords):
    n = coords.shape[0]
    m = np.zeros(n, bool)
    if kind == "all":
        m[:] = True
    elif kind == "first":
        m[0] = True
    elif kind == "last":
        m[-1] = True
    elif kind == "alternating":
        m[::2] = True
    else:  # the middle sample of three removed entirely
        m = coords[:, 0] != 1
    return m


@pytest.mark.parametrize("kind", ["all", "first", "last", "alternating", "middle"])
@pytest.mark.parametrize("n", [1, 64, 65, 255, 256, 257, 513])
def test_pruning(n, kind):
    ME = _ME()
    assert _prune_block() == 256  # 255 / 256 / 257 / 513 = the compaction's workgroup size - 1, at it, + 1, twice it + 1
    B, ts = 3, 2
    coords = R.random_parents(np.random.default_rng(n), n, ts, B)
    mask = _mask(kind, coords)
    gen = torch.Generator().manual_seed(n)
    for C in (1, 3, 4, 32):
        xf = torch.randn(n, C, generator=gen)
        xf[torch.from_numpy(~mask)] = float("nan")  # a NaN in a pruned row appears nowhere in the output
        want_f, want_c, want_off, _, _ = R.prune(xf, coords, mask, B)
        hx = xf.cuda().requires_grad_(True)
        y = ME.MinkowskiPruning()(_derived(coords, hx, ts, B), torch.from_numpy(mask).cuda())
        m = y.coordinate_manager
        assert y.tensor_stride == [ts] * 3 and len(y) == int(mask.sum()) == m.size(y.coordinate_map_key)
        assert torch.equal(y.F.detach().cpu(), want_f) and bool(torch.isfinite(y.F).all())  # bit-exact: a copy
        assert torch.equal(y.C.cpu(), torch.from_numpy(want_c))
        assert m.batch_size() == B and m.batch_offsets(y.coordinate_map_key).cpu().tolist() == want_off.tolist()
        g = torch.randn(len(y), C, generator=gen)
        y.F.backward(g.cuda())
        # kept rows: their gradient row, untouched by the NaN of the pruned rows; pruned rows: zeros (not NaN)
        assert torch.equal(hx.grad.cpu(), R.prune_grad(g, mask))


def test_pruning_refusals():
    ME = _ME()
    coords = R.random_parents(np.random.default_rng(0), 10, 2, 2)
    x = _derived(coords, torch.randn(10, 4, device="cuda"), 2, 2)
    prune = ME.MinkowskiPruning()
    with pytest.raises(ValueError, match="keeps no row"):
        prune(x, torch.zeros(10, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="bool"):
        prune(x, torch.ones(10, device="cuda"))
    with pytest.raises(ValueError, match="one entry per row"):
        prune(x, torch.ones(9, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="is on cpu"):
        prune(x, torch.ones(10, dtype=torch.bool))
    # results live on a manager of their own: adding them to a tensor of the manager they came from is refused
    y = prune(x, torch.ones(10, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="share the coordinate manager"):
        y + x


# ---------------------------------------------------------------------------------------------- downstream of both operators
def _downstream(oracle_maps, t, emptied=None):
    """3x3x3 convolutions at strides 1 and 2 and a global average pool on the HIP tensor `t` at tensor stride 2, against the
    oracle on a fresh tensor made from the coordinates divided by 2 (a convolution at stride s on multiples of s is the
    stride-1 convolution on the divided coordinates)."""
    ME = _ME()
    from oracle import me_cpu as OME

    C = t.F.shape[1]
    torch.manual_seed(C)
    coords = t.C.cpu()
    small = coords.clone()
    small[:, 1:] //= 2
    assert torch.equal(small[:, 1:] * 2, coords[:, 1:])
    rt = OME.TensorField(coordinates=small.float(), features=t.F.detach().cpu()).sparse()
    assert torch.equal(rt.C, small)
    for stride in (1, 2):
        rconv = OME.MinkowskiConvolution(C, 12, kernel_size=3, stride=stride, dimension=3)
        hconv = ME.MinkowskiConvolution(C, 12, kernel_size=3, stride=stride, dimension=3).cuda()
        hconv.load_state_dict(rconv.state_dict())
        hy, ry = hconv(t), rconv(rt)
        assert hy.tensor_stride == [2 * stride] * 3
        hc = hy.C.cpu()
        assert torch.equal(hc[:, 0], ry.C[:, 0]) and torch.equal(hc[:, 1:], ry.C[:, 1:] * 2)
        assert torch.allclose(hy.F.detach().cpu(), ry.F.detach(), atol=2e-5, rtol=1e-5)
    hp = ME.MinkowskiGlobalAvgPooling()(t).F.detach().cpu()
    B = t.coordinate_manager.batch_size()
    assert hp.shape == (B, C)
    f, b = t.F.detach().cpu().double(), coords[:, 0].long()
    for s in range(B):
        rows = f[b == s]
        if s == emptied:
            assert rows.shape[0] == 0 and bool((hp[s] == 0).all())  # the pooled row of the emptied sample is zero
        else:
            assert torch.allclose(hp[s].double(), rows.mean(0), atol=2e-5, rtol=1e-5)
    rp = OME.MinkowskiGlobalAvgPooling()(rt).F
    keep = [s for s in range(rp.shape[0]) if s != emptied]
    assert torch.allclose(hp[keep], rp[keep].float(), atol=2e-5, rtol=1e-5)


def test_downstream_of_generation(oracle_maps):
    ME = _ME()
    parents = R.random_parents(np.random.default_rng(7), 90, 4, 3)
    gen = ME.MinkowskiGenerativeConvolutionTranspose(6, 8).cuda()
    _downstream(oracle_maps, gen(_derived(parents, torch.randn(90, 6, device="cuda"), 4, 3)))


def test_downstream_of_pruning(oracle_maps):
    ME = _ME()
    coords = R.random_parents(np.random.default_rng(8), 700, 2, 3, lo=-5, hi=5)
    mask = (coords[:, 0] != 1) & (np.random.default_rng(9).random(700) < 0.7)  # the middle sample loses every voxel
    y = ME.MinkowskiPruning()(_derived(coords, torch.randn(700, 8, device="cuda"), 2, 3), torch.from_numpy(mask).cuda())
    _downstream(oracle_maps, y, emptied=1)


# ------------------------------------------------------------------------------------------------------------------ occupancy
@pytest.mark.parametrize("ts", [1, 2, 4])
def test_occupancy(ts):
    ME = _ME()
    rng = np.random.default_rng(ts)
    tcoords = R.random_parents(rng, 400, 1, 2, lo=-8, hi=8)
    target = ME.SparseTensor(torch.ones(400, 1, device="cuda"), coordinates=torch.from_numpy(tcoords).cuda())
    tm = target.coordinate_manager
    floored = tcoords.astype(np.int64)
    floored[:, 1:] = floored[:, 1:] // ts * ts
    inside = np.unique(floored, axis=0)[::2]
    outside = R.random_parents(rng, 150, ts, 2, lo=-12, hi=12).astype(np.int64)
    q = np.unique(np.concatenate([inside, outside]), axis=0)  # (sorted: the batch column is non-decreasing)
    out = _derived(q, torch.zeros(q.shape[0], 1, device="cuda"), ts, 2)
    want = R.occupancy(q, tcoords, ts)
    assert 0 < want.sum() < want.shape[0]
    assert out.coordinate_manager is not tm and (ts == 1 or not tm.has_level(ts))  # another manager; the level is built on demand
    got = ME.generative.occupancy(out, target)
    assert got.dtype == torch.bool and got.cpu().numpy().tolist() == want.tolist()
    assert tm.has_level(ts)
    assert ME.generative.occupancy(out, target).cpu().numpy().tolist() == want.tolist()  # ... and found the second time
    if ts > 1:  # a tensor of the target's own manager at that stride: every voxel is one of the target's
        own = ME.SparseTensor(torch.zeros(tm.size(ME.CoordinateMapKey(ts)), 1, device="cuda"), ME.CoordinateMapKey(ts), tm)
        assert bool(ME.generative.occupancy(own, target).all())


# ---------------------------------------------------------------------------------------------------------------- whole model
CIN = 4
CLS_BIAS = -8.0  # far below every logit: in training the prediction ORed into the keep mask is empty, the masks are the target's


def _model_case():
    """Everything of the whole-model test that needs no GPU: weights, the partial input, the full target, the float64 pass."""
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from oracle import me_cpu as OME

    torch.manual_seed(0)
    model = get_model("CompletionNet", CIN, 1)
    with torch.no_grad():
        model.dec1.cls.bias.fill_(CLS_BIAS), model.dec2.cls.bias.fill_(CLS_BIAS)
    coords, feats = batch_scenes([41, 42], grid=16, cin=CIN)
    coords = coords.int()
    seen = torch.rand(coords.shape[0], generator=torch.Generator().manual_seed(2)) < 0.5  # the input: half of the target's voxels
    ref = R.RefCompletion(OME, CIN).double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()})
    for net in (model, ref):  # momentum 1: after the one training pass the running statistics ARE that batch's, so the eval pass
        for mod in net.modules():  # below sees normalised activations instead of an untrained net's near-zero logits
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.momentum = 1.0
    ref.train()
    rx = OME.TensorField(coordinates=coords[seen].double(), features=feats[seen].double()).sparse()
    levels, _ = ref(rx, coords.numpy())
    return model, ref, rx, coords, feats, seen, levels


def test_completion_net(oracle_maps):
    import torch.nn.functional as F

    ME = _ME()
    model, ref, rx, coords, feats, seen, rlevels = _model_case()
    # on the CPU, before any GPU work: at each level the target keeps at least one and fewer than all generated voxels, and
    # no classifier output comes near zero (so the ORed prediction cannot differ between fp32 and float64)
    assert len(rlevels) == 2
    for logits, occ, c, pred in rlevels:
        assert 1 <= int(occ.sum()) < occ.shape[0] == c.shape[0]
        assert not pred.any() and float(logits.detach().max()) < -1.0
    rloss = sum(F.binary_cross_entropy_with_logits(lg[:, 0], torch.from_numpy(occ).double()) for lg, occ, _, _ in rlevels) / 2
    rloss.backward()
    # ... and the eval-mode pass without a target keeps a good many voxels at each level, and not all
    with torch.no_grad():
        ref.dec1.cls.bias.zero_(), ref.dec2.cls.bias.zero_()
        ref.eval()
        for _, _, c, pred in ref(rx)[0]:
            assert 100 <= int(pred.sum()) < c.shape[0] - 100

    hip = model.cuda().train()
    x = ME.SparseTensor(feats[seen].cuda(), coordinates=coords[seen].cuda())
    target = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device="cuda"), coordinates=coords.cuda())
    levels, out = hip(x, target)
    assert out.tensor_stride == [1, 1, 1] and len(levels) == 2
    for (hl, hocc), (rl, rocc, rc, _) in zip(levels, rlevels):
        assert torch.equal(hl.C.cpu(), torch.from_numpy(rc)) and hocc.cpu().numpy().tolist() == rocc.tolist()
        assert torch.allclose(hl.F.detach().cpu().double(), rl.detach(), atol=1e-3, rtol=0), float((hl.F.detach().cpu().double() - rl.detach()).abs().max())
    assert len(out) == int(rlevels[1][1].sum())
    loss = hip.loss(levels)
    assert abs(loss.item() - rloss.item()) < 1e-3
    loss.backward()
    hp, rp = dict(hip.named_parameters()), dict(ref.named_parameters())
    assert hp.keys() == rp.keys()
    rel = {k: float((hp[k].grad.cpu().double() - rp[k].grad).norm() / rp[k].grad.norm().clamp_min(1e-12)) for k in hp}
    assert max(rel.values()) < 0.15, max(rel.items(), key=lambda kv: kv[1])
    errs = sorted(rel.values())
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
    flat_g = torch.cat([hp[k].grad.cpu().double().flatten() for k in hp])
    flat_o = torch.cat([rp[k].grad.flatten() for k in hp])
    assert float(torch.dot(flat_g, flat_o) / (flat_g.norm() * flat_o.norm())) > 0.999

    # one eval-mode pass without a target: keep = logits > 0
    with torch.no_grad():
        hip.dec1.cls.bias.zero_(), hip.dec2.cls.bias.zero_()
        hip.eval()
        levels, out = hip(x)
    assert [occ for _, occ in levels] == [None, None] and out.tensor_stride == [1, 1, 1]
    generated = set(map(tuple, levels[1][0].C.cpu().tolist()))
    final = list(map(tuple, out.C.cpu().tolist()))
    assert 0 < len(final) <= len(generated) and set(final) <= generated
    assert len(final) == int((levels[1][0].F[:, 0] > 0).sum())
