"""The float64 restatement of instance norm and layer norm (tests/norm_restate.py) against torch's own float64 forward and
autograd; the layer factory's norm types; the state-dict layout of the two modules.  No GPU, no shared library."""
import pytest
import torch
import torch.nn.functional as F

import norm_restate as NR

SIZES = [0, 700, 1, 0, 413, 64, 65]  # empty samples first and in the middle, a one-row sample, sizes on / off a 64-row boundary
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (relu, residual)


def _offsets(sizes):
    off = [0]
    for k in sizes:
        off.append(off[-1] + k)
    return off


def _inputs(n, C, seed, residual):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g, dtype=torch.float64) * 1.5 + 0.2
    dy = torch.randn(n, C, generator=g, dtype=torch.float64)
    gamma = torch.linspace(0.5, 1.5, C, dtype=torch.float64)
    beta = torch.linspace(-0.2, 0.2, C, dtype=torch.float64)
    res = torch.randn(n, C, generator=g, dtype=torch.float64) if residual else None
    return x, dy, gamma, beta, res


def _torch_grads(y, dy, leaves):
    return torch.autograd.grad(y, leaves, dy, allow_unused=True)


@pytest.mark.parametrize("relu,residual", VARIANTS)
@pytest.mark.parametrize("sizes,C", [(SIZES, 24), (SIZES, 3), ([257], 5)])
def test_instance_norm_restatement_matches_torch_float64(sizes, C, relu, residual):
    off = _offsets(sizes)
    n, eps = off[-1], 1e-8
    x, dy, gamma, beta, res = _inputs(n, C, 3, residual)
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)] + ([res.clone().requires_grad_(True)] if residual else [])
    xr, gr, br = leaves[:3]
    parts = []
    for s, e in zip(off[:-1], off[1:]):
        if e - s > 1:  # F.instance_norm over (1, C, rows): biased variance, per channel
            parts.append(F.instance_norm(xr[s:e].t()[None], eps=eps)[0].t() * gr + br)
        elif e > s:  # (torch refuses a single spatial element: the explicit formula)
            seg = xr[s:e]
            mu, var = seg.mean(0, keepdim=True), seg.var(0, unbiased=False, keepdim=True)
            parts.append((seg - mu) / torch.sqrt(var + eps) * gr + br)
    z = torch.cat(parts)
    if residual:
        z = z + leaves[3]
    y = torch.relu(z) if relu else z
    grads = _torch_grads(y, dy, leaves)
    got = NR.instance_norm_fwd(x, off, gamma, beta, eps, res, relu)
    assert torch.allclose(got, y.detach(), atol=1e-9, rtol=1e-9)  # (1 / sqrt(0 + 1e-8) amplifies the one-row sample's rounding)
    dx, dga, dbe, dres = NR.instance_norm_bwd(dy, x, off, gamma, beta, eps, res, relu)
    assert torch.allclose(dx, grads[0], atol=1e-8, rtol=1e-9)
    assert torch.allclose(dga, grads[1], atol=1e-9, rtol=1e-10) and torch.allclose(dbe, grads[2], atol=1e-10, rtol=1e-10)
    if residual:
        assert torch.allclose(dres, grads[3], atol=0, rtol=0)


@pytest.mark.parametrize("relu,residual", VARIANTS)
@pytest.mark.parametrize("n,C", [(1, 1), (63, 3), (65, 32), (100, 96), (7, 512)])
def test_layer_norm_restatement_matches_torch_float64(n, C, relu, residual):
    eps = 1e-5
    x, dy, gamma, beta, res = _inputs(n, C, 4, residual)
    leaves = [t.clone().requires_grad_(True) for t in (x, gamma, beta)] + ([res.clone().requires_grad_(True)] if residual else [])
    z = F.layer_norm(leaves[0], (C,), leaves[1], leaves[2], eps)
    if residual:
        z = z + leaves[3]
    y = torch.relu(z) if relu else z
    grads = _torch_grads(y, dy, leaves)
    assert torch.allclose(NR.layer_norm_fwd(x, gamma, beta, eps, res, relu), y.detach(), atol=1e-12, rtol=1e-12)
    dx, dga, dbe, dres = NR.layer_norm_bwd(dy, x, gamma, beta, eps, res, relu)
    assert torch.allclose(dx, grads[0], atol=1e-11, rtol=1e-10)
    assert torch.allclose(dga, grads[1], atol=1e-11, rtol=1e-10) and torch.allclose(dbe, grads[2], atol=1e-12, rtol=1e-12)
    if residual:
        assert torch.allclose(dres, grads[3], atol=0, rtol=0)


def test_empty_and_one_row_samples():
    C, eps = 4, 1e-8
    x = torch.tensor([[1.0, -2.0, 3.0, 50.0]], dtype=torch.float64)
    gamma, beta = torch.full((C,), 2.0, dtype=torch.float64), torch.arange(C, dtype=torch.float64)
    off = [0, 0, 1, 1]  # empty, one row, empty
    mean, invstd, xhat = NR.instance_stats(x, off, eps)
    assert torch.equal(mean[1], x[0]) and torch.equal(mean[0], torch.zeros(C, dtype=torch.float64)) and bool((invstd[2] == 0).all())
    assert torch.equal(xhat, torch.zeros_like(x))  # variance 0: xhat = 0, y = beta
    assert torch.equal(NR.instance_norm_fwd(x, off, gamma, beta, eps), beta[None])
    dx, dga, dbe, dres = NR.instance_norm_bwd(torch.ones_like(x), x, off, gamma, beta, eps)
    assert torch.equal(dx, torch.zeros_like(x)) and torch.equal(dga, torch.zeros(C, dtype=torch.float64))
    assert torch.equal(dbe, torch.ones(C, dtype=torch.float64)) and torch.equal(dres, torch.ones_like(x))
    # nothing at all
    e = torch.zeros(0, C, dtype=torch.float64)
    assert NR.instance_norm_fwd(e, [0, 0], gamma, beta, eps).shape == (0, C)
    dx, dga, dbe, _ = NR.instance_norm_bwd(e, e, [0, 0], gamma, beta, eps)
    assert dx.shape == (0, C) and not dga.any() and not dbe.any()
    assert NR.sample_of_rows([0, 0, 3, 3, 5], 5).tolist() == [1, 1, 1, 3, 3]
    with pytest.raises(AssertionError):
        NR.sample_of_rows([0, 3], 5)


def test_get_norm_types():
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models.mink.modules.common import get_norm

    assert type(get_norm("BN", 8)) is ME.MinkowskiBatchNorm
    assert type(get_norm("IN", 8)) is ME.MinkowskiInstanceNorm
    assert type(get_norm("LN", 8)) is ME.MinkowskiLayerNorm
    with pytest.raises(ValueError, match="PN.*not implemented"):
        get_norm("PN", 8)
    with pytest.raises(ValueError, match="GN not supported"):
        get_norm("GN", 8)


def test_state_dict_layout_and_sync_conversion():
    from nerf_downstream_amd import minkowski as ME

    ln = ME.MinkowskiLayerNorm(12)
    assert list(ln.state_dict()) == ["ln.weight", "ln.bias"] and ln.ln.eps == 1e-5 and ln.ln.weight.shape == (12,)
    assert list(ME.MinkowskiLayerNorm(12, affine=False).state_dict()) == []
    inorm = ME.MinkowskiInstanceNorm(12)
    assert {k: tuple(v.shape) for k, v in inorm.state_dict().items()} == {"weight": (1, 12), "bias": (1, 12)} and inorm.eps == 1e-8
    assert not list(ln.buffers()) and not list(inorm.buffers())  # no running statistics
    seq = torch.nn.Sequential(ln, inorm, ME.MinkowskiBatchNorm(12))
    out = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(seq)
    assert out[0] is ln and out[1] is inorm and type(out[2]) is ME.MinkowskiSyncBatchNorm


@pytest.mark.parametrize("norm_type", ["IN", "LN"])
def test_models_build_with_per_sample_norms(norm_type):
    """Construction only (no device): every norm layer of Res16UNet follows NORM_TYPE; a ResNet's follows it at the stem, its
    blocks and shortcuts keep batch norm as the reference's _make_layer does; the native trunk refuses the model."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models.mink.res16unet import Res16UNet14, Res16UNet50
    from nerf_downstream_amd.co3d_3d.src.models.mink.resnet import ResNet14, ResNet50
    from nerf_downstream_amd.minkowski import trunk

    kind = {"IN": ME.MinkowskiInstanceNorm, "LN": ME.MinkowskiLayerNorm}[norm_type]
    for cls in (Res16UNet14, Res16UNet50):
        net = cls(3, 20, NORM_TYPE=norm_type)
        norms = [m for m in net.modules() if isinstance(m, (ME.MinkowskiBatchNorm, ME.MinkowskiInstanceNorm, ME.MinkowskiLayerNorm))]
        assert norms and all(type(m) is kind for m in norms)
        assert not list(net.buffers())
        key = "conv0p1s1.1.ln.weight" if norm_type == "LN" else "conv0p1s1.1.weight"
        assert key in net.state_dict()
    for base in (ResNet14, ResNet50):
        net = type(base.__name__ + norm_type, (base,), {"NORM_TYPE": norm_type})(28, 10)
        assert type(net.bn1) is kind and type(net.layer1[0].norm1) is ME.MinkowskiBatchNorm
        assert type(net.layer1[0].downsample[1]) is ME.MinkowskiBatchNorm
        assert net.bn1 not in net._norms and trunk.plan_for(net) is None
