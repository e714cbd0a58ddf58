"""-m gpu: the segmented instance norm and the row-wise layer norm (csrc/norm.hip) against the float64 restatement of
tests/norm_restate.py -- at the functional level with explicit offsets and through the modules; centred inputs at the
tolerances of the existing instance-norm test, non-centred inputs (mean 50, sd 1, one channel constant within a sample) at
the bound fp32 inputs allow; bitwise reproducibility; no host synchronisation; and whole networks built with NORM_TYPE
"IN" / "LN" against the same network in float64 on the CPU oracle."""
import pytest
import torch
import torch.nn.functional as F

import norm_restate as NR
from helpers import batch_scenes, misaligned, trunk_node

pytestmark = pytest.mark.gpu

SIZES = [0, 700, 1, 0, 413, 64, 65]  # empty samples first and in the middle, one row (variance 0), on / off a 64-row boundary
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (relu, residual)
FWD_TOL = dict(atol=2e-5, rtol=1e-5)   # tests/test_gpu_compat.py test_prelu_and_instance_norm_match_torch
GRAD_TOL = dict(atol=2e-4, rtol=1e-4)
BOUND_FACTOR = 2.0  # the non-centred cases: measured error <= BOUND_FACTOR x the bound norm_restate derives from the fp32 inputs


def _offsets(sizes):
    off = [0]
    for k in sizes:
        off.append(off[-1] + k)
    return off


def _inputs(n, C, seed, centre=0.2, spread=1.5):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * spread + centre
    dy = torch.randn(n, C, generator=g)
    res = torch.randn(n, C, generator=g)
    gamma, beta = torch.linspace(0.5, 1.5, C), torch.linspace(-0.2, 0.2, C)
    return x, dy, res, gamma, beta


def _sparse(x, sizes):
    from nerf_downstream_amd import minkowski as ME

    coords = torch.zeros(x.shape[0], 4)
    coords[:, 0] = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes)).float()
    coords[:, 1] = torch.arange(x.shape[0])
    field = ME.TensorField(coordinates=coords.cuda(), features=x.detach())
    return ME.SparseTensor(x, ME.CoordinateMapKey(1), field.coordinate_manager)


def _run_in(x, dy, res, gamma, beta, off, eps, relu, residual):
    """One forward + backward of InstanceNormFunction with explicit offsets -> (y, dx, dgamma, dbeta, dres) on the host."""
    from nerf_downstream_amd.minkowski import functional as Fn

    leaves = [t.clone().cuda().requires_grad_(True) for t in (x, gamma, beta)]
    r = res.clone().cuda().requires_grad_(True) if residual else None
    offd = torch.tensor(off, dtype=torch.int32, device="cuda")
    y = Fn.InstanceNormFunction.apply(leaves[0], leaves[1], leaves[2], offd, eps, r, relu)
    y.backward(dy.cuda())
    return [y.detach().cpu()] + [t.grad.cpu() for t in leaves] + [r.grad.cpu() if residual else None]


def _run_ln(x, dy, res, gamma, beta, eps, relu, residual):
    from nerf_downstream_amd.minkowski import functional as Fn

    leaves = [t.clone().cuda().requires_grad_(True) for t in (x, gamma, beta)]
    r = res.clone().cuda().requires_grad_(True) if residual else None
    y = Fn.LayerNormFunction.apply(leaves[0], leaves[1], leaves[2], eps, r, relu)
    y.backward(dy.cuda())
    return [y.detach().cpu()] + [t.grad.cpu() for t in leaves] + [r.grad.cpu() if residual else None]


def _close(got, ref, tol, what):
    assert got.shape == ref.shape, what
    assert torch.allclose(got.double(), ref, **tol), (what, float((got.double() - ref).abs().max()))


def _check_centred(got, ref_fwd, ref_bwd, z_ref, relu, residual, what):
    """`got` = (y, dx, dgamma, dbeta, dres); the restatement's backward runs under the kernel's own ReLU decisions, which may
    differ from float64's only where the pre-activation is zero to rounding."""
    y, dx, dga, dbe, dres = got
    _close(y, ref_fwd, FWD_TOL, what + " y")
    mask = (y > 0) if relu else None
    if relu:
        flips = mask != (z_ref > 0)
        assert not flips.any() or float(z_ref[flips].abs().max()) <= 2e-5, what + " relu decisions"
    rdx, rdga, rdbe, rdres = ref_bwd(mask)
    _close(dx, rdx, GRAD_TOL, what + " dx")
    _close(dga, rdga, GRAD_TOL, what + " dgamma")
    _close(dbe, rdbe, GRAD_TOL, what + " dbeta")
    if residual:
        assert torch.equal(dres.double(), rdres), what + " dresidual"


# ------------------------------------------------------------------------------------------------ instance norm
@pytest.mark.parametrize("sizes", [SIZES, [513]], ids=["B7", "B1"])
@pytest.mark.parametrize("C", [3, 24, 32, 70, 96, 256])  # (70: dword lanes, more column groups than one row lane holds)
def test_instance_norm_function_matches_float64(sizes, C):
    off, eps = _offsets(sizes), 1e-8
    x, dy, res, gamma, beta = _inputs(off[-1], C, 7)
    for relu, residual in VARIANTS:
        got = _run_in(x, dy, res, gamma, beta, off, eps, relu, residual)
        r = res if residual else None
        z = NR.instance_norm_fwd(x, off, gamma, beta, eps, r, False)
        _check_centred(got, z.clamp_min(0) if relu else z,
                       lambda mask: NR.instance_norm_bwd(dy, x, off, gamma, beta, eps, r, relu, mask), z, relu, residual,
                       f"IN C={C} relu={relu} res={residual}")


@pytest.mark.parametrize("C", [3, 24])
def test_instance_norm_module_matches_float64_without_host_sync(C):
    from nerf_downstream_amd import minkowski as ME

    off = _offsets(SIZES)
    x, dy, res, gamma, beta = _inputs(off[-1], C, 8)
    mod = ME.MinkowskiInstanceNorm(C).cuda()
    with torch.no_grad():
        mod.weight.copy_(gamma[None]), mod.bias.copy_(beta[None])
    assert not list(mod.buffers()) and mod.eps == 1e-8
    xs = x.clone().cuda().requires_grad_(True)
    st = _sparse(xs, SIZES)
    rs = ME.SparseTensor(res.clone().cuda().requires_grad_(True), st.coordinate_map_key, st.coordinate_manager)
    mod(st)  # the first call builds the batch offsets (one read-back of the sortedness flag)
    mod.eval()  # no running statistics: eval mode is training mode
    dyd = dy.cuda()  # (a copy from pageable host memory synchronises: made before the guarded region)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = mod(st, relu=True, residual=rs)
        out.F.backward(dyd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert out.coordinate_map_key == st.coordinate_map_key
    for relu, residual in VARIANTS[:3]:  # the other three variants through the module (fresh leaves, parameter gradients reset)
        xp, rp = x.clone().cuda().requires_grad_(True), res.clone().cuda().requires_grad_(True)
        saved = (mod.weight.grad.clone(), mod.bias.grad.clone())
        mod.weight.grad, mod.bias.grad = None, None
        kw = dict(relu=relu, residual=ME.SparseTensor(rp, st.coordinate_map_key, st.coordinate_manager) if residual else None)
        o = mod(ME.SparseTensor(xp, st.coordinate_map_key, st.coordinate_manager), **kw)
        o.F.backward(dyd)
        r = res if residual else None
        zp = NR.instance_norm_fwd(x, off, gamma, beta, mod.eps, r, False)
        gotp = [o.F.detach().cpu(), xp.grad.cpu(), mod.weight.grad.cpu().reshape(-1), mod.bias.grad.cpu().reshape(-1),
                rp.grad.cpu() if residual else None]
        _check_centred(gotp, zp.clamp_min(0) if relu else zp,
                       lambda mask, r=r, relu=relu: NR.instance_norm_bwd(dy, x, off, gamma, beta, mod.eps, r, relu, mask), zp, relu,
                       residual, f"IN module C={C} relu={relu} res={residual}")
        mod.weight.grad, mod.bias.grad = saved
    z = NR.instance_norm_fwd(x, off, gamma, beta, mod.eps, res, False)
    got = [out.F.detach().cpu(), xs.grad.cpu(), mod.weight.grad.cpu().reshape(-1), mod.bias.grad.cpu().reshape(-1), rs.F.grad.cpu()]
    assert mod.weight.grad.shape == (1, C)
    _check_centred(got, z.clamp_min(0), lambda mask: NR.instance_norm_bwd(dy, x, off, gamma, beta, mod.eps, res, True, mask), z,
                   True, True, f"IN module C={C}")


def _report(name, errs, bounds):
    ratios = {k: float((errs[k] / bounds[k].clamp_min(1e-300)).max()) for k in errs}
    print(f"[norm parity] {name}: measured / bound " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    return ratios


@pytest.mark.parametrize("C", [3, 24])
def test_instance_norm_non_centred_within_what_fp32_inputs_allow(C):
    """mean 50, sd 1 per channel, channel 1 constant within sample 1; eps = 1e-8.  The bounds are norm_restate's."""
    off, eps = _offsets(SIZES), 1e-8
    x, dy, res, gamma, beta = _inputs(off[-1], C, 9, centre=50.0, spread=1.0)
    x[off[1]:off[2], 1] = 50.25
    rows = NR.sample_of_rows(off, off[-1])
    y, dx, dga, dbe, _ = _run_in(x, dy, res, gamma, beta, off, eps, False, False)
    _, invstd, xhat = NR.instance_stats(x, off, eps)
    is_rows = invstd[rows]
    y_ref = NR.instance_norm_fwd(x, off, gamma, beta, eps)
    rdx, rdga, rdbe, _ = NR.instance_norm_bwd(dy, x, off, gamma, beta, eps)
    assert torch.equal(y[off[1]:off[2], 1].double(), beta.double()[1].expand(SIZES[1]))  # the constant channel: y == beta exactly
    bx, bga, bbe = NR.grad_bounds(dy, x, xhat, is_rows, gamma, rows, rdx)
    errs = {"y": (y.double() - y_ref).abs(), "dx": (dx.double() - rdx).abs(), "dgamma": (dga.double() - rdga).abs(),
            "dbeta": (dbe.double() - rdbe).abs()}
    ratios = _report(f"instance norm C={C} n={off[-1]}", errs, {"y": NR.forward_bound(x, is_rows, gamma, y_ref), "dx": bx, "dgamma": bga, "dbeta": bbe})
    assert max(ratios.values()) <= BOUND_FACTOR, ratios


# ------------------------------------------------------------------------------------------------ layer norm
@pytest.mark.parametrize("C", [1, 3, 32, 70, 96, 256, 510, 512])  # (70, 510: dword lanes holding 2 and 8 columns each)
def test_layer_norm_function_matches_float64(C):
    eps = 1e-5
    for n in (1, 63, 64, 65, 1000):
        x, dy, res, gamma, beta = _inputs(n, C, 10 + n)
        for relu, residual in VARIANTS:
            got = _run_ln(x, dy, res, gamma, beta, eps, relu, residual)
            r = res if residual else None
            z = NR.layer_norm_fwd(x, gamma, beta, eps, r, False)
            _check_centred(got, z.clamp_min(0) if relu else z, lambda mask: NR.layer_norm_bwd(dy, x, gamma, beta, eps, r, relu, mask),
                           z, relu, residual, f"LN n={n} C={C} relu={relu} res={residual}")


def test_layer_norm_module_on_sparse_tensor_and_field():
    from nerf_downstream_amd import minkowski as ME

    C, sizes = 20, [300, 211]
    x, dy, res, gamma, beta = _inputs(sum(sizes), C, 11)
    mod = ME.MinkowskiLayerNorm(C).cuda()
    assert list(mod.state_dict()) == ["ln.weight", "ln.bias"] and not list(mod.buffers())
    with torch.no_grad():
        mod.ln.weight.copy_(gamma), mod.ln.bias.copy_(beta)
    st = _sparse(x.clone().cuda(), sizes)
    out = mod(st, relu=True)
    assert type(out) is ME.SparseTensor and out.coordinate_map_key == st.coordinate_map_key
    ref = NR.layer_norm_fwd(x, gamma, beta, 1e-5, None, True)
    _close(out.F.cpu(), ref, FWD_TOL, "LN module")
    _close(mod.eval()(st, relu=True).F.cpu(), ref, FWD_TOL, "LN module, eval mode")
    coords = torch.zeros(sum(sizes), 4)
    coords[:, 0] = torch.repeat_interleave(torch.arange(2), torch.tensor(sizes)).float()
    coords[:, 1] = torch.arange(sum(sizes))
    field = ME.TensorField(coordinates=coords.cuda(), features=x.clone().cuda())
    fout = mod(field)
    assert type(fout) is ME.TensorField and fout.coordinate_manager is field.coordinate_manager
    _close(fout.F.cpu(), NR.layer_norm_fwd(x, gamma, beta, 1e-5), FWD_TOL, "LN module on a field")
    with pytest.raises(ValueError, match="at most 512"):  # refused where the mistake is made, not at the first forward
        ME.MinkowskiLayerNorm(516)


@pytest.mark.parametrize("n,C", [(1000, 96), (65, 3), (200, 512)])
def test_layer_norm_non_centred_within_what_fp32_inputs_allow(n, C):
    eps = 1e-5
    x, dy, res, gamma, beta = _inputs(n, C, 12, centre=50.0, spread=1.0)
    y, dx, dga, dbe, _ = _run_ln(x, dy, res, gamma, beta, eps, False, False)
    _, invstd, xhat = NR.layer_stats(x, eps)
    y_ref = NR.layer_norm_fwd(x, gamma, beta, eps)
    rdx, rdga, rdbe, _ = NR.layer_norm_bwd(dy, x, gamma, beta, eps)
    bx, bga, bbe = NR.grad_bounds(dy, x, xhat, invstd, gamma, None, rdx)
    errs = {"y": (y.double() - y_ref).abs(), "dx": (dx.double() - rdx).abs(), "dgamma": (dga.double() - rdga).abs(),
            "dbeta": (dbe.double() - rdbe).abs()}
    ratios = _report(f"layer norm n={n} C={C}", errs, {"y": NR.forward_bound(x, invstd, gamma, y_ref), "dx": bx, "dgamma": bga, "dbeta": bbe})
    assert max(ratios.values()) <= BOUND_FACTOR, ratios


# ------------------------------------------------------------------------------------------------ alignment fallback
def test_misaligned_input_takes_the_dword_kernels():
    """C % 4 == 0 but x starts 4 bytes off a 16-byte boundary: instance norm and layer norm, forward and backward, must run
    their dword kernels.  The restatements and tolerances of the two *_function_matches_float64 tests above."""
    from nerf_downstream_amd.minkowski import functional as Fn

    off, C = _offsets(SIZES), 24
    n = off[-1]
    x, dy, res, gamma, beta = _inputs(n, C, 15)
    offd = torch.tensor(off, dtype=torch.int32, device="cuda")
    for relu, residual in VARIANTS:
        r = res if residual else None
        for kind in ("IN", "LN"):
            flat, xv = misaligned(x, requires_grad=True)
            ga, be = (t.clone().cuda().requires_grad_(True) for t in (gamma, beta))
            rd = res.clone().cuda().requires_grad_(True) if residual else None
            assert xv.data_ptr() % 16 == 4
            if kind == "IN":
                eps = 1e-8
                y = Fn.InstanceNormFunction.apply(xv, ga, be, offd, eps, rd, relu)
                z = NR.instance_norm_fwd(x, off, gamma, beta, eps, r, False)
                bwd = lambda mask: NR.instance_norm_bwd(dy, x, off, gamma, beta, eps, r, relu, mask)  # noqa: E731
            else:
                eps = 1e-5
                y = Fn.LayerNormFunction.apply(xv, ga, be, eps, rd, relu)
                z = NR.layer_norm_fwd(x, gamma, beta, eps, r, False)
                bwd = lambda mask: NR.layer_norm_bwd(dy, x, gamma, beta, eps, r, relu, mask)  # noqa: E731
            y.backward(dy.cuda())
            got = [y.detach().cpu(), flat.grad[1:1 + n * C].view(n, C).cpu(), ga.grad.cpu(), be.grad.cpu(), rd.grad.cpu() if residual else None]
            _check_centred(got, z.clamp_min(0) if relu else z, bwd, z, relu, residual, f"misaligned {kind} relu={relu} res={residual}")


# ------------------------------------------------------------------------------------------------ reproducibility
def test_two_runs_are_bitwise_equal():
    off = _offsets(SIZES)
    x, dy, res, gamma, beta = _inputs(off[-1], 96, 13)
    a, b = (_run_in(x, dy, res, gamma, beta, off, 1e-8, True, True) for _ in range(2))
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    x, dy, res, gamma, beta = _inputs(5000, 96, 14)
    off = [0, 1234, 5000]  # more rows than one chunk per sample: several partials per column
    a, b = (_run_in(x, dy, res, gamma, beta, off, 1e-8, True, True) for _ in range(2))
    assert all(torch.equal(p, q) for p, q in zip(a, b))
    a, b = (_run_ln(x, dy, res, gamma, beta, 1e-5, True, True) for _ in range(2))
    assert all(torch.equal(p, q) for p, q in zip(a, b))


# ------------------------------------------------------------------------------------------------ whole networks
class _OracleME:
    """oracle.me_cpu with the one layer it lacks: MinkowskiLayerNorm as torch's own LayerNorm on F."""

    def __init__(self):
        from oracle import me_cpu as OME

        self._ome = OME

        class MinkowskiLayerNorm(torch.nn.Module):
            def __init__(self, num_features, eps=1e-5, affine=True):
                super().__init__()
                self.ln = torch.nn.LayerNorm(num_features, eps=eps, elementwise_affine=affine)

            def forward(self, input):
                return OME.SparseTensor(self.ln(input.F), input.coordinate_map_key, input._manager)

        self.MinkowskiLayerNorm = MinkowskiLayerNorm

    def __getattr__(self, name):
        return getattr(self._ome, name)


def _net_pair(name, norm_type, cin, ncls):
    from nerf_downstream_amd.co3d_3d.src.models.mink import res16unet, resnet

    torch.manual_seed(0)
    if name.startswith("Res16UNet"):
        cls = getattr(res16unet, name)
        mk = lambda **kw: cls(cin, ncls, NORM_TYPE=norm_type, **kw)  # noqa: E731
    else:
        cls = type(name + norm_type, (getattr(resnet, name),), {"NORM_TYPE": norm_type})
        mk = lambda **kw: cls(cin, ncls, **kw)  # noqa: E731
    ref = mk(ME=_OracleME()).double()
    hip = mk().cuda()
    with torch.no_grad():  # affine parameters away from (1, 0), so that their gradients and a swapped pair would show
        for p_name, p in ref.named_parameters():
            if p_name.endswith(("weight", "bias")) and "final" not in p_name:
                p.add_(0.1 * torch.randn_like(p))
    hip.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    return hip, ref


@pytest.mark.parametrize("name,norm_type,in_eps", [("Res16UNet14", "IN", None), ("Res16UNet14", "IN", 1e-5), ("Res16UNet14", "LN", None),
                                                  ("ResNet14", "IN", None)])
def test_networks_with_per_sample_norms_match_float64(oracle_maps, name, norm_type, in_eps):
    """Two 32^3 shell scenes (~2 k voxels each, centred on the origin so that the coarsest level keeps several voxels per
    scene), one training step: logits and every parameter gradient against the same network in float64 on the oracle's maps.
    Tolerances: those of the batch-norm counterparts on such scenes, tests/test_gpu_unet.py test_res16unet_matches_oracle (logits
    1e-3; per-tensor relative gradient error < 0.15, median < 2e-2, cosine > 0.999 -- a ReLU that takes the other branch in
    fp32 is what the slack is for) and tests/test_gpu_resnet.py test_resnet_matches_oracle (logits 1e-3, cosine > 0.999,
    per-tensor relative error <= max(1e-3, 3 / sqrt(rows x channels of the tensor's stage))).

    `in_eps`: the eps of every MinkowskiInstanceNorm, on both sides.  At the layer's own 1e-8 a channel that ReLU has left
    (nearly) constant within a scene has invstd up to 1e4, and its dx = gamma invstd (g - mean g - ...) multiplies the fp32
    rounding of the incoming gradient by that: Res16UNet14 "IN" then sits at a median per-tensor error of 5e-3 on these scenes
    (2e-3 on 64^3 scenes) -- inside the batch-norm counterpart's tolerances, which is all that case asserts.  With eps = 1e-5
    both sides are well conditioned and the same network, kernels and scenes give 1.5e-6: that case asserts the fp32-kind
    bound of tests/test_gpu_resnet.py, 1e-3 per tensor, with no slack for anything else."""
    from nerf_downstream_amd import minkowski as ME

    seg = name.startswith("Res16UNet")
    cin, ncls = 28, (20 if seg else 51)
    hip, ref = _net_pair(name, norm_type, cin, ncls)
    kind = {"IN": ME.MinkowskiInstanceNorm, "LN": ME.MinkowskiLayerNorm}[norm_type]
    if in_eps is not None:
        for m in list(hip.modules()) + list(ref.modules()):
            if type(m).__name__ == "MinkowskiInstanceNorm":
                m.eps = in_eps
    mine = [m for m in hip.modules() if isinstance(m, kind)]
    assert mine and not any(list(m.buffers()) for m in mine)  # no running statistics on those layers
    if seg:
        assert not list(hip.buffers()) and not any(isinstance(m, ME.MinkowskiBatchNorm) for m in hip.modules())
    coords, feats = batch_scenes([51, 52], grid=32, cin=cin, negative=True)
    assert 1500 < coords.shape[0] / 2 < 4000
    rng = torch.Generator().manual_seed(2)
    labels = torch.randint(0, ncls, (coords.shape[0] if seg else 2,), generator=rng)
    hip.train(), ref.train()
    field = hip.process_input({"coordinates": coords.cuda(), "features": feats.cuda()})
    out = hip(field)
    assert trunk_node(out) is None and not getattr(hip, "_trunk_plan", None)  # the one-call native trunk is not taken
    out64 = ref(ref.process_input({"coordinates": coords, "features": feats.double()}))
    assert out.shape == out64.shape
    err = float((out.detach().cpu().double() - out64).abs().max())
    print(f"[{name} {norm_type} eps={in_eps}] logits: max |err| {err:.2e} against float64 (max |logit| {float(out64.abs().max()):.2f})")
    assert err <= 1e-3
    F.cross_entropy(out, labels.cuda()).backward()
    F.cross_entropy(out64, labels).backward()
    hp, rp = dict(hip.named_parameters()), dict(ref.named_parameters())
    assert hp.keys() == rp.keys() and all(p.grad is not None for p in hp.values())
    rel = {k: float((hp[k].grad.cpu().double() - rp[k].grad).norm() / rp[k].grad.norm().clamp_min(1e-12)) for k in hp}
    flat_g = torch.cat([hp[k].grad.cpu().double().flatten() for k in hp])
    flat_o = torch.cat([rp[k].grad.flatten() for k in hp])
    cos = float(torch.dot(flat_g, flat_o) / (flat_g.norm() * flat_o.norm()))
    worst = max(rel.items(), key=lambda kv: kv[1])
    errs = sorted(rel.values())
    print(f"[{name} {norm_type} eps={in_eps}] parameter gradients: worst {worst[0]} {worst[1]:.2e}, median {errs[len(errs) // 2]:.2e}, cosine {cos:.6f}")
    assert cos > 0.999, cos
    if in_eps is not None:
        assert worst[1] <= 1e-3, worst
    if seg:
        assert worst[1] < 0.15, worst
        assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
    else:
        rows_at = {ts: lev.n for ts, lev in field.coordinate_manager.levels.items()}
        for k, e in rel.items():
            rows = rows_at[2 ** (int(k[5]) + 1)] if k.startswith("layer") else (2 if k.startswith("final") else rows_at[1])
            assert e <= max(1e-3, 3.0 / (rows * rp[k].shape[-1]) ** 0.5), (k, e)
    # convert_sync_batchnorm leaves instance / layer norms as they were
    before = [id(m) for m in hip.modules() if isinstance(m, kind)]
    conv = ME.MinkowskiSyncBatchNorm.convert_sync_batchnorm(hip)
    assert [id(m) for m in conv.modules() if isinstance(m, kind)] == before
    if seg and norm_type == "IN":  # no running statistics anywhere: eval mode computes what training mode computes
        hip.eval()
        with torch.no_grad():
            assert torch.equal(hip(field), out.detach())


def test_bottleneck_block_runs_with_instance_and_layer_norm(oracle_maps):
    """Bottleneck(norm_type=...) forward + backward on the fused path against the same block in float64 on the oracle."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models.mink.modules.resnet_block import Bottleneck

    coords, feats = batch_scenes([61, 62], grid=24, cin=32)
    for norm_type in ("IN", "LN"):
        torch.manual_seed(1)
        ref = Bottleneck(32, 8, norm_type=norm_type, ME=_OracleME()).double()
        hip = Bottleneck(32, 8, norm_type=norm_type).cuda()
        hip.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
        OME = _OracleME()
        rx = OME.TensorField(coordinates=coords, features=feats.double()).sparse()
        hx = ME.TensorField(coordinates=coords.cuda(), features=feats.cuda()).sparse()
        ro, ho = ref(rx), hip(hx)
        assert torch.allclose(ho.F.detach().cpu().double(), ro.F.detach(), atol=1e-4, rtol=1e-4)
        g = torch.randn(ro.F.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
        ro.F.backward(g), ho.F.backward(g.float().cuda())
        for (k, p), q in zip(hip.named_parameters(), ref.parameters()):
            e = float((p.grad.cpu().double() - q.grad).norm() / q.grad.norm().clamp_min(1e-12))
            assert e < 2e-2, (norm_type, k, e)
