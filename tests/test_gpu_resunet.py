"""-m gpu: the registration networks (co3d_3d/src/models/mink/resunet.py) on the HIP backend against the CPU oracle: first the
operators the family adds -- convolution k=3 s=2 down, transposed convolution k=3 s=2 back onto the encoder's map (a fine voxel
has up to eight parents), cat -- under the bounds of test_gpu_unet.py::test_down_up_convolutions_match_oracle, then
ResUNetBN2C / ResUNetIN2C forward + backward under the criteria of test_res16unet_matches_oracle, and eval mode."""
import pytest
import torch

from helpers import batch_scenes

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cin,cmid,cout", [(28, 32, 48), (20, 160, 36)])
def test_down_up_convolutions_kernel3_match_oracle(oracle_maps, cin, cmid, cout):
    from nerf_downstream_amd import minkowski as ME
    from oracle import me_cpu as OME

    torch.manual_seed(0)
    coords, feats = batch_scenes([21, 22, 23], grid=32, cin=cin)
    rdown = OME.MinkowskiConvolution(cin, cmid, kernel_size=3, stride=2, dimension=3)
    rup = OME.MinkowskiConvolutionTranspose(cmid, cout, kernel_size=3, stride=2, bias=True, dimension=3)
    hdown = ME.MinkowskiConvolution(cin, cmid, kernel_size=3, stride=2, dimension=3).cuda()
    hup = ME.MinkowskiConvolutionTranspose(cmid, cout, kernel_size=3, stride=2, bias=True, dimension=3).cuda()
    assert hdown.kernel.shape == (27, cin, cmid) and hup.kernel.shape == (27, cmid, cout)
    assert float(hup.kernel.detach().abs().max()) <= (cout * 27) ** -0.5  # initialised from the OUT channels
    hdown.load_state_dict(rdown.state_dict()), hup.load_state_dict(rup.state_dict())

    rtf = OME.TensorField(coordinates=coords, features=feats)
    rx = rtf.sparse()
    rF = rx.F.detach().clone().requires_grad_(True)
    ry = rdown(OME.SparseTensor(rF, rx.coordinate_map_key, rx._manager))
    rz = rup(ry)
    rc = OME.cat(rz, rx).F

    htf = ME.TensorField(coordinates=coords.cuda(), features=feats.cuda())
    hx = htf.sparse()
    hF = hx.F.detach().clone().requires_grad_(True)
    hy = hdown(ME.SparseTensor(hF, hx.coordinate_map_key, hx.coordinate_manager))
    hz = hup(hy)
    hc = ME.cat(hz, hx).F
    assert hy.tensor_stride[0] == 2 and hz.tensor_stride[0] == 1 and hz.coordinate_map_key == hx.coordinate_map_key
    assert torch.equal(hx.C.cpu(), rx.C) and torch.equal(hy.C.cpu(), ry.C)  # canonical (first-occurrence) order on both sides
    nbr, _ = hx.coordinate_manager.kernel_table(hx.coordinate_map_key, hy.coordinate_map_key, 3, 1, transposed=True)
    print(f"[resunet] k3 s2 ({cin}, {cmid}, {cout}): y max|diff| {float((hy.F.cpu() - ry.F).abs().max()):.2e}, "
          f"z max|diff| {float((hz.F.cpu() - rz.F).abs().max()):.2e}")
    assert torch.allclose(hy.F.cpu(), ry.F, atol=2e-5, rtol=1e-5)
    assert torch.allclose(hz.F.cpu(), rz.F, atol=2e-5, rtol=1e-5)
    assert torch.allclose(hc.cpu(), rc, atol=2e-5, rtol=1e-5) and hc.shape == (hx.F.shape[0], cout + cin)
    g = torch.randn_like(rz.F)
    rz.F.backward(g)
    hz.F.backward(g.cuda())
    assert torch.allclose(hF.grad.cpu(), rF.grad, atol=2e-5, rtol=1e-4)
    for h, r in ((hdown, rdown), (hup, rup)):
        scale = float(r.kernel.grad.abs().max())
        assert torch.allclose(h.kernel.grad.cpu(), r.kernel.grad, atol=2e-5 * max(scale, 1.0), rtol=1e-4)
    assert torch.allclose(hup.bias.grad.cpu(), rup.bias.grad, atol=1e-4, rtol=1e-5)
    assert int((nbr >= 0).sum()) > hx.F.shape[0]  # more (fine, coarse) pairs than fine voxels: some voxel has several parents


def _pair(name, normalize):
    from nerf_downstream_amd.co3d_3d.src.models import MODELS
    from oracle import me_cpu as OME

    torch.manual_seed(0)
    ref = MODELS[name](3, 32, normalize_feature=normalize, ME=OME)
    hip = MODELS[name](3, 32, normalize_feature=normalize).cuda()
    hip.load_state_dict(ref.state_dict())
    return ref, hip


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("name", ["ResUNetBN2C", "ResUNetIN2C"])
def test_resunet_matches_oracle(oracle_maps, name, normalize):
    from nerf_downstream_amd import minkowski as ME

    ref, hip = _pair(name, normalize)
    coords, feats = batch_scenes([31, 32, 33], grid=48, cin=3)
    out = hip(hip.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
    oout = ref(ref.process_input({"coordinates": coords, "features": feats}))
    assert isinstance(out, ME.SparseTensor) and out.tensor_stride[0] == 1
    n = coords.shape[0]
    assert out.F.shape == (n, 32) == oout.F.shape and torch.equal(out.C.cpu(), oout.C)
    print(f"[resunet] {name} normalize={normalize}: out max|diff| {float((out.F.detach().cpu() - oout.F.detach()).abs().max()):.2e}")
    assert torch.allclose(out.F.detach().cpu(), oout.F.detach(), atol=1e-3), (out.F.detach().cpu() - oout.F.detach()).abs().max()
    if normalize:
        assert float((out.F.detach().norm(dim=1) - 1).abs().max()) < 1e-5
    G = torch.randn(n, 32, generator=torch.Generator().manual_seed(1))
    ((out.F * G.cuda()).sum() / n).backward()
    ((oout.F * G).sum() / n).backward()
    hp, rp = dict(hip.named_parameters()), dict(ref.named_parameters())
    assert hp.keys() == rp.keys()
    rel = {k: float((hp[k].grad.cpu().double() - rp[k].grad.double()).norm() / rp[k].grad.double().norm().clamp_min(1e-12)) for k in hp}
    errs = sorted(rel.values())
    flat_g = torch.cat([hp[k].grad.cpu().double().flatten() for k in hp])
    flat_o = torch.cat([rp[k].grad.double().flatten() for k in hp])
    cos = float(torch.dot(flat_g, flat_o) / (flat_g.norm() * flat_o.norm()))
    print(f"[resunet] {name} normalize={normalize}: gradient relative error max {errs[-1]:.3e} "
          f"({max(rel.items(), key=lambda kv: kv[1])[0]}), median {errs[len(errs) // 2]:.3e}, cosine {cos:.6f}")
    assert max(rel.values()) < 0.15, max(rel.items(), key=lambda kv: kv[1])
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]  # see test_gpu_resnet.py on ReLU flips
    assert cos > 0.999
    hb, rb = dict(hip.named_buffers()), dict(ref.named_buffers())
    assert hb.keys() == rb.keys()
    for k in hb:
        assert torch.allclose(hb[k].float().cpu(), rb[k].float(), atol=1e-3, rtol=1e-3), k


@pytest.mark.parametrize("name", ["ResUNetBN2C", "ResUNetIN2C"])
def test_resunet_eval_mode_matches_oracle(oracle_maps, name):
    ref, hip = _pair(name, True)
    coords, feats = batch_scenes([31, 32], grid=48, cin=3)
    with torch.no_grad():  # one training step's worth of running statistics first, so that eval mode has something to use
        ref(ref.process_input({"coordinates": coords, "features": feats}))
    hip.load_state_dict(ref.state_dict())
    ref.eval(), hip.eval()
    with torch.no_grad():
        out = hip(hip.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
        oout = ref(ref.process_input({"coordinates": coords, "features": feats}))
    assert out.F.shape == oout.F.shape == (coords.shape[0], 32)
    assert torch.allclose(out.F.cpu(), oout.F, atol=1e-3), (out.F.cpu() - oout.F).abs().max()
    # a SparseTensor goes in as the reference's forward takes it
    field = hip.process_input({"coordinates": coords.cuda(), "features": feats.cuda()})
    with torch.no_grad():
        assert torch.equal(hip(field.sparse()).F, hip(field).F)
