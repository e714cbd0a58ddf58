"""PowerNorm without a GPU: the float64 restatement (tests/pn_restate.py) against the recorded run of the reference's
MaskPowerNorm (tests/golden/powernorm_ref_v1.npz, scripts/make_powernorm_golden.py) and against torch's autograd for the group
scaling; the module's state dict; convert_powernorm on whole networks; the train / evaluate switches; and the argument
checks of the C ABI, which come before any launch."""
import inspect
import os

import numpy as np
import pytest
import torch

import pn_restate as PR
from nerf_downstream_amd import gin_lite as gin

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "powernorm_ref_v1.npz")
CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "nerf_downstream_amd", "co3d_3d", "configs")
TOL = 1e-12


def _close(got, ref, what):
    ref = torch.as_tensor(ref, dtype=torch.float64).reshape(got.shape)
    err = float((got - ref).abs().max())
    assert err <= TOL, f"{what}: off by {err:.3e}"


@pytest.mark.parametrize("cfg", ["a", "b"])
def test_restatement_reproduces_the_recorded_reference_run(cfg):
    """Five training steps (warmup_iters = 2: it < W, it == W, it > W, a non-zero ema_gz from step 2 on) and the eval forward:
    y, the three gradients, both buffers and the counter, to 1e-12."""
    d = np.load(GOLDEN)
    k = lambda name: d[f"{cfg}_{name}"]  # noqa: E731
    G, W = int(k("group_num")), int(k("warmup_iters"))
    assert (G, W) == ({"a": 3, "b": 1}[cfg], 2)
    eps, afwd, abkw = float(k("eps")), float(k("alpha_fwd")), float(k("alpha_bkw"))
    w, b = torch.from_numpy(k("weight")), torch.from_numpy(k("bias"))
    state = PR.State.fresh(w.numel())
    for s in range(int(d["steps"])):
        x, dy = torch.from_numpy(k(f"s{s}_x")), torch.from_numpy(k(f"s{s}_dy"))
        y, aux, mid = PR.forward(x, w, b, state, eps, afwd, W, G)
        dx, dw, db, dres, state, _ = PR.backward(dy, aux, w, mid, eps, abkw)
        what = f"config {cfg} step {s}"
        _close(y, k(f"s{s}_y"), what + " y")
        _close(dx, k(f"s{s}_dx"), what + " dx")
        _close(dw, k(f"s{s}_dweight"), what + " dweight")
        _close(db, k(f"s{s}_dbias"), what + " dbias")
        _close(state.running_phi, k(f"s{s}_running_phi"), what + " running_phi")
        _close(state.ema_gz, k(f"s{s}_ema_gz"), what + " ema_gz")
        assert state.iters == int(k(f"s{s}_iters")[0]) == s + 1
        assert torch.equal(dres, dy)
        if s >= 1:
            assert float(torch.from_numpy(k(f"s{s}_ema_gz")).abs().min()) > 0  # the backward really ran with a non-zero state
    ye, _, after = PR.forward(torch.from_numpy(k("eval_x")), w, b, state, eps, afwd, W, G, training=False)
    _close(ye, k("eval_y"), f"config {cfg} eval y")
    assert after.iters == state.iters and torch.equal(after.running_phi, state.running_phi)


@pytest.mark.parametrize("C,G", [(12, 3), (12, 1), (6, 6), (5, 1)])
def test_group_scaling_derivative_matches_autograd(C, G):
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(23, C, generator=g, dtype=torch.float64) * 3 + 1).requires_grad_(True)
    dxh = torch.randn(23, C, generator=g, dtype=torch.float64)
    xg = x.reshape(23, G, C // G)
    xh_t = (xg / torch.sqrt((xg * xg).mean(2, keepdim=True) + 1e-5)).reshape(23, C)
    xh_t.backward(dxh)
    r, xh = PR.group_scale(x, G)
    _close(xh, xh_t.detach(), "xh")
    _close(PR.group_scale_bwd(dxh, r, xh, G), x.grad, "dx through the group scaling")


def test_fused_tail_of_the_restatement():
    """residual add and ReLU: y and the masked gradients, against autograd on the differentiable eval form."""
    g = torch.Generator().manual_seed(4)
    C, G = 8, 2
    x = (torch.randn(19, C, generator=g, dtype=torch.float64) * 3 + 1).requires_grad_(True)
    res = torch.randn(19, C, generator=g, dtype=torch.float64).requires_grad_(True)
    w = torch.linspace(0.5, 1.5, C, dtype=torch.float64).requires_grad_(True)
    b = torch.linspace(-0.2, 0.2, C, dtype=torch.float64).requires_grad_(True)
    dy = torch.randn(19, C, generator=g, dtype=torch.float64)
    st = PR.State(torch.linspace(0.5, 2.0, C), torch.zeros(C), 7)
    xg = x.reshape(19, G, C // G)
    xh = (xg / torch.sqrt((xg * xg).mean(2, keepdim=True) + 1e-5)).reshape(19, C)
    yt = torch.relu(w * xh / torch.sqrt(st.running_phi + 1e-5) + b + res)
    yt.backward(dy)
    y, aux, _ = PR.forward(x, w, b, st, 1e-5, groups=G, training=False, residual=res, relu=True)
    dx, dw, db, dres, after, _ = PR.backward(dy, aux, w, st, 1e-5, relu=True)
    for got, ref, what in ((y, yt.detach(), "y"), (dx, x.grad, "dx"), (dw, w.grad, "dweight"), (db, b.grad, "dbias"), (dres, res.grad, "dresidual")):
        _close(got, ref, what)
    assert torch.equal(after.ema_gz, st.ema_gz)


# ------------------------------------------------------------------------------------------------ the module
def test_state_dict_keys_shapes_and_dtypes():
    from nerf_downstream_amd import minkowski as ME

    m = ME.MinkowskiPowerNorm(12, eps=1e-4, alpha_fwd=0.8, alpha_bkw=0.7, affine=False, warmup_iters=5, group_num=3)
    sd = m.state_dict()
    assert {k: (tuple(v.shape), v.dtype) for k, v in sd.items()} == {
        "pn.weight": ((12,), torch.float32), "pn.bias": ((12,), torch.float32), "pn.running_phi": ((1, 12, 1, 1), torch.float32),
        "pn.ema_gz": ((1, 12, 1, 1), torch.float32), "pn.iters": ((1,), torch.int64)}
    assert [n for n, _ in m.named_parameters()] == ["pn.weight", "pn.bias"]  # parameters whatever `affine` says
    assert bool((sd["pn.running_phi"] == 1).all()) and bool((sd["pn.ema_gz"] == 0).all()) and int(sd["pn.iters"]) == 0
    assert repr(m) == "MinkowskiPowerNorm(12, eps=0.0001, affine=False, alpha_fwd=0.8, alpha_bkw=0.7, warmup_iters=5, group_num=3)"
    assert ME.MinkowskiPowerNorm.__name__ == "MinkowskiPowerNorm" and "MinkowskiPowerNorm" in dir(ME)


def test_reference_layout_state_dict_loads():
    """A checkpoint written by the reference's module: the same five keys, float32 / int64."""
    from nerf_downstream_amd import minkowski as ME

    ref = {"pn.weight": torch.rand(8), "pn.bias": torch.rand(8), "pn.running_phi": torch.rand(1, 8, 1, 1) + 0.5,
           "pn.ema_gz": torch.rand(1, 8, 1, 1), "pn.iters": torch.tensor([41], dtype=torch.int64)}
    m = ME.MinkowskiPowerNorm(8)
    m.load_state_dict(ref, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ref[k]) and v.dtype == ref[k].dtype, k


def test_channels_not_divisible_by_the_groups_are_refused():
    from nerf_downstream_amd import minkowski as ME

    with pytest.raises(ValueError, match="divide"):
        ME.MinkowskiPowerNorm(10, group_num=4)
    with pytest.raises(ValueError, match="divide"):
        ME.MinkowskiPowerNorm(10, group_num=0)
    ME.MinkowskiPowerNorm(10, group_num=10), ME.MinkowskiPowerNorm(10, group_num=5)


def test_gin_configures_the_module():
    from nerf_downstream_amd import minkowski as ME

    gin.clear_config()
    try:
        gin.parse_config("MinkowskiPowerNorm.warmup_iters = 3\nMinkowskiPowerNorm.group_num = 2")
        m = ME.MinkowskiPowerNorm(8)
        assert (m.pn.warmup_iters, m.pn.group_num) == (3, 2)
    finally:
        gin.clear_config()


@pytest.mark.parametrize("name,cin,cout", [("Res16UNet14", 3, 8), ("ResNet14", 28, 51)])
def test_convert_powernorm_replaces_every_batch_norm(name, cin, cout):
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models import get_model

    torch.manual_seed(0)
    model = get_model(name, cin, cout)
    bns = {n: m for n, m in model.named_modules() if isinstance(m, ME.MinkowskiBatchNorm)}
    assert len(bns) >= 10
    with torch.no_grad():
        for i, m in enumerate(bns.values()):  # make the statistics distinguishable
            m.bn.running_var.uniform_(0.5, 2.0), m.bn.running_mean.fill_(3.0), m.bn.num_batches_tracked.fill_(i + 1)
    keys_before = set(model.state_dict())
    out = ME.MinkowskiPowerNorm.convert_powernorm(model)
    assert out is model
    assert not [n for n, m in model.named_modules() if isinstance(m, (ME.MinkowskiBatchNorm, torch.nn.BatchNorm1d))]
    pns = {n: m for n, m in model.named_modules() if isinstance(m, ME.MinkowskiPowerNorm)}
    assert sorted(pns) == sorted(bns)
    for i, (n, old) in enumerate(bns.items()):
        new = pns[n].pn
        assert new.weight is old.bn.weight and new.bias is old.bn.bias, n
        assert new.running_phi.shape == (1, old.bn.num_features, 1, 1) and torch.equal(new.running_phi.reshape(-1), old.bn.running_var)
        assert new.iters.shape == (1,) and new.iters.dtype == torch.int64 and int(new.iters) == i + 1
        assert (new.eps, new.affine, new.num_features) == (old.bn.eps, old.bn.affine, old.bn.num_features)
        assert bool((new.ema_gz == 0).all()) and pns[n].training == old.training
    keys = set(model.state_dict())
    assert not [k for k in keys if "running_mean" in k or ".bn." in k]
    assert {k.replace(".pn.running_phi", ".bn.running_var").replace(".pn.iters", ".bn.num_batches_tracked").replace(".pn.", ".bn.")
            for k in keys if ".pn.ema_gz" not in k} == {k for k in keys_before if "running_mean" not in k}
    assert len(list(model.parameters())) == len({id(p) for p in model.parameters()})
    # what the network cached about its batch norms is gone: no counter left to bump, no native-trunk plan
    assert getattr(model, "_norms", []) == [] and getattr(model, "_trunk_plan", None) is None


def test_converted_fresh_network_equals_one_with_power_norms():
    """Freshly initialised and converted == the same state dict as building MinkowskiPowerNorm layers directly."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models import get_model

    model = ME.MinkowskiPowerNorm.convert_powernorm(get_model("ResNet14", 4, 5))
    for n, m in model.named_modules():
        if isinstance(m, ME.MinkowskiPowerNorm):
            fresh = ME.MinkowskiPowerNorm(m.pn.num_features, eps=m.pn.eps, affine=m.pn.affine)
            for k, v in fresh.state_dict().items():
                assert torch.equal(v, m.state_dict()[k]) and v.dtype == m.state_dict()[k].dtype, (n, k)
            assert repr(fresh) == repr(m)


def test_switches_are_gin_parameters_and_refused_with_the_oracle(tmp_path):
    from nerf_downstream_amd.co3d_3d import eval as E
    from nerf_downstream_amd.co3d_3d import train as T
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from oracle import me_cpu as OME

    assert inspect.signature(T.train).parameters["convert_powernorm"].default is False
    assert inspect.signature(E.evaluate).parameters["convert_powernorm"].default is False
    assert not hasattr(OME, "MinkowskiPowerNorm")
    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings(
            [f"{CFG}/co3d_cls.gin", f"{CFG}/synthetic_seg.gin", f"{CFG}/res16unet.gin"],
            ["train.gpus=0", "train.max_steps=1", "train.batch_size=2", "train.val_batch_size=2", "SparseVoxelSegDataset.grid=16",
             "SparseVoxelSegDataset.num_samples=4", "train.convert_powernorm=True", "evaluate.convert_powernorm=True"],
        )
        with pytest.raises(ValueError, match="MinkowskiPowerNorm"):
            T.train(save_path=str(tmp_path), resume_training=False, run_name="s", run_name_postfix=None, ME=OME)
        model = get_model(ME=OME)
        ckpt = str(tmp_path / "bn.ckpt")
        torch.save({"state_dict": {"model." + k: v for k, v in model.state_dict().items()}}, ckpt)
        with pytest.raises(ValueError, match="MinkowskiPowerNorm"):
            E.evaluate(save_path=str(tmp_path / "eval"), load_path=ckpt, tag="t", ME=OME)
        assert not os.path.exists(tmp_path / "eval" / "t.json")
    finally:
        gin.clear_config()
    # the two pinned spellings stay refused, each with a hint at the route that works
    from nerf_downstream_amd.co3d_3d.src.models.mink.modules.common import get_norm

    with pytest.raises(ValueError, match="PN.*not implemented.*convert_powernorm"):
        get_norm("PN", 8)
    assert "evaluate.convert_powernorm=True" in E.POWERNORM_HINT and E.main(["--convert_powernorm", "--load_path", "x"]) == 2


# ------------------------------------------------------------------------------------------------ the C ABI, before any launch
def test_c_abi_argument_checks_without_a_device():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    assert _lib.CONSTANTS["MINK_PN_MAX_C"] == 4096 and _lib.CONSTANTS["MINK_ABI_VERSION"] == 4  # additive
    P = 1 << 20  # dummy non-NULL pointer, 16-byte aligned: every check comes before the first launch
    need = L.mink_pn_workspace_bytes(1000, 64, 4)
    assert need > 0 and L.mink_pn_workspace_bytes(1000, 64, 1) == need  # the partials do not depend on the groups
    assert L.mink_pn_workspace_bytes(10, 4097, 1) == 0 and L.mink_pn_workspace_bytes(10, 10, 4) == 0 and L.mink_pn_workspace_bytes(-1, 8, 1) == 0

    def fwd(n=1000, C=64, G=4, ldx=None, ws=need, x=P, iters=P):
        return L.mink_pn_fwd(x, C if ldx is None else ldx, n, C, G, 1e-5, 0.9, 2, P, P, None, 0, P, P, P, P, P, iters, P, ws, None)

    def bwd(n=1000, C=64, G=4, ws=need, relu=0, y=None, training=1, ema=P):
        return L.mink_pn_bwd(P, P, C, y, n, C, G, 1e-5, 0.9, training, P, P, P, P, relu, ema, P, None, P, P, P, ws, None)

    for call, text in ((lambda: fwd(C=4097, G=1), b"1 <= C <= 4096"), (lambda: fwd(C=10, G=4), b"groups must divide C"),
                       (lambda: fwd(G=0), b"groups"), (lambda: fwd(n=0), b"no rows"), (lambda: fwd(ldx=63), b"row pitch"),
                       (lambda: fwd(x=None), b"NULL"), (lambda: fwd(iters=P + 4), b"8-byte"), (lambda: fwd(ws=need - 1), b"workspace"),
                       (lambda: bwd(C=4097, G=1), b"1 <= C <= 4096"), (lambda: bwd(n=0), b"no rows"), (lambda: bwd(ws=need - 1), b"workspace"),
                       (lambda: bwd(relu=1), b"ReLU needs the forward output"), (lambda: bwd(ema=None), b"ema_gz"),
                       (lambda: L.mink_pn_apply(P, 64, 10, 64, 3, 1e-5, P, P, P, None, 0, P, P, P, None), b"groups must divide C"),
                       (lambda: L.mink_pn_apply(None, 64, 10, 64, 4, 1e-5, P, P, P, None, 0, P, P, P, None), b"NULL")):
        assert call() == -1
        assert text in L.mink_last_error(), (text, L.mink_last_error())
    assert fwd(ws=need - 1) == -1 and str(need).encode() in L.mink_last_error()
    assert L.mink_pn_apply(None, 64, 0, 64, 4, 1e-5, None, None, None, None, 0, None, None, None, None) == 0  # eval, no rows: nothing to do
