"""-m gpu: PowerNorm (csrc/powernorm.hip, MinkowskiPowerNorm, convert_powernorm) against the float64 restatement of
tests/pn_restate.py, every comparison within the fp32 bounds that file derives (factor 1: measured error <= bound).

The operator on non-centred inputs (mean 1, scale 3) over row counts around the wave / chunk boundaries and channel / group
shapes on both lane widths, in all three warm-up regimes and with a non-zero ema_gz; a four-step sequence through the module
with the buffers compared after every step, then eval; bitwise reproducibility; no host synchronisation; guard bands through
the C ABI; NaN / inf footprints; converted Res16UNet14 / ResNet14 for three training steps with every PowerNorm layer held to
the restatement on its recorded input; and the train / evaluate switches on the synthetic segmentation set.

ReLU: the forward is compared with float64's own decisions (a flipped decision is an error of |pre-activation|, which the
bound must cover); the restatement's backward runs under the kernel's decisions (y > 0)."""
import json
import os

import pytest
import torch
import torch.nn.functional as F

import footprint as FP
import pn_restate as PR
from guarded import Guarded, assert_finite, check_all
from helpers import batch_scenes, trunk_node
from nerf_downstream_amd import gin_lite as gin

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "nerf_downstream_amd", "co3d_3d", "configs")
VARIANTS = [(False, False), (True, False), (False, True), (True, True)]  # (relu, residual)
# fp32-representable settings: the restatement then computes with exactly the numbers the kernels are handed
HP = dict(eps=PR.f32(1e-5), alpha_fwd=PR.f32(0.9), alpha_bkw=PR.f32(0.9), warmup_iters=2)
WORST = {}  # quantity -> worst measured error / bound over the module's tests (printed; scripts/powernorm_bench.py records its own)


def _inputs(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * 3 + 1
    dy = torch.randn(n, C, generator=g)
    res = torch.randn(n, C, generator=g)
    w, b = torch.linspace(0.5, 1.5, C), torch.linspace(-0.2, 0.2, C)
    return x, dy, res, w, b


def _state(C, iters, seed=0):
    """A state with fp32-representable buffers: running_phi in [0.5, 2), a non-zero ema_gz once a step has been taken."""
    g = torch.Generator().manual_seed(100 + seed)
    phi = torch.rand(C, generator=g) * 1.5 + 0.5 if iters else torch.ones(C)
    ema = (torch.rand(C, generator=g) - 0.5) * 0.2 if iters else torch.zeros(C)
    return PR.State(phi, ema, iters)


def _run(x, dy, res, w, b, state, groups, relu, residual, training=True, hp=HP):
    """One forward + backward of PowerNormFunction from `state` -> dict of host tensors (y, dx, dw, db, dres, phi, ema, iters)."""
    from nerf_downstream_amd.minkowski import functional as Fn

    C = x.shape[1]
    phi = state.running_phi.float().reshape(1, C, 1, 1).cuda()
    ema = state.ema_gz.float().reshape(1, C, 1, 1).cuda()
    iters = torch.tensor([state.iters], dtype=torch.int64, device="cuda")
    leaves = [t.clone().cuda().requires_grad_(True) for t in (x, w, b)]
    r = res.clone().cuda().requires_grad_(True) if residual else None
    y = Fn.PowerNormFunction.apply(leaves[0], leaves[1], leaves[2], phi, ema, iters, training, hp["eps"], hp["alpha_fwd"],
                                   hp["alpha_bkw"], hp["warmup_iters"], groups, r, relu)
    y.backward(dy.cuda())
    return dict(y=y.detach().cpu(), dx=leaves[0].grad.cpu(), dw=leaves[1].grad.cpu(), db=leaves[2].grad.cpu(),
                dres=r.grad.cpu() if residual else None, phi=phi.reshape(-1).cpu(), ema=ema.reshape(-1).cpu(), iters=int(iters.cpu()))


def _restate(x, dy, res, w, b, state, groups, relu, residual, training, y_gpu, hp=HP):
    """-> (references, bounds) as dicts over y, dx, dw, db, dres, phi, ema (+ iters in the references)."""
    r = res if residual else None
    y, aux, mid = PR.forward(x, w, b, state, hp["eps"], hp["alpha_fwd"], hp["warmup_iters"], groups, training, r, relu)
    mask = (y_gpu > 0) if relu else None
    dx, dw, db, dres, after, bw = PR.backward(dy, aux, w, mid, hp["eps"], hp["alpha_bkw"], relu, mask)
    dx_b, dw_b, db_b, ema_b = PR.grad_bounds(aux, bw, w, mid, hp["alpha_bkw"], (dx, dw, db, after.ema_gz))
    ref = dict(y=y, dx=dx, dw=dw, db=db, dres=dres, phi=after.running_phi, ema=after.ema_gz, iters=after.iters)
    bnd = dict(y=PR.forward_bound(aux, y), dx=dx_b, dw=dw_b, db=db_b, ema=ema_b,
               phi=PR.phi_bound(aux, state, after, hp["alpha_fwd"], hp["warmup_iters"]) if training else None)
    return ref, bnd


def _hold(got, ref, bnd, training, residual, what):
    for k in ("y", "dx", "dw", "db") + (("phi", "ema") if training else ()):
        assert got[k].shape == ref[k].shape, (what, k)
        assert_finite(got[k], f"{what} {k}")
        err = (got[k].double() - ref[k]).abs()
        ratio = float((err / bnd[k]).max())
        WORST[k] = max(WORST.get(k, 0.0), ratio)
        assert ratio <= 1.0, f"{what} {k}: error / bound = {ratio:.3f} (max |err| {float(err.max()):.3e})"
    if not training:
        assert torch.equal(got["phi"].double(), ref["phi"]) and torch.equal(got["ema"].double(), ref["ema"]), what + ": eval changed a buffer"
    assert got["iters"] == ref["iters"], (what, got["iters"], ref["iters"])
    if residual:
        assert torch.equal(got["dres"].double(), ref["dres"]), what + " dresidual"


# ------------------------------------------------------------------------------------------------ the operator
SHAPES = [(1, 1), (3, 1), (6, 3), (12, 3), (32, 1), (32, 4), (96, 96), (256, 2)]


@pytest.mark.parametrize("C,G", SHAPES)
def test_operator_matches_float64_within_the_bounds(C, G):
    """Rows on / off a wave (63, 65), more than one chunk of 256 (257), many chunks and an odd count (4099), one row.  The
    four tail variants start at iters = 0, 1, 2, 3 with warmup_iters = 2: it < W, it == W, it > W twice, ema_gz non-zero."""
    for n in (1, 63, 65, 257, 4099):
        x, dy, res, w, b = _inputs(n, C, 7 + n)
        for it0, (relu, residual) in enumerate(VARIANTS):
            st = _state(C, it0, seed=n)
            got = _run(x, dy, res, w, b, st, G, relu, residual)
            ref, bnd = _restate(x, dy, res, w, b, st, G, relu, residual, True, got["y"])
            _hold(got, ref, bnd, True, residual, f"PN n={n} C={C} G={G} relu={relu} res={residual} iters={it0}")
    print(f"\n[PN C={C} G={G}] worst error / bound so far: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))


@pytest.mark.parametrize("G", [1, 4096])
def test_widest_layer(G):
    from nerf_downstream_amd._lib import CONSTANTS

    C, n = CONSTANTS["MINK_PN_MAX_C"], 65
    assert C == 4096 >= 2048  # the Bottleneck nets' widest layer is 512 * 4
    x, dy, res, w, b = _inputs(n, C, 11)
    st = _state(C, 1)
    got = _run(x, dy, res, w, b, st, G, True, True)
    ref, bnd = _restate(x, dy, res, w, b, st, G, True, True, True, got["y"])
    _hold(got, ref, bnd, True, True, f"PN n={n} C={C} G={G}")
    from nerf_downstream_amd import minkowski as ME

    with pytest.raises(ValueError, match="at most 4096"):
        _run(*_inputs(4, C + 4, 1), PR.State.fresh(C + 4), 1, False, False)
    assert ME.MinkowskiPowerNorm(C + 4) is not None  # (construction is free; the refusal comes with the first rows)


def test_eval_mode_and_its_backward():
    for C, G in ((12, 3), (32, 4)):
        x, dy, res, w, b = _inputs(130, C, 5)
        st = _state(C, 5)
        for relu, residual in VARIANTS:
            got = _run(x, dy, res, w, b, st, G, relu, residual, training=False)
            ref, bnd = _restate(x, dy, res, w, b, st, G, relu, residual, False, got["y"])
            _hold(got, ref, bnd, False, residual, f"PN eval C={C} G={G} relu={relu} res={residual}")


def test_no_rows():
    """Training mode: refused before any launch (the reference would write NaN into running_phi); eval: the empty result."""
    x, dy, res, w, b = _inputs(0, 8, 1)
    st = _state(8, 1)
    with pytest.raises(ValueError, match="at least one row"):
        _run(x, dy, res, w, b, st, 2, True, True)
    got = _run(x, dy, res, w, b, st, 2, True, True, training=False)
    assert got["y"].shape == (0, 8) and got["dx"].shape == (0, 8) and got["dres"].shape == (0, 8)
    assert not got["dw"].any() and not got["db"].any() and got["iters"] == 1
    assert torch.equal(got["phi"].double(), st.running_phi) and torch.equal(got["ema"].double(), st.ema_gz)
    from nerf_downstream_amd.minkowski import functional as Fn

    with pytest.raises(ValueError, match="not divisible"):
        Fn.PowerNormFunction.apply(torch.zeros(4, 10, device="cuda"), torch.ones(10, device="cuda"), torch.zeros(10, device="cuda"),
                                   torch.ones(10, device="cuda"), torch.zeros(10, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda"),
                                   True, 1e-5, 0.9, 0.9, 2, 4, None, False)


def test_two_runs_are_bitwise_equal():
    for C, G, n in ((12, 3, 4099), (32, 1, 4099), (256, 2, 700)):
        x, dy, res, w, b = _inputs(n, C, 3)
        st = _state(C, 1)
        a, c = _run(x, dy, res, w, b, st, G, True, True), _run(x, dy, res, w, b, st, G, True, True)
        for k in ("y", "dx", "dw", "db", "dres", "phi", "ema"):
            assert torch.equal(a[k], c[k]), (C, G, k)
        assert a["iters"] == c["iters"] == 2


# ------------------------------------------------------------------------------------------------ the module
def _sparse(x):
    from nerf_downstream_amd import minkowski as ME

    coords = torch.zeros(x.shape[0], 4)
    coords[:, 1] = torch.arange(x.shape[0])
    field = ME.TensorField(coordinates=coords.cuda(), features=x.detach())
    return ME.SparseTensor(x, ME.CoordinateMapKey(1), field.coordinate_manager)


def _module(C, G, w, b):
    from nerf_downstream_amd import minkowski as ME

    mod = ME.MinkowskiPowerNorm(C, eps=HP["eps"], alpha_fwd=HP["alpha_fwd"], alpha_bkw=HP["alpha_bkw"], warmup_iters=HP["warmup_iters"],
                                group_num=G).cuda()
    with torch.no_grad():
        mod.pn.weight.copy_(w), mod.pn.bias.copy_(b)
    return mod


def _module_state(mod):
    return PR.State(mod.pn.running_phi, mod.pn.ema_gz, int(mod.pn.iters))


@pytest.mark.parametrize("C,G", [(12, 3), (32, 1)])
def test_four_step_sequence_then_eval(C, G):
    """warmup_iters = 2: steps 1..4 cross it < W, it == W, it > W (twice); ema_gz is non-zero from step 2 on.  Every step is
    restated from the module's own buffers before it, and outputs, gradients, both buffers and the counter are compared after it."""
    from nerf_downstream_amd import minkowski as ME

    n = 300
    _, _, _, w, b = _inputs(n, C, 0)
    mod = _module(C, G, w, b).train()
    seen_ema = False
    for step in range(4):
        x, dy, res, _, _ = _inputs(n, C, 40 + step)
        before = _module_state(mod)
        assert before.iters == step
        seen_ema = seen_ema or bool(before.ema_gz.abs().max() > 0)
        xs, rs = x.clone().cuda().requires_grad_(True), res.clone().cuda().requires_grad_(True)
        st = _sparse(xs)
        mod.pn.weight.grad = mod.pn.bias.grad = None
        out = mod(st, relu=True, residual=ME.SparseTensor(rs, st.coordinate_map_key, st.coordinate_manager))
        assert isinstance(out, ME.SparseTensor) and out.coordinate_map_key == st.coordinate_map_key
        out.F.backward(dy.cuda())
        after = _module_state(mod)
        got = dict(y=out.F.detach().cpu(), dx=xs.grad.cpu(), dw=mod.pn.weight.grad.cpu(), db=mod.pn.bias.grad.cpu(), dres=rs.grad.cpu(),
                   phi=after.running_phi.float(), ema=after.ema_gz.float(), iters=after.iters)
        ref, bnd = _restate(x, dy, res, w, b, before, G, True, True, True, got["y"])
        _hold(got, ref, bnd, True, True, f"PN module C={C} G={G} step {step + 1}")
    assert seen_ema and int(mod.pn.iters) == 4
    mod.eval()
    x, dy, res, _, _ = _inputs(n, C, 50)
    before = _module_state(mod)
    field = ME.TensorField(coordinates=torch.cat([torch.zeros(n, 1), torch.rand(n, 3) * 20], 1).cuda(), features=x.cuda())
    with torch.no_grad():
        out = mod(field)
    assert isinstance(out, ME.TensorField) and out.coordinate_manager is field.coordinate_manager  # a field in, a field out
    y, aux, _ = PR.forward(x, w, b, before, HP["eps"], groups=G, training=False)
    assert bool(((out.F.cpu().double() - y).abs() <= PR.forward_bound(aux, y)).all())
    after = _module_state(mod)
    assert after.iters == 4 and torch.equal(after.running_phi, before.running_phi) and torch.equal(after.ema_gz, before.ema_gz)


def test_no_host_synchronisation():
    """Forward and backward in training mode, inside and after warm-up, under torch's sync debug mode: the counter, the
    warm-up branch and the buffer updates never come back to the host (the reference reads iters with .item() per layer)."""
    C, n = 32, 1000
    x, dy, res, w, b = _inputs(n, C, 9)
    mod = _module(C, 4, w, b).train()
    xs = x.clone().cuda().requires_grad_(True)
    st = _sparse(xs)
    mod(st)  # (the scratch buffer and the map exist after the first call)
    dyd = dy.cuda()  # (a copy from pageable host memory synchronises: made before the guarded region)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        for _ in range(3):  # iters 2, 3, 4 with warmup_iters = 2: both branches
            out = mod(st, relu=True)
            out.F.backward(dyd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(mod.pn.iters) == 4


# ------------------------------------------------------------------------------------------------ guard bands, the C ABI
def _dev():
    return torch.device("cuda", 0)


def _gin(t, ld=None, name="input", skew=0):
    return Guarded.input(t.to(_dev()), ld=ld, name=name, skew=skew)


def _gout(shape, dtype=torch.float32, name="output", **kw):
    return Guarded(shape, dtype, _dev(), name=name, **kw)


def _p(g):
    return None if g is None else g.ptr


def _guarded_step(n, C, G, relu, residual, ldx, skew=None, expect_vec=None, short_ws=False):
    """mink_pn_fwd then mink_pn_bwd with every buffer a Guarded of exactly the documented size; x has NaN pad columns when
    ldx > C; `skew` names the one pointer put 4 bytes behind a 16-byte boundary."""
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    stream = torch.cuda.current_stream().cuda_stream
    sk = lambda name: 4 if skew == name else 0  # noqa: E731
    x, dy, res, w, b = _inputs(n, C, 21)
    st = _state(C, 1)
    gx = _gin(x, ld=ldx, name="x", skew=sk("x"))
    gres = _gin(res, name="residual") if residual else None
    gw, gb = _gin(w, name="weight", skew=sk("weight")), _gin(b, name="bias")
    gy = _gout((n, C), name="y", skew=sk("y"))
    grs, gvar, gsc = _gout((n, G), name="rscale"), _gout((C,), name="var"), _gout((C,), name="scale")
    gphi = _gout((C,), name="running_phi", init=st.running_phi.float())
    gema = _gout((C,), name="ema_gz", init=st.ema_gz.float())
    git = _gout((1,), torch.int64, name="iters", init=torch.tensor([st.iters]))
    need = L.mink_pn_workspace_bytes(n, C, G)
    assert need == max(1, min(-(-n // 256), 2048)) * 3 * C * 8 + 2 * C * 4
    vec = (C // G) % 4 == 0 and ldx % 4 == 0 and all(g is None or g.ptr % 16 == 0 for g in (gx, gy, gres))
    if expect_vec is not None:
        assert vec == expect_vec
    ws = Guarded(int(need), torch.uint8, _dev(), written="any", name="pn workspace")
    args = (gx.ptr, ldx, n, C, G, HP["eps"], HP["alpha_fwd"], HP["warmup_iters"], gw.ptr, gb.ptr, _p(gres), int(relu), gy.ptr, grs.ptr,
            gvar.ptr, gsc.ptr, gphi.ptr, git.ptr, ws.ptr)
    if short_ws:  # refused before any launch: nothing, the counter included, has moved
        assert L.mink_pn_fwd(*args, need - 1, stream) == -1 and b"workspace" in L.mink_last_error()
        torch.cuda.synchronize()
        for g in (gy, grs, gvar, gsc, gphi, git):
            g.set_written(False)
        check_all(gx, gres, gw, gb, gy, grs, gvar, gsc, gphi, git, ws)
        return
    check(L.mink_pn_fwd(*args, need, stream))
    torch.cuda.synchronize()
    check_all(gx, gres, gw, gb, gy, grs, gvar, gsc, gphi, git, ws)
    y = gy.logical().cpu()
    gdy, gyin = _gin(dy, name="dy", skew=sk("dy")), _gin(y, name="y (in)")
    grs_in, gvar_in, gsc_in = _gin(grs.logical().cpu(), name="rscale (in)"), _gin(gvar.logical().cpu(), name="var (in)"), _gin(gsc.logical().cpu(), name="scale (in)")
    gdx = _gout((n, C), name="dx", skew=sk("dx"))
    gdres = _gout((n, C), name="dresidual") if residual else None
    gdw, gdb = _gout((C,), name="dweight"), _gout((C,), name="dbias")
    ws2 = Guarded(int(need), torch.uint8, _dev(), written="any", name="pn workspace (bwd)")
    check(L.mink_pn_bwd(gdy.ptr, gx.ptr, ldx, gyin.ptr if relu else None, n, C, G, HP["eps"], HP["alpha_bkw"], 1, grs_in.ptr, gvar_in.ptr,
                        gsc_in.ptr, gw.ptr, int(relu), gema.ptr, gdx.ptr, _p(gdres), gdw.ptr, gdb.ptr, ws2.ptr, need, stream))
    torch.cuda.synchronize()
    check_all(gdy, gx, gyin, grs_in, gvar_in, gsc_in, gw, gema, gdx, gdres, gdw, gdb, ws2)
    got = dict(y=y, dx=gdx.logical().cpu(), dw=gdw.logical().cpu(), db=gdb.logical().cpu(), dres=gdres.logical().cpu() if residual else None,
               phi=gphi.logical().cpu(), ema=gema.logical().cpu(), iters=int(git.logical().cpu()))
    ref, bnd = _restate(x, dy, res, w, b, st, G, relu, residual, True, y)
    _hold(got, ref, bnd, True, residual, f"PN guarded n={n} C={C} G={G} ldx={ldx} skew={skew}")


@pytest.mark.parametrize("n,C,G,ldx,vec", [(300, 32, 4, 32, True), (300, 32, 4, 40, True), (300, 32, 4, 35, False), (257, 12, 3, 12, True), (257, 12, 2, 12, False),
                                           (65, 6, 3, 9, False), (1, 8, 1, 8, True), (513, 96, 96, 96, False), (700, 256, 2, 260, True)])
def test_guard_bands_exact_sizes_and_nan_pad_columns(n, C, G, ldx, vec):
    _guarded_step(n, C, G, True, True, ldx, expect_vec=vec)
    _guarded_step(n, C, G, False, False, ldx, expect_vec=vec)


@pytest.mark.parametrize("which", ["x", "y", "dy", "dx", "weight"])
def test_guard_bands_with_one_pointer_off_the_16_byte_boundary(which):
    """x / y move the forward to dword lanes, dy / dx the backward; the [C] vectors may sit anywhere (weight: lanes stay wide)."""
    _guarded_step(300, 32, 4, True, True, 32, skew=which, expect_vec=which not in ("x", "y"))


def test_undersized_workspace_is_refused_before_any_launch():
    _guarded_step(300, 32, 4, True, True, 32, short_ws=True)


# ------------------------------------------------------------------------------------------------ non-finite footprints
@pytest.mark.parametrize("C,G", [(12, 3), (32, 4)])
@pytest.mark.parametrize("poison", list(FP.POISONS))
def test_non_finite_footprints(C, G, poison):
    """One NaN / +inf / -inf in channel 0 of the poison rows of x or of dy, during warm-up (x: the row's group, then through the
    batch second moment every row of the group's channels, and running_phi there) and after it (running_phi scales: only the
    row's group; running_phi still takes it).  One channel, so that group 0 -- a third / a quarter of the channels -- is what
    the poison can reach and the footprint stays visible."""
    n, value = 130, FP.POISONS[poison]
    x, dy, res, w, b = _inputs(n, C, 31)
    rows = FP.poison_rows(n)
    res[rows, 0] = 10.0  # the poisoned positions pass the ReLU, so that a poisoned dy is not simply masked away
    for target in ("x", "dy"):
        for it0 in (0, 3):
            xp = FP.poison(x, value, rows, channels=[0]) if target == "x" else x
            dyp = FP.poison(dy, value, rows, channels=[0]) if target == "dy" else dy
            st = _state(C, it0)
            what = f"PN {poison} in {target} C={C} G={G} iters={it0}"
            got = _run(xp, dyp, res, w, b, st, G, True, True)
            ref, bnd = _restate(xp, dyp, res, w, b, st, G, True, True, True, got["y"])
            FP.visible({k: ref[k] for k in ("y", "dx", "dres")}, what)
            if target == "x":
                FP.visible_reduction({"running_phi": ref["phi"]}, what)
            for k in ("y", "dx", "dw", "db", "phi", "ema"):
                FP.same_footprint(got[k], ref[k], bnd[k], f"{what} {k}")
            FP.same_footprint(got["dres"], ref["dres"], None, what + " dresidual")


# ------------------------------------------------------------------------------------------------ networks
def _net(name, cin, ncls, seed=0):
    from nerf_downstream_amd.co3d_3d.src.models import get_model

    torch.manual_seed(seed)
    return get_model(name, cin, ncls).cuda()


def _train_steps(model, batches, labels, steps=3, lr=0.05):
    opt = torch.optim.SGD(model.parameters(), lr=lr)
    model.train()
    outs = []
    for s in range(steps):
        coords, feats = batches[s % len(batches)]
        opt.zero_grad(set_to_none=True)
        out = model(model.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
        loss = F.cross_entropy(out, labels[s % len(batches)].cuda())
        loss.backward()
        opt.step()
        outs.append((out.detach().clone(), loss.detach().clone(), out))
    return outs


@pytest.mark.parametrize("name", ["Res16UNet14", "ResNet14"])
def test_converted_networks_train_with_every_layer_within_its_bound(name):
    """Two batches of two tiny scenes (grids 16 and 24), three training steps of the converted network.  Hooks record every
    PowerNorm layer's input, flags, parameters and buffers before the call, and its output; each output (and running_phi) is
    held to the restatement on the recorded input.  The unconverted twin is run before and after the conversion of another
    instance: bit-identical, and it keeps the batch-norm paths (the native-trunk plan, the one-launch counter bump)."""
    from nerf_downstream_amd import minkowski as ME

    seg = name.startswith("Res16UNet")
    cin, ncls = 8, (6 if seg else 5)
    batches = [batch_scenes([71, 72], grid=16, cin=cin), batch_scenes([73, 74], grid=24, cin=cin)]
    g = torch.Generator().manual_seed(5)
    labels = [torch.randint(0, ncls, (c.shape[0] if seg else 2,), generator=g) for c, _ in batches]
    plain = [[(o, l) for o, l, _ in _train_steps(_net(name, cin, ncls), batches, labels)]]

    model = ME.MinkowskiPowerNorm.convert_powernorm(_net(name, cin, ncls))
    layers = {n: m for n, m in model.named_modules() if isinstance(m, ME.MinkowskiPowerNorm)}
    assert layers and not any(isinstance(m, ME.MinkowskiBatchNorm) for m in model.modules())
    names = {id(m): n for n, m in layers.items()}
    records = []

    def pre(mod, args, kwargs):
        res = kwargs.get("residual")
        mod._rec = dict(before=_module_state(mod), relu=bool(kwargs.get("relu", False)), x=args[0].F.detach().cpu(),
                        residual=None if res is None else res.F.detach().cpu(), w=mod.pn.weight.detach().cpu(), b=mod.pn.bias.detach().cpu())

    def post(mod, args, kwargs, out):
        rec = mod.__dict__.pop("_rec")
        rec.update(y=out.F.detach().cpu(), after=_module_state(mod), name=names[id(mod)], pn=mod.pn)
        records.append(rec)

    for m in layers.values():
        m.pn.warmup_iters = 2  # three steps then cross it < W, it == W and it > W
        m.register_forward_pre_hook(pre, with_kwargs=True)
        m.register_forward_hook(post, with_kwargs=True)
    outs = _train_steps(model, batches, labels)
    assert all(trunk_node(o) is None for _, _, o in outs) and not getattr(model, "_trunk_plan", None)  # module by module
    assert all(bool(torch.isfinite(l)) for _, l, _ in outs)
    assert len(records) == 3 * len(layers) and all(int(m.pn.iters) == 3 for m in layers.values())
    assert any(r["relu"] for r in records) and any(r["residual"] is not None for r in records)
    assert any(float(m.pn.ema_gz.abs().max()) > 0 for m in layers.values())
    worst = 0.0
    for r in records:
        pn = r["pn"]
        y, aux, after = PR.forward(r["x"], r["w"], r["b"], r["before"], PR.f32(pn.eps), PR.f32(pn.afwd), pn.warmup_iters, pn.group_num, True,
                                   r["residual"], r["relu"])
        ratio = float(((r["y"].double() - y).abs() / PR.forward_bound(aux, y)).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (r["name"], r["before"].iters, ratio)
        pb = PR.phi_bound(aux, r["before"], after, PR.f32(pn.afwd), pn.warmup_iters)
        assert bool(((r["after"].running_phi - after.running_phi).abs() <= pb).all()), (r["name"], "running_phi")
        assert r["after"].iters == r["before"].iters + 1
    print(f"\n[{name} converted] {len(records)} PowerNorm calls, worst forward error / bound {worst:.3f}")

    twin = _net(name, cin, ncls)
    plain.append([(o, l) for o, l, _ in _train_steps(twin, batches, labels)])
    for (o1, l1), (o2, l2) in zip(*plain):
        assert torch.equal(o1, o2) and torch.equal(l1, l2)
    if not seg:  # an unconverted ResNet14 still plans its native trunk and bumps its counters in one launch
        assert twin._trunk_plan and len(twin._norms) == len(layers)
        assert all(int(m.bn.num_batches_tracked) == 3 for m in twin._norms)


# ------------------------------------------------------------------------------------------------ train / evaluate
def test_train_and_evaluate_switches(tmp_path):
    """A three-step batch-norm checkpoint evaluated as PowerNorm (converted after loading), and a checkpoint trained with
    train.convert_powernorm=True (its keys carry .pn.running_phi: converted before loading) loaded back and evaluated."""
    from nerf_downstream_amd.co3d_3d.eval import evaluate
    from nerf_downstream_amd.co3d_3d.train import load_checkpoint_file, train

    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings(
            [f"{CFG}/co3d_cls.gin", f"{CFG}/synthetic_seg.gin", f"{CFG}/res16unet.gin"],
            ["train.gpus=1", "train.max_steps=3", "train.val_every_n_steps=3", "train.log_every_n_steps=1", "train.batch_size=2",
             "train.val_batch_size=2", "SparseVoxelSegDataset.grid=16", "SparseVoxelSegDataset.num_samples=8", "train.lr=0.01",
             "train.train_num_workers=0", "train.val_num_workers=0"],
        )
        train(save_path=str(tmp_path), resume_training=False, run_name="bn", run_name_postfix=None)
        bn_ckpt = str(tmp_path / "bn" / "last.ckpt")
        keys = list(load_checkpoint_file(bn_ckpt)["state_dict"])
        assert any(".bn.running_var" in k for k in keys) and not any(".pn." in k for k in keys)
        out = str(tmp_path / "eval")
        res = evaluate(save_path=out, load_path=bn_ckpt, tag="bn_as_pn", convert_powernorm=True)
        assert sorted(res) == ["val/OA", "val/loss", "val/mAcc", "val/mIoU"] and res["val/loss"] == res["val/loss"]
        assert json.load(open(os.path.join(out, "bn_as_pn.json"))) == res
        plain = evaluate(save_path=out, load_path=bn_ckpt, tag="bn")
        assert plain != res  # PowerNorm subtracts no mean: the same weights score differently

        train(save_path=str(tmp_path), resume_training=False, run_name="pn", run_name_postfix=None, convert_powernorm=True)
        pn_ckpt = str(tmp_path / "pn" / "last.ckpt")
        sd = load_checkpoint_file(pn_ckpt)["state_dict"]
        assert any(".pn.running_phi" in k for k in sd) and not any(".bn." in k for k in sd)
        assert all(int(v) == 3 for k, v in sd.items() if k.endswith(".pn.iters"))
        assert any(float(v.abs().max()) > 0 for k, v in sd.items() if k.endswith(".pn.ema_gz"))
        res2 = evaluate(save_path=out, load_path=pn_ckpt, tag="pn", convert_powernorm=True)
        assert json.load(open(os.path.join(out, "pn.json"))) == res2 and res2["val/loss"] == res2["val/loss"]
        with pytest.raises(RuntimeError, match="pn.running_phi|Unexpected|Missing"):  # a PN checkpoint does not fit batch norms
            evaluate(save_path=out, load_path=pn_ckpt, tag="pn_unconverted")
    finally:
        gin.clear_config()
