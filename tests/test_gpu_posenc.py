"""-m gpu: mink_posenc_fwd / mink_posenc_bwd (csrc/posenc.hip) against the float64 restatement of tests/posenc_restate.py.

Bounds, derived (posenc_restate.forward_bound / backward_bound): with a = f x + phase evaluated in float64 from the fp32 inputs and
the layer's fp32 constants,
    |y - sin(a)| <= (|a| + 4) 2^-23                                    -- one fp32 rounding of the argument, a few ulps of a sine
    |dx - ref|   <= 2^-22 sum_q f_q |dy_q| (|a_q| + 4) + 4 ulps of |ref|
and the pass-through columns are bit-equal to x (their dy is added exactly once)."""
import pytest
import torch

import posenc_restate as R
from helpers import batch_scenes

pytestmark = pytest.mark.gpu

SIZES = (0, 1, 63, 64, 65, 1000)
CASES = [(1, 1, None, None), (3, 4, None, None), (3, 6, (0, 3), None), (5, 3, (1, 2), None), (28, 4, None, None), (3, 6, None, 0.01)]
IDS = ["C1L1", "C3L4", "C3L6+0:3", "C5L3+1:2", "C28L4", "C3L6res0.01"]


def _module(C, L, rng, res):
    from nerf_downstream_amd import minkowski as ME

    return ME.MinkowskiPositionalEncoding(C, num_encoding_functions=L, include_original_channel_range=rng, min_resolution=res).cuda()


def _constants(mod):
    """(chan, freq, phase) of the restatement with the MODULE's fp32 values: what the kernel reads."""
    return mod.coo[0].cpu(), mod.frequencies.detach().cpu().double(), mod.offset.detach().cpu().view(-1).double()


def _run(mod, x, dy):
    from nerf_downstream_amd.minkowski import functional as Fn

    lo, hi = mod.include_original_channel_range or (0, 0)
    xd = x.cuda().requires_grad_(True)
    y = Fn.PositionalEncodingFunction.apply(xd, mod.frequencies, mod.offset.view(-1), mod.num_encoding_functions, lo, hi)
    y.backward(dy.cuda())
    return y.detach().cpu(), xd.grad.cpu()


def _check(y, dx, x, dy, consts, rng, what):
    chan, freq, phase = consts
    Q = chan.numel()
    ref = R.forward(x, chan, freq, phase, rng)
    assert y.shape == ref.shape and y.dtype == torch.float32, what
    err, bound = (y[:, :Q].double() - ref[:, :Q]).abs(), R.forward_bound(x, chan, freq, phase)
    print(f"[{what}] forward: max |err| {float(err.max()) if err.numel() else 0:.2e}, max err / bound "
          f"{float((err / bound).max()) if err.numel() else 0:.3f}")
    assert bool((err <= bound).all()), (what, float((err - bound).max()))
    lo, hi = rng or (0, 0)
    assert torch.equal(y[:, Q:], x[:, lo:hi]), what  # bit-equal
    rdx = R.backward(x, dy, chan, freq, phase, rng)
    derr, dbound = (dx.double() - rdx).abs(), R.backward_bound(x, dy, chan, freq, phase, rdx)
    print(f"[{what}] backward: max |err| {float(derr.max()) if derr.numel() else 0:.2e}, max err / bound "
          f"{float((derr / dbound.clamp_min(1e-300)).max()) if derr.numel() else 0:.3f}")
    assert dx.shape == x.shape and bool((derr <= dbound).all()), (what, float((derr - dbound).max()))


@pytest.mark.parametrize("C,L,rng,res", CASES, ids=IDS)
def test_operator_matches_restatement(C, L, rng, res):
    mod = _module(C, L, rng, res)
    consts = _constants(mod)
    for n in SIZES:
        x = R.inputs(n, C, seed=n + C)
        dy = torch.randn(n, mod.out_channels, generator=torch.Generator().manual_seed(n + 7))
        y, dx = _run(mod, x, dy)
        _check(y, dx, x, dy, consts, rng, f"C={C} L={L} range={rng} res={res} n={n}")
        if n == 1000:  # two runs are bitwise equal
            y2, dx2 = _run(mod, x, dy)
            assert torch.equal(y, y2) and torch.equal(dx, dx2)


def _abi(mod, x, y, ldy, dy=None, dx=None):
    """The C ABI on raw device pointers (x contiguous [n, C]); dy given -> backward into dx."""
    from nerf_downstream_amd._lib import check, lib

    n, C = x.shape
    lo, hi = mod.include_original_channel_range or (0, 0)
    st = torch.cuda.current_stream().cuda_stream
    f, p, L = mod.frequencies.data_ptr(), mod.offset.data_ptr(), mod.num_encoding_functions
    if dy is None:
        check(lib().mink_posenc_fwd(x.data_ptr(), n, C, C, f, p, L, lo, hi, y.data_ptr(), ldy, st))
    else:
        check(lib().mink_posenc_bwd(dy.data_ptr(), ldy, x.data_ptr(), n, C, C, f, p, L, lo, hi, dx.data_ptr(), C, st))


@pytest.mark.parametrize("C,L,rng", [(4, 4, None), (3, 4, (0, 3)), (28, 4, (3, 7))], ids=["off-by-4-bytes", "27-columns", "C28+pad"])
def test_dword_lanes_and_row_pitch(C, L, rng):
    """The dword form (a base pointer 4 bytes behind a 16-byte boundary; 27 columns) gives bit for bit what the 16-byte form
    gives, and with ldy wider than the row nothing to the right of the written columns changes."""
    mod = _module(C, L, rng, None)
    consts = _constants(mod)
    n, W = 333, mod.out_channels
    x = R.inputs(n, C, seed=5)
    dy = torch.randn(n, W, generator=torch.Generator().manual_seed(6))
    y0, dx0 = _run(mod, x, dy)  # contiguous, pitch W: 16-byte lanes when W % 4 == 0
    _check(y0, dx0, x, dy, consts, rng, f"C={C} L={L} range={rng} contiguous")
    xd = x.cuda()
    for ldy, skew in ((W, 1), (W + 5, 0), (W + 8 - W % 4, 0), (W + 8 - W % 4, 1)):
        flat = torch.full((n * ldy + 4,), -7.0, device="cuda")
        y = flat[skew: skew + n * ldy].view(n, ldy)
        assert y.data_ptr() % 16 == 4 * skew
        _abi(mod, xd, y, ldy)
        assert torch.equal(y[:, :W].cpu(), y0), (ldy, skew)
        assert bool((y[:, W:] == -7.0).all()) and bool((flat[:skew] == -7.0).all()) and bool((flat[skew + n * ldy:] == -7.0).all())
        gflat = torch.full((n * ldy + 4,), float("nan"), device="cuda")  # NaN pad columns: a read of one would show in dx
        g = gflat[skew: skew + n * ldy].view(n, ldy)
        g[:, :W] = dy.cuda()
        dx = torch.empty(n, C, device="cuda")
        _abi(mod, xd, None, ldy, dy=g, dx=dx)
        assert torch.equal(dx.cpu(), dx0), (ldy, skew)


def test_module_kinds_and_no_host_synchronisation():
    from nerf_downstream_amd import minkowski as ME

    coords, feats = batch_scenes([3, 4], grid=16, cin=3)
    coords = coords.clone()
    coords[:, 1:] += 0.25
    mod = _module(3, 4, (0, 3), None)
    field = ME.TensorField(coordinates=coords.cuda(), features=feats.cuda().requires_grad_(True))
    sp = field.sparse()
    dyd = torch.randn(coords.shape[0], mod.out_channels).cuda()
    mod(field)  # (settles the field)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out_f = mod(field)
        out_f.F.backward(dyd)
        out_s = mod(sp)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert isinstance(out_f, ME.TensorField) and out_f.coordinate_manager is field.coordinate_manager and out_f.C is field.C
    assert isinstance(out_s, ME.SparseTensor) and out_s.coordinate_manager is sp.coordinate_manager
    assert out_s.coordinate_map_key == sp.coordinate_map_key and out_s.F.shape == (sp.F.shape[0], 27)
    consts = _constants(mod)
    _check(out_f.F.detach().cpu(), field.F.grad.cpu(), feats, dyd.cpu(), consts, (0, 3), "module on a field")
    assert out_f.sparse().F.shape == (sp.F.shape[0], 27)  # the encoded field quantises on the same manager
    ident = ME.MinkowskiPositionalEncoding(3, 0)
    assert ident(field) is field and ident(sp) is sp
    # a loaded checkpoint's constants rule
    sd = {k: v.clone() for k, v in mod.state_dict().items()}
    sd["frequencies"] *= 0.5
    sd["offset"] += 0.125
    mod.load_state_dict(sd)
    y = mod(sp).F.detach().cpu()
    ref = R.forward(sp.F.detach().cpu(), *_constants(mod), (0, 3))
    assert float((y.double() - ref).abs().max()) <= 1e-5 and float((y[:, :24] - out_s.F.detach().cpu()[:, :24]).abs().max()) > 0.1
