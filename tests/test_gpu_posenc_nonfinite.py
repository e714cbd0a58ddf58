"""-m gpu: non-finite footprints of the positional encoding (tests/footprint.py).  One NaN, +inf or -inf in x or in dy comes
out exactly where the float64 restatement has a non-finite value -- the channel's own 2L columns (sin and cos of an infinity
are NaN) and its pass-through column, which keeps the value itself -- and nowhere else: not in another channel's columns, not in
another row.  Finite elements keep the derived bounds of tests/posenc_restate.py."""
import pytest
import torch

import footprint as FP
import posenc_restate as R

pytestmark = pytest.mark.gpu

CASES = [(3, 4, (0, 3)), (28, 4, None), (5, 3, (1, 2))]  # dword lanes with pass-through, 16-byte lanes, 2L = 6
N = 130


def _run(C, L, rng, x, dy):
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.minkowski import functional as Fn

    mod = ME.MinkowskiPositionalEncoding(C, num_encoding_functions=L, include_original_channel_range=rng).cuda()
    lo, hi = rng or (0, 0)
    xd = x.cuda().requires_grad_(True)
    y = Fn.PositionalEncodingFunction.apply(xd, mod.frequencies, mod.offset.view(-1), L, lo, hi)
    y.backward(dy.cuda())
    consts = (mod.coo[0].cpu(), mod.frequencies.detach().cpu().double(), mod.offset.detach().cpu().view(-1).double())
    return y.detach().cpu(), xd.grad.cpu(), consts


@pytest.mark.parametrize("poison", list(FP.POISONS))
@pytest.mark.parametrize("C,L,rng", CASES, ids=["C3L4+0:3", "C28L4", "C5L3+1:2"])
def test_footprint_of_a_poisoned_input(C, L, rng, poison):
    lo, hi = rng or (0, 0)
    Q = 2 * L * C
    x = R.inputs(N, C, seed=C, big_column=False)
    dy = torch.randn(N, Q + hi - lo, generator=torch.Generator().manual_seed(1))
    rows, ch = FP.poison_rows(N), FP.poison_channels(C)
    xp = FP.poison(x, FP.POISONS[poison], rows, ch)
    y, dx, consts = _run(C, L, rng, xp, dy)
    ref, rdx = R.forward(xp, *consts, rng), R.backward(xp, dy, *consts, rng)
    FP.visible({"y": ref, "dx": rdx}, f"x {poison}")
    want = torch.zeros(N, Q + hi - lo, dtype=torch.bool)  # the footprint, written out: the channel's 2L columns and its pass-through
    for r in rows:
        for c in ch:
            want[r, 2 * L * c: 2 * L * (c + 1)] = True
            if lo <= c < hi:
                want[r, Q + c - lo] = True
    assert torch.equal(FP.footprint(ref), want)
    bound = torch.cat([R.forward_bound(x, *consts), torch.zeros(N, hi - lo, dtype=torch.float64)], dim=1)
    FP.same_footprint(y, ref, bound, f"y, x {poison}")
    assert torch.equal(y[:, Q:], xp[:, lo:hi]) or FP.is_nan(FP.POISONS[poison])  # an infinity passes through as itself
    FP.same_footprint(dx, rdx, R.backward_bound(x, dy, *consts, R.backward(x, dy, *consts, rng)), f"dx, x {poison}")
    clean_y, clean_dx, _ = _run(C, L, rng, x, dy)
    FP.untouched(y, clean_y, ~want, f"y, x {poison}")
    FP.untouched(dx, clean_dx, torch.isfinite(xp), f"dx, x {poison}")


@pytest.mark.parametrize("poison", list(FP.POISONS))
@pytest.mark.parametrize("C,L,rng", CASES, ids=["C3L4+0:3", "C28L4", "C5L3+1:2"])
def test_footprint_of_a_poisoned_gradient(C, L, rng, poison):
    lo, hi = rng or (0, 0)
    Q, W = 2 * L * C, 2 * L * C + hi - lo
    x = R.inputs(N, C, seed=C + 1, big_column=False)
    dy = torch.randn(N, W, generator=torch.Generator().manual_seed(2))
    rows = FP.poison_rows(N)
    cols = sorted({0, 2 * L - 1, Q - 1, W - 1})  # first and last column of a channel, the last encoded one, the last of the row
    dyp = FP.poison(dy, FP.POISONS[poison], rows, cols)
    y, dx, consts = _run(C, L, rng, x, dyp)
    rdx = R.backward(x, dyp, *consts, rng)
    FP.visible({"dx": rdx}, f"dy {poison}")
    want = torch.zeros(N, C, dtype=torch.bool)
    for r in rows:
        for q in cols:
            want[r, q // (2 * L) if q < Q else lo + q - Q] = True
    assert torch.equal(FP.footprint(rdx), want)
    clean = R.backward(x, dy, *consts, rng)
    # a reference infinity is f cos(a) inf: its sign is that of the cosine, which the fp32 argument shares away from a zero of it
    FP.same_footprint(dx, rdx, R.backward_bound(x, dy, *consts, clean), f"dx, dy {poison}")
    clean_y, clean_dx, _ = _run(C, L, rng, x, dy)
    assert torch.equal(y, clean_y)  # the forward does not see dy
    FP.untouched(dx, clean_dx, ~want, f"dx, dy {poison}")
