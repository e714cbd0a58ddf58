"""-m gpu: mink_posenc_fwd / mink_posenc_bwd inside guard bands (tests/guarded.py), by the rules of
tests/test_gpu_guard_rowpass.py: the C ABI directly, every output a Guarded of exactly the size include/mink_hip.h names, every
input a Guarded.input with NaN bands and NaN pad columns.  After the call: check() on every buffer (bands untouched, every
column of the row written, pad columns right of them and every input bit for bit as before), then the values within the
derived bounds of tests/posenc_restate.py.  The lane form is restated from the host code: 16 bytes iff 2L % 4 == 0, ldy % 4 == 0
and y (dy), freq and phase are 16-byte aligned; dwords otherwise -- through 27 columns, through a pitch, or through a
pointer that Guarded(skew=4) puts 4 bytes behind a 16-byte boundary.  Nothing here is meant to fault."""
import pytest
import torch

import posenc_restate as R
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu

# (C, L, range, ldx - C, ldy - columns, skew of y / dy, skew of freq) -> the lanes the host picks
CASES = [
    (28, 4, None, 0, 0, 0, 0, 4),       # exact size, 16-byte lanes
    (28, 4, None, 4, 8, 0, 0, 4),       # NaN pad columns on both sides, still 16-byte lanes
    (4, 2, (1, 3), 0, 2, 0, 0, 4),      # 18 columns in a pitch of 20
    (3, 4, (0, 3), 0, 0, 0, 0, 1),      # 27 columns: dwords
    (3, 4, (0, 3), 1, 5, 0, 0, 4),      # 27 columns in a pitch of 32: 2L = 8, aligned -- 16-byte lanes again
    (28, 4, None, 0, 0, 4, 0, 1),       # the output 4 bytes behind a 16-byte boundary
    (28, 4, None, 0, 0, 0, 4, 1),       # the frequencies 4 bytes behind one
    (5, 3, (1, 2), 0, 3, 0, 0, 1),      # 2L = 6
    (1, 1, None, 0, 0, 0, 0, 1),
]
N = 300  # two workgroups of row-channel lanes at C = 3, more above


def _dev():
    return torch.device("cuda", 0)


def _vec(L, ldy, *bufs):
    return (2 * L) % 4 == 0 and ldy % 4 == 0 and all(g.ptr % 16 == 0 for g in bufs)


@pytest.mark.parametrize("C,L,rng,padx,pady,skew_y,skew_f,lanes", CASES)
def test_posenc_inside_guard_bands(C, L, rng, padx, pady, skew_y, skew_f, lanes):
    from nerf_downstream_amd._lib import check, lib

    lo, hi = rng or (0, 0)
    Q, W = 2 * L * C, 2 * L * C + hi - lo
    ldx, ldy = C + padx, W + pady
    chan, freq64, phase64 = R.columns(C, L)
    freq, phase = freq64.float(), phase64.float()
    consts = (chan, freq.double(), phase.double())
    x = R.inputs(N, C, seed=C + L)
    dy = torch.randn(N, W, generator=torch.Generator().manual_seed(9))
    gx = Guarded.input(x.to(_dev()), ld=ldx, name="x")
    gf = Guarded.input(freq.to(_dev()), name="freq", skew=skew_f)
    gp = Guarded.input(phase.to(_dev()), name="phase")
    gy = Guarded((N, ldy), torch.float32, _dev(), cols=W, name="y", skew=skew_y)
    gdy = Guarded.input(dy.to(_dev()), ld=ldy, name="dy", skew=skew_y)
    gdx = Guarded((N, ldx), torch.float32, _dev(), cols=C, name="dx")
    assert (4 if _vec(L, ldy, gy, gf, gp) else 1) == lanes and (4 if _vec(L, ldy, gdy, gf, gp) else 1) == lanes
    st = torch.cuda.current_stream().cuda_stream
    check(lib().mink_posenc_fwd(gx.ptr, N, C, ldx, gf.ptr, gp.ptr, L, lo, hi, gy.ptr, ldy, st))
    check(lib().mink_posenc_bwd(gdy.ptr, ldy, gx.ptr, N, C, ldx, gf.ptr, gp.ptr, L, lo, hi, gdx.ptr, ldx, st))
    torch.cuda.synchronize()
    check_all(gx, gf, gp, gy, gdy, gdx)
    y, dx = gy.logical().cpu(), gdx.logical().cpu()
    assert_finite(y, "y"), assert_finite(dx, "dx")
    ref = R.forward(x, *consts, rng)
    assert bool(((y[:, :Q].double() - ref[:, :Q]).abs() <= R.forward_bound(x, *consts)).all())
    assert torch.equal(y[:, Q:], x[:, lo:hi])
    rdx = R.backward(x, dy, *consts, rng)
    assert bool(((dx.double() - rdx).abs() <= R.backward_bound(x, dy, *consts, rdx)).all())
