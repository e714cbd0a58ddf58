"""-m gpu: mink_generate_children, mink_prune_compact, mink_prune_gather and mink_prune_gather_bwd inside guard bands
(tests/guarded.py), by the rules of tests/test_gpu_guard_rowpass.py: the C ABI directly, every output and workspace a Guarded of
exactly the size include/mink_hip.h names, every input a Guarded.input with NaN bands and NaN pad columns.  After the call:
check() on every buffer, then the values against tests/gen_restate.py.  The lane form of the row passes is restated from the host
code: 16 bytes iff C % 4 == 0, both pitches % 4 == 0 and both matrices 16-byte aligned; dwords otherwise -- through an odd
width, an odd pitch, or a pointer that Guarded(skew=4) puts 4 bytes behind a 16-byte boundary.  Nothing here is meant to fault."""
import numpy as np
import pytest
import torch

import gen_restate as R
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


@pytest.mark.parametrize("n,ts", [(1, 2), (65, 4)])
def test_children_inside_guard_bands(n, ts):
    from nerf_downstream_amd._lib import check, lib

    parents = R.random_parents(np.random.default_rng(n), n, ts, 2, top=True)
    gp = Guarded.input(torch.from_numpy(parents).to(_dev()), name="parents")
    gc = Guarded((8 * n, 4), torch.int32, _dev(), name="children")
    check(lib().mink_generate_children(gp.ptr, n, ts, gc.ptr, _stream()))
    torch.cuda.synchronize()
    check_all(gp, gc)
    assert torch.equal(gc.t.cpu(), torch.from_numpy(R.children(parents, ts)))


@pytest.mark.parametrize("n", [1, 257])
def test_prune_compact_inside_guard_bands(n):
    from nerf_downstream_amd._lib import check, lib

    L, B = lib(), 3
    coords = R.random_parents(np.random.default_rng(n), n, 2, B)
    mask = np.ones(n, bool) if n == 1 else (coords[:, 0] != 1) & (np.arange(n) % 3 != 0)  # the middle sample goes entirely
    _, want_c, want_off, want_kept, want_o2n = R.prune(torch.zeros(n, 1), coords, mask, B)
    k = int(mask.sum())
    first = torch.arange(n) < k
    gm = Guarded.input(torch.from_numpy(mask.astype(np.uint8)).to(_dev()), name="mask")
    gc = Guarded.input(torch.from_numpy(coords).to(_dev()), name="coords")
    gkept = Guarded((n,), torch.int32, _dev(), written=first, name="kept")
    go2n = Guarded((n,), torch.int32, _dev(), name="old2new")
    gout = Guarded((n, 4), torch.int32, _dev(), written=first[:, None].expand(n, 4), name="out_coords")
    goff = Guarded((B + 1,), torch.int32, _dev(), name="batch_offsets")
    gtot = Guarded((1,), torch.int32, _dev(), name="total")
    gws = Guarded(int(L.mink_prune_workspace_bytes(n)), torch.uint8, _dev(), written="any", name="workspace")
    check(L.mink_prune_compact(gm.ptr, gc.ptr, n, B, gkept.ptr, go2n.ptr, gout.ptr, goff.ptr, gtot.ptr, gws.ptr, gws.nbytes, _stream()))
    torch.cuda.synchronize()
    check_all(gm, gc, gkept, go2n, gout, goff, gtot, gws)
    assert int(gtot.t.item()) == k
    assert gkept.t[:k].cpu().tolist() == want_kept.tolist() and go2n.t.cpu().tolist() == want_o2n.tolist()
    assert torch.equal(gout.t[:k].cpu(), torch.from_numpy(want_c)) and goff.t.cpu().tolist() == want_off.tolist()


# (C, source pad columns, destination pad columns, skew of the destination) -> the lanes the host picks
ROW_CASES = [
    (4, 0, 0, 0, 4),    # exact size, 16-byte lanes
    (32, 4, 8, 0, 4),   # NaN pad columns on both sides, still 16-byte lanes
    (4, 1, 0, 0, 1),    # a pitch of 5
    (3, 0, 0, 0, 1),
    (1, 0, 0, 0, 1),
    (4, 0, 0, 4, 1),    # the destination 4 bytes behind a 16-byte boundary
]


@pytest.mark.parametrize("C,pads,padd,skew,lanes", ROW_CASES)
def test_prune_row_passes_inside_guard_bands(C, pads, padd, skew, lanes):
    from nerf_downstream_amd._lib import check, lib

    L, n = lib(), 65
    mask = np.arange(n) % 3 != 1
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(n, C, generator=gen)
    want, _, _, kept, o2n = R.prune(x, np.zeros((n, 4), np.int32), mask, 1)
    k = kept.shape[0]
    g = torch.randn(k, C, generator=gen)
    gkept = Guarded.input(torch.from_numpy(kept).to(_dev()), name="kept")
    go2n = Guarded.input(torch.from_numpy(o2n).to(_dev()), name="old2new")

    def vec(src, dst, lds, ldd):
        return C % 4 == 0 and lds % 4 == 0 and ldd % 4 == 0 and src.ptr % 16 == 0 and dst.ptr % 16 == 0

    # forward: y = x[kept]
    gx = Guarded.input(x.to(_dev()), ld=C + pads, name="x")
    gy = Guarded((k, C + padd), torch.float32, _dev(), cols=C, name="y", skew=skew)
    assert (4 if vec(gx, gy, C + pads, C + padd) else 1) == lanes
    check(L.mink_prune_gather(gx.ptr, C + pads, n, C, gkept.ptr, k, gy.ptr, C + padd, _stream()))
    # backward: dx = dy[old2new], zeros for a pruned row
    gdy = Guarded.input(g.to(_dev()), ld=C + pads, name="dy")
    gdx = Guarded((n, C + padd), torch.float32, _dev(), cols=C, name="dx", skew=skew)
    assert (4 if vec(gdy, gdx, C + pads, C + padd) else 1) == lanes
    check(L.mink_prune_gather_bwd(gdy.ptr, C + pads, k, C, go2n.ptr, n, gdx.ptr, C + padd, _stream()))
    torch.cuda.synchronize()
    check_all(gkept, go2n, gx, gy, gdy, gdx)
    y, dx = gy.logical().cpu(), gdx.logical().cpu()
    assert_finite(y, "y"), assert_finite(dx, "dx")
    assert torch.equal(y, want) and torch.equal(dx, R.prune_grad(g, mask))
