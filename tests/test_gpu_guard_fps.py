"""-m gpu: mink_fps_scenes inside guard bands (tests/guarded.py), called through the C ABI with idx of exactly B x m words, a
workspace of exactly mink_fps_workspace_bytes, the coordinates at ld = 4 with NaN in the fourth column and their pointer 4 bytes
off a 16-byte boundary, at one scene size per residency: the bands are untouched, every idx element and the status word are
written, the inputs are unchanged, and the picks are the restatement's (a NaN read into a distance would change them).
Nothing here is meant to fault: no buffer is smaller than the header asks for."""
import numpy as np
import pytest
import torch

import fps_restate as FR
from guarded import Guarded, check_all

pytestmark = pytest.mark.gpu


def _sizes(with_workspace):
    from nerf_downstream_amd import _lib

    small, xyz_reg, dist_reg = _lib.FPS_XYZ_REG_ROWS_SMALL, _lib.FPS_XYZ_REG_ROWS, _lib.FPS_DIST_REG_ROWS
    sizes = [small - 47, xyz_reg - 1191, dist_reg - 20343]  # neither a multiple of the workgroup nor of the wave
    return sizes + [dist_reg + 1657] if with_workspace else sizes


@pytest.mark.parametrize("with_workspace", [True, False])
@pytest.mark.parametrize("skew", [0, 4])
def test_fps_stays_inside_its_buffers(with_workspace, skew):
    from nerf_downstream_amd._lib import check, lib

    L, dev = lib(), torch.device("cuda", 0)
    sizes = _sizes(with_workspace)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n, B, m = int(off[-1]), len(sizes), 8
    g = torch.Generator().manual_seed(B + skew)
    xyz = torch.randint(0, 128, (n, 3), generator=g).float()
    start = [n_b - 1 - b for b, n_b in enumerate(sizes)]
    gx = Guarded.input(xyz.to(dev), ld=4, name="xyz", skew=skew)  # (pad column and bands: NaN)
    assert gx.ptr % 16 == skew
    go = Guarded.input(torch.tensor(off, dtype=torch.int32, device=dev), name="offsets")
    gs = Guarded.input(torch.tensor(start, dtype=torch.int32, device=dev), name="start")
    gidx = Guarded((B, m), torch.int32, dev, name="idx")
    gstatus = Guarded((1,), torch.int32, dev, name="status")
    n_max = max(sizes)
    need = L.mink_fps_workspace_bytes(n_max, B)
    assert (need == B * n_max * 4) if with_workspace else need == 0
    gws = Guarded(need, torch.uint8, dev, written="any", name="workspace") if need else None
    check(L.mink_fps_scenes(gx.ptr, n, 4, go.ptr, gs.ptr, B, m, n_max, gidx.ptr, gstatus.ptr, gws.ptr if gws else None, need,
                            torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check_all(gx, go, gs, gidx, gstatus, gws)
    assert int(gstatus.t[0]) == 0
    assert np.array_equal(gidx.t.cpu().numpy().astype(np.int64), FR.fps_batch(xyz.numpy(), off, m, start))
