"""-m gpu: mink_knn_cross inside guard bands (tests/guarded.py), called through the C ABI with idx and dist of exactly
nq x k elements, both inputs at a leading dimension beyond C with NaN pad columns, and both offset arrays guarded: the bands are
untouched, every idx and dist element is written, the inputs are unchanged, and no pad column reaches a result.  Nothing here
is meant to fault: no buffer is smaller than the header asks for."""
import pytest
import torch

import match_restate as MR
from guarded import Guarded, check_all

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("k", [1, 64])
@pytest.mark.parametrize("C", [3, 33])
def test_knn_cross_stays_inside_its_buffers(C, k):
    from nerf_downstream_amd._lib import check, lib

    L, dev = lib(), torch.device("cuda", 0)
    q_off, c_off = MR.offsets(k)
    g = torch.Generator().manual_seed(10 * C + k)
    q = torch.randint(-8, 9, (q_off[-1], C), generator=g).float()  # (integers: the table and the distances are exact)
    c = torch.randint(-8, 9, (c_off[-1], C), generator=g).float()
    ldq, ldc = C + 5, C + 2
    gq, gc = Guarded.input(q.to(dev), ld=ldq, name="q"), Guarded.input(c.to(dev), ld=ldc, name="c")
    gqo = Guarded.input(torch.tensor(q_off, dtype=torch.int32, device=dev), name="q_offsets")
    gco = Guarded.input(torch.tensor(c_off, dtype=torch.int32, device=dev), name="c_offsets")
    gidx = Guarded((q_off[-1], k), torch.int32, dev, name="idx")
    gdist = Guarded((q_off[-1], k), torch.float32, dev, name="dist")
    check(L.mink_knn_cross(gq.ptr, q_off[-1], ldq, gc.ptr, c_off[-1], ldc, C, gqo.ptr, gco.ptr, len(q_off) - 1, k, gidx.ptr, gdist.ptr,
                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check_all(gq, gc, gqo, gco, gidx, gdist)
    ref, refd = MR.knn_cross(q, c, q_off, c_off, k)
    got, gd = gidx.t.cpu().long(), gdist.t.cpu().double()
    assert torch.equal(got, ref)
    assert not bool(torch.isnan(gd).any()) and torch.equal(gd, refd)  # a pad column read would have made a distance NaN
    # dist = NULL: the same table, and nothing else written
    gidx2 = Guarded((q_off[-1], k), torch.int32, dev, name="idx (no dist)")
    check(L.mink_knn_cross(gq.ptr, q_off[-1], ldq, gc.ptr, c_off[-1], ldc, C, gqo.ptr, gco.ptr, len(q_off) - 1, k, gidx2.ptr, None,
                           torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check_all(gq, gc, gqo, gco, gidx2)
    assert torch.equal(gidx2.t, gidx.t)
