"""-m gpu: mink_union_build and mink_union_sum inside guard bands (tests/guarded.py), by the rules of
tests/test_gpu_guard_generative.py: the C ABI directly, every output and the workspace a Guarded of exactly the size
include/mink_hip.h names, every input a Guarded.input with NaN (or sentinel) bands and NaN pad columns.  After the call: check()
on every buffer -- rows of out_coords and entries of out2in past *total must still hold the sentinel -- then the values against
tests/union_restate.py.  The lane form of the sum is restated from the host code: 16 bytes iff C % 4 == 0, every pitch % 4 == 0 and
every matrix 16-byte aligned; dwords otherwise -- through an odd width, an odd pitch, or ONE input that Guarded(skew=4) puts
4 bytes behind a 16-byte boundary.  Nothing here is meant to fault."""
import ctypes

import numpy as np
import pytest
import torch

import union_restate as U
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _pointers(bufs):
    return (ctypes.c_void_p * len(bufs))(*[b.ptr for b in bufs])


@pytest.mark.parametrize("relation,n,k", [("disjoint", 1, 2), ("partial", 257, 3), ("emptied", 256, 8), ("twice", 255, 2)])
def test_union_build_inside_guard_bands(relation, n, k):
    from nerf_downstream_amd._lib import check, lib

    L, B, ts = lib(), 3, 2
    lists = U.related_lists(np.random.default_rng(n), relation, n, k, B, ts, edges=True)
    want_c, want_i2o, want_o2i, want_off = U.union_map(lists, B)
    N, S = want_c.shape[0], sum(c.shape[0] for c in lists)
    assert N < S or relation == "disjoint"  # rows past the count exist: they must keep the sentinel
    counts = (ctypes.c_int64 * k)(*[c.shape[0] for c in lists])
    gcoords = [Guarded.input(torch.from_numpy(c).to(_dev()), name=f"coords {i}") for i, c in enumerate(lists)]
    goffs = [Guarded.input(torch.from_numpy(U.R.batch_offsets(c, B)).to(_dev()), name=f"offsets {i}") for i, c in enumerate(lists)]
    first = torch.arange(S) < N
    gout = Guarded((S, 4), torch.int32, _dev(), written=first[:, None].expand(S, 4), name="out_coords")
    gi2o = [Guarded((c.shape[0],), torch.int32, _dev(), name=f"in2out {i}") for i, c in enumerate(lists)]
    go2i = Guarded((k, S), torch.int32, _dev(), written=first[None, :].expand(k, S), name="out2in")
    goff = Guarded((B + 1,), torch.int32, _dev(), name="batch_offsets")
    gtot = Guarded((1,), torch.int32, _dev(), name="total")
    need = int(L.mink_union_workspace_bytes(k, counts, B))
    gws = Guarded(need, torch.uint8, _dev(), written="any", name="workspace")
    check(L.mink_union_build(k, _pointers(gcoords), _pointers(goffs), counts, B, gout.ptr, _pointers(gi2o), go2i.ptr, S, goff.ptr, gtot.ptr,
                             gws.ptr, gws.nbytes, _stream()))
    torch.cuda.synchronize()
    check_all(*gcoords, *goffs, gout, *gi2o, go2i, goff, gtot, gws)
    assert int(gtot.t.item()) == N
    assert torch.equal(gout.t[:N].cpu(), torch.from_numpy(want_c)) and goff.t.cpu().tolist() == want_off.tolist()
    assert all(g.t.cpu().tolist() == w.tolist() for g, w in zip(gi2o, want_i2o))
    assert torch.equal(go2i.t[:, :N].cpu(), torch.from_numpy(want_o2i))


# (C, pad columns of the inputs, pad columns of y, skew of input 1) -> the lanes the host picks
ROW_CASES = [
    (4, 0, 0, 0, 4),    # exact size, 16-byte lanes
    (32, 4, 8, 0, 4),   # NaN pad columns on every matrix, still 16-byte lanes
    (36, 0, 4, 0, 4),
    (4, 1, 0, 0, 1),    # a pitch of 5
    (3, 0, 0, 0, 1),
    (1, 2, 1, 0, 1),
    (4, 0, 0, 4, 1),    # ONE input 4 bytes behind a 16-byte boundary
]


@pytest.mark.parametrize("C,padx,pady,skew,lanes", ROW_CASES)
def test_union_sum_inside_guard_bands(C, padx, pady, skew, lanes):
    from nerf_downstream_amd._lib import check, lib

    L, B, k = lib(), 2, 3
    lists = U.related_lists(np.random.default_rng(C), "partial", 65, k, B, 2)
    want_c, _, want_o2i, _ = U.union_map(lists, B)
    N, S = want_c.shape[0], sum(c.shape[0] for c in lists)
    gen = torch.Generator().manual_seed(C)
    feats = [torch.randn(c.shape[0], C, generator=gen) for c in lists]
    want = torch.from_numpy(U.union_sum([f.numpy() for f in feats], want_o2i))
    gx = [Guarded.input(f.to(_dev()), ld=C + padx, name=f"x {i}", skew=skew if i == 1 else 0) for i, f in enumerate(feats)]
    # out2in as mink_union_build leaves it: k rows of pitch S, the entries past the count never written
    o2i = torch.full((k, S), 0x5A5A5A5A, dtype=torch.int32)
    o2i[:, :N] = torch.from_numpy(want_o2i)
    go2i = Guarded.input(o2i.to(_dev()), name="out2in")
    gy = Guarded((N, C + pady), torch.float32, _dev(), cols=C, name="y")
    vec = C % 4 == 0 and padx % 4 == 0 and pady % 4 == 0 and all(g.ptr % 16 == 0 for g in gx) and gy.ptr % 16 == 0
    assert (4 if vec else 1) == lanes
    check(L.mink_union_sum(k, _pointers(gx), (ctypes.c_int32 * k)(*[C + padx] * k), (ctypes.c_int64 * k)(*[f.shape[0] for f in feats]), C,
                           go2i.ptr, S, N, gy.ptr, C + pady, _stream()))
    torch.cuda.synchronize()
    check_all(*gx, go2i, gy)
    y = gy.logical().cpu().contiguous()
    assert_finite(y, "y")
    assert torch.equal(y.view(torch.int32), want.view(torch.int32))
