"""-m gpu: the count -> scan -> fill entry points of csrc/rulebook.hip (mink_rulebook, mink_class_partition,
mink_class_partition_batch) write nothing outside the buffers they are given.

Their workspace is carved by one helper (chunk_ws: counts | offsets | total, one counter column per 256-row chunk), so the row
counts sit on the chunk boundary and on both sides of it: 1, 255, 256, 257, 513.  Every workspace is a guarded.Guarded of
EXACTLY *_workspace_bytes() bytes and every output is guarded; the results are held to the references of test_gpu_coords.py
(the oracle's table and its ME-format lists) and to helpers.class_perm."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from guarded import Guarded, check_all
from helpers import class_perm

pytestmark = pytest.mark.gpu

ROWS = (1, 255, 256, 257, 513)
TS, PAD = 2, 128


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ws(nbytes, name):
    return Guarded(int(nbytes), torch.uint8, "cuda", written="any", name=name)


@functools.lru_cache(maxsize=None)
def _rows(n):
    """n distinct rows of a tensor-stride-2 map (one batch, cells of a 12^3 grid in scan order, negative ones among them)."""
    cells = np.sort(np.random.default_rng(n).permutation(12 ** 3)[:n])
    c = np.zeros((n, 4), np.int32)
    c[:, 1], c[:, 2], c[:, 3] = cells // 144 - 6, cells // 12 % 12 - 6, cells % 12 - 6
    c[:, 1:] *= TS
    return c


@functools.lru_cache(maxsize=None)
def _want_perm(n):
    """The whole permutation buffer: helpers.class_perm of the rows' parity classes, and -1 behind it."""
    cell = torch.from_numpy(_rows(n)[:, 1:].astype(np.int64)) // TS
    segs = class_perm((cell[:, 0] & 1) | ((cell[:, 1] & 1) << 1) | ((cell[:, 2] & 1) << 2), PAD)
    return torch.cat([segs, torch.full((n + 8 * (PAD - 1) - len(segs),), -1, dtype=torch.int32)])


@pytest.mark.parametrize("n", ROWS)
def test_rulebook_stays_inside_an_exact_workspace(oracle_maps, n):
    from nerf_downstream_amd._lib import check, lib

    L, K = lib(), 27
    table = oracle_maps.kernel_map_table(_rows(n), _rows(n), oracle_maps.kernel_offsets(3, TS))
    want = oracle_maps.table_to_lists(table)
    total = sum(v.shape[1] for v in want.values())
    nbr = Guarded.input(torch.from_numpy(table).cuda(), name="nbr")
    counts = Guarded((K + 1,), torch.int32, "cuda", name="counts")
    live = torch.arange(n * K) < total  # pairs_in / pairs_out hold n_out * K entries, the first `total` are written
    pin = Guarded((n * K,), torch.int32, "cuda", written=live, name="pairs_in")
    pout = Guarded((n * K,), torch.int32, "cuda", written=live, name="pairs_out")
    ws = _ws(L.mink_rulebook_workspace_bytes(n, K), "rulebook workspace")
    check(L.mink_rulebook(nbr.ptr, n, K, counts.ptr, pin.ptr, pout.ptr, ws.ptr, ws.nbytes, _st()))
    torch.cuda.synchronize()
    check_all(nbr, counts, pin, pout, ws)
    c = counts.t.tolist()
    assert c[0] == 0 and c[K] == total
    got = {k: np.stack([pin.t[c[k] : c[k + 1]].cpu().numpy(), pout.t[c[k] : c[k + 1]].cpu().numpy()]) for k in range(K) if c[k + 1] > c[k]}
    assert sorted(got) == sorted(want)
    for k, v in got.items():
        assert np.array_equal(v, want[k]), k


@pytest.mark.parametrize("n", ROWS)
def test_class_partition_stays_inside_an_exact_workspace(n):
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    rows = int(L.mink_class_partition_rows(n, PAD))
    assert rows == n + 8 * (PAD - 1)
    coords = Guarded.input(torch.from_numpy(_rows(n)).cuda(), name="coords")
    perm = Guarded((rows,), torch.int32, "cuda", name="perm")
    ws = _ws(L.mink_class_partition_workspace_bytes(n), "class_partition workspace")
    check(L.mink_class_partition(coords.ptr, n, TS, PAD, perm.ptr, ws.ptr, ws.nbytes, _st()))
    torch.cuda.synchronize()
    check_all(coords, perm, ws)
    assert torch.equal(perm.t.cpu(), _want_perm(n))


@pytest.mark.parametrize("n_a,n_b", [(1, 513), (255, 257), (256, 1), (257, 255), (513, 256)])
def test_class_partition_batch_stays_inside_exact_workspaces(n_a, n_b):
    from nerf_downstream_amd._lib import ClassPartitionDesc, check, lib

    L = lib()
    descs = (ClassPartitionDesc * 2)()
    bufs = []
    for d, n in zip(descs, (n_a, n_b)):
        coords = Guarded.input(torch.from_numpy(_rows(n)).cuda(), name=f"coords[{n}]")
        perm = Guarded((int(L.mink_class_partition_rows(n, PAD)),), torch.int32, "cuda", name=f"perm[{n}]")
        ws = _ws(L.mink_class_partition_workspace_bytes(n), f"class_partition workspace[{n}]")
        d.coords, d.n, d.ts, d.pad, d.perm, d.workspace, d.workspace_bytes = coords.ptr, n, TS, PAD, perm.ptr, ws.ptr, ws.nbytes
        bufs.append((coords, perm, ws))
    check(L.mink_class_partition_batch(2, ctypes.byref(descs), _st()))
    torch.cuda.synchronize()
    for n, (coords, perm, ws) in zip((n_a, n_b), bufs):
        check_all(coords, perm, ws)
        assert torch.equal(perm.t.cpu(), _want_perm(n)), n
