"""-m gpu: mink_lidar_decode_scans / mink_lidar_finish_rows inside guard bands (tests/guarded.py), by the rules of
tests/test_gpu_guard_rowpass.py: the C ABI directly, every output a Guarded of exactly the size include/mink_hip.h names,
every input a Guarded.input with NaN bands.  After the call: check() on every buffer (bands untouched, every element the
header says is written no longer the sentinel, pad columns and every other element bit for bit as before), then the values
against tests/lidar_restate.py.  The lane form is restated from the host code: 16-byte rows iff every pointer involved is
16-byte aligned and the feature pitch (and, for the finish step, the first column) is a multiple of 4; dwords otherwise --
through a pitch of 5 or 7, a first column of 1, or a pointer that Guarded(skew=4) puts 4 bytes behind a 16-byte boundary.
Nothing here is meant to fault."""
import numpy as np
import pytest
import torch

from guarded import Guarded, check_all
from lidar_restate import decode, finish, label_table, synthetic_scan

pytestmark = pytest.mark.gpu

IGNORE = -100
SIZES = (130, 0, 1, 64, 200)  # 395 rows: two workgroups, an empty scan, a single row, a wave


def _dev():
    return torch.device("cuda", 0)


def _stream():
    return torch.cuda.current_stream().cuda_stream


# (ldo, skew of scan / coords / feats, labels given) -> the lanes the host picks
DECODE = [
    (4, 0, 0, 0, True, 4),    # exact size, 16-byte rows
    (8, 0, 0, 0, True, 4),    # NaN pad columns 4..7, still 16-byte rows
    (5, 0, 0, 0, True, 1),    # a pitch of 5: dwords
    (4, 4, 0, 0, True, 1),    # the scan 4 bytes behind a 16-byte boundary
    (4, 0, 4, 0, False, 1),   # the coordinates; NULL labels
    (8, 0, 0, 4, True, 1),    # the features
]


@pytest.mark.parametrize("ldo,skew_s,skew_c,skew_f,with_labels,lanes", DECODE)
def test_decode_inside_guard_bands(ldo, skew_s, skew_c, skew_f, with_labels, lanes):
    from nerf_downstream_amd._lib import check, lib

    rng = np.random.default_rng(ldo + skew_s + skew_c + skew_f)
    pairs = [synthetic_scan(rng, n) for n in SIZES]
    scans, words = [p[0] for p in pairs], [p[1] for p in pairs]
    words[0][5], words[4][199] = 260, 0xFFFF  # two ids outside the table
    n = sum(SIZES)
    offs = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int32)
    table, _ = label_table(IGNORE)
    gs = Guarded.input(torch.from_numpy(np.concatenate(scans)).to(_dev()), name="scan", skew=skew_s)
    gw = Guarded.input(torch.from_numpy(np.concatenate(words).view(np.int32)).to(_dev()), name="raw_labels") if with_labels else None
    go = Guarded.input(torch.from_numpy(offs).to(_dev()), name="scene_offsets")
    gl = Guarded.input(torch.from_numpy(table.astype(np.int32)).to(_dev()), name="lut")
    gc = Guarded((n, 4), torch.float32, _dev(), name="coords", skew=skew_c)
    gf = Guarded((n, ldo), torch.float32, _dev(), cols=4, name="feats", skew=skew_f)
    glab = Guarded((n,), torch.int32, _dev(), name="labels")
    gst = Guarded((1,), torch.int32, _dev(), name="status")
    assert (4 if ldo % 4 == 0 and all(g.ptr % 16 == 0 for g in (gs, gc, gf)) else 1) == lanes
    check(lib().mink_lidar_decode_scans(gs.ptr, gw.ptr if gw else None, n, go.ptr, len(SIZES), gl.ptr, len(table), IGNORE, gc.ptr, gf.ptr,
                                        ldo, glab.ptr, gst.ptr, _stream()))
    torch.cuda.synchronize()
    check_all(gs, gw, go, gl, gc, gf, glab, gst)
    rc, rf, rl, bad = decode(scans, words if with_labels else [None] * len(SIZES), table, IGNORE)
    assert np.array_equal(gc.logical().cpu().numpy().view(np.uint32), rc.view(np.uint32))
    assert np.array_equal(gf.logical().cpu().numpy().view(np.uint32), rf.view(np.uint32))
    assert np.array_equal(glab.t.cpu().numpy(), rl) and int(gst.t.item()) == bad == (2 if with_labels else 0)


def test_decode_of_an_empty_batch_writes_only_the_status_word():
    from nerf_downstream_amd._lib import check, lib

    go = Guarded.input(torch.zeros(3, dtype=torch.int32, device=_dev()), name="scene_offsets")
    gl = Guarded.input(torch.zeros(260, dtype=torch.int32, device=_dev()), name="lut")
    gc = Guarded((0, 4), torch.float32, _dev(), name="coords")
    gst = Guarded((1,), torch.int32, _dev(), name="status")
    check(lib().mink_lidar_decode_scans(gc.ptr, None, 0, go.ptr, 2, gl.ptr, 260, IGNORE, gc.ptr, gc.ptr, 4, gc.ptr, gst.ptr, _stream()))
    torch.cuda.synchronize()
    check_all(go, gl, gc, gst)
    assert int(gst.t.item()) == 0


def test_overlapping_operands_are_refused_before_any_launch():
    """The kernels' pointers are __restrict__: byte ranges that share a byte -- not only equal base pointers -- are an
    argument error, and nothing is written."""
    from nerf_downstream_amd._lib import lib

    n = 64
    g = Guarded((3 * n, 4), torch.float32, _dev(), written=False, name="arena")
    go = Guarded.input(torch.tensor([0, n], dtype=torch.int32, device=_dev()), name="scene_offsets")
    gl = Guarded.input(torch.zeros(260, dtype=torch.int32, device=_dev()), name="lut")
    glab = Guarded((n,), torch.int32, _dev(), written=False, name="labels")
    gst = Guarded((1,), torch.int32, _dev(), written="any", name="status")  # (zeroed before the operands are looked at)
    row = 16
    a, b, c = g.ptr, g.ptr + n * row, g.ptr + 2 * n * row  # three disjoint [n][4] matrices: accepted below with n = 0 rows only
    L = lib()
    for scan, coords, feats in [(a, a + row, c), (a, b, b + 8 * row), (a + (n - 1) * row, b, a), (a, b, b)]:
        assert L.mink_lidar_decode_scans(scan, None, n, go.ptr, 1, gl.ptr, 260, IGNORE, coords, feats, 4, glab.ptr, gst.ptr, _stream()) != 0
        assert b"overlap" in L.mink_last_error()
    assert L.mink_lidar_decode_scans(a, None, n, go.ptr, 1, gl.ptr, 260, IGNORE, b, c, 4, a + 4, gst.ptr, _stream()) != 0  # labels in the scan
    gn = Guarded.input(torch.tensor([n], dtype=torch.int32, device=_dev()), name="n_rows")
    for coords, feats, count in [(a, a + (n - 1) * row, gn.ptr), (a, b, a + 8), (a, b, b + 12)]:
        assert L.mink_lidar_finish_rows(coords, n, count, 0.05, feats, 4, 0, _stream()) != 0
        assert b"overlap" in L.mink_last_error()
    torch.cuda.synchronize()
    check_all(g, go, gl, glab, gn)


# (ldf, first column c0, skew of coords / feats) -> lanes
FINISH = [
    (4, 0, 0, 0, 4),    # exact size, 16-byte rows
    (8, 0, 0, 0, 4),    # NaN pad columns past column 4
    (8, 4, 0, 0, 4),    # the xyz go into columns 4..6
    (7, 0, 0, 0, 1),    # a pitch of 7: dwords
    (8, 1, 0, 0, 1),    # a first column of 1
    (4, 0, 4, 0, 1),    # the coordinates 4 bytes behind a 16-byte boundary
    (8, 0, 0, 4, 1),    # the features
]
N = 395


@pytest.mark.parametrize("count", [0, 129, N, N + 1000])
@pytest.mark.parametrize("ldf,c0,skew_c,skew_f,lanes", FINISH)
def test_finish_inside_guard_bands(ldf, c0, skew_c, skew_f, lanes, count):
    """A device row count of 0, of 129 (inside the second workgroup), of n, and one past the buffers (clamped to n)."""
    from nerf_downstream_amd._lib import check, lib

    rng = np.random.default_rng(ldf + c0)
    r = np.concatenate([rng.integers(0, 4, (N, 1)).astype(np.float32), (rng.random((N, 3)) * 160 - 80).astype(np.float32)], 1)
    r[7, 1:] = [0.05, -0.05, 0.0]
    cols = max(4, c0 + 3)  # (the columns right of them are NaN pads)
    f0 = rng.random((N, cols)).astype(np.float32)
    k = min(count, N)
    rows = torch.arange(N) < k
    wc = rows[:, None] & torch.tensor([False, True, True, True])
    wf = rows[:, None] & ((torch.arange(cols) >= c0) & (torch.arange(cols) < c0 + 3))
    gc = Guarded((N, 4), torch.float32, _dev(), written=wc, init=torch.from_numpy(r), name="coords", skew=skew_c)
    gf = Guarded((N, ldf), torch.float32, _dev(), written=wf, init=torch.from_numpy(f0), cols=cols, name="feats", skew=skew_f)
    gn = Guarded.input(torch.tensor([count], dtype=torch.int32, device=_dev()), name="n_rows")
    assert (4 if ldf % 4 == 0 and c0 % 4 == 0 and gc.ptr % 16 == 0 and gf.ptr % 16 == 0 else 1) == lanes
    check(lib().mink_lidar_finish_rows(gc.ptr, N, gn.ptr, 0.05, gf.ptr, ldf, c0, _stream()))
    torch.cuda.synchronize()
    check_all(gc, gf, gn)
    want_c, want_f = r.copy(), f0.copy()
    want_c[:k, 1:], want_f[:k, c0:c0 + 3] = finish(r[:k, 1:], 0.05)
    assert np.array_equal(gc.t.cpu().numpy().view(np.uint32), want_c.view(np.uint32))
    assert np.array_equal(gf.logical().cpu().numpy().view(np.uint32), want_f.view(np.uint32))
