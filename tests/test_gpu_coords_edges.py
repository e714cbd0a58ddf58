"""-m gpu: the HIP coordinate maps at the limits of the 16-bit key space and at wave / workgroup boundaries, BIT-EXACT against
the C oracle and against the brute-force maps (which pack no keys), on the inputs of tests/edge_coords.py.

Every field goes through the pyramid (`mink_coords_build_levels`, float and int32 rows) and through the single-level path
(`mink_coords_make_keys` + `mink_coords_unique`); every table through the three look-up paths (3^3 block kernel, small-K
block kernel, per-voxel hash).  Rows outside the range must raise and leave nothing behind.  On fully occupied cubes the
convolutions are also held to `torch.nn.functional.conv3d` in float64 on the densified cube -- a check that shares no
map code with the kernels or with the oracle."""
import numpy as np
import pytest
import torch

import edge_coords as E
from test_gpu_ops import ATOL, RTOL  # the fp32 convolution bounds of test_convolution: no new number here

pytestmark = pytest.mark.gpu

# the ops of test_block_index_tables_match_oracle: (kind, ts_in, ts_out, kernel size, dilation, transposed)
OPS = [("ktable", 1, 1, 3, 1, False), ("ktable", 1, 2, 2, 1, False), ("ktable", 2, 4, 3, 1, True), ("ktable", 2, 4, 1, 1, True),
       ("ktable", 4, 4, 3, 1, False), ("ktable", 4, 8, 3, 1, True), ("ktable", 8, 8, 3, 1, False), ("ktable", 8, 16, 1, 1, True),
       ("ktable", 16, 16, 3, 1, False), ("ktable", 2, 2, 2, 1, True), ("ktable", 1, 2, 1, 1, True), ("ktable", 2, 2, 3, 1, True)]

_DENSE = {name: (side, org, rows) for name, side, org, rows in E.dense_cubes()}
_RUNS = E.runs()
_SIZES = E.sizes()


def _me():
    from nerf_downstream_amd import minkowski as ME

    return ME


def _np(t):
    return t.cpu().numpy()


def _strictly_ascending(q):
    r = q.tolist()
    return all(a < b for a, b in zip(r[:-1], r[1:]))  # (lists compare like the packed keys: batch, x, y, z)


def _pyramid(field):
    """The whole pyramid in one native call (mink_coords_build_levels), ts 1 .. 16."""
    from nerf_downstream_amd.minkowski.coords import CoordinateManager

    m = CoordinateManager()
    m.insert_field(torch.from_numpy(field).cuda(), ahead_strides=(2, 2, 2, 2))
    return m


def _check_levels(m, ref, where):
    assert np.array_equal(_np(m.field_unique_index), ref["ui"]), where
    assert np.array_equal(_np(m.field_inverse), ref["inv"]), where
    for ts in E.LEVELS:
        assert m.levels[ts].n == len(ref["coords"][ts]), (where, ts)
        assert np.array_equal(_np(m.levels[ts].coords), ref["coords"][ts]), (where, ts)
        if ts > 1:
            assert np.array_equal(_np(m.in2out[(ts // 2, ts)]), ref["i2o"][ts]), (where, ts)


def _check_field_paths(oracle_maps, field, q):
    """`field` (float32 or int32 rows) through the pyramid, through TensorField + on-demand strides and through the
    single-level calls; everything against the oracle AND the brute force.  -> (pyramid manager, reference)."""
    ME = _me()
    from nerf_downstream_amd.minkowski.coords import CoordinateManager, check_block_index_overflow

    ref = E.reference_maps(oracle_maps, q, brute=True)
    fast = _strictly_ascending(q)
    m = _pyramid(field)
    assert m.levels[1].hash_empty == fast  # strictly ascending rows, and only those, skip the level-0 insert
    _check_levels(m, ref, "pyramid")
    # TensorField (level 1 alone), then every coarser level on demand: mink_coords_make_keys + mink_coords_unique per level
    t = torch.from_numpy(field).cuda()
    tf = ME.TensorField(coordinates=t, features=torch.zeros(len(field), 4, device="cuda"))
    m2 = tf.coordinate_manager
    assert m2.levels[1].hash_empty == fast
    key = ME.CoordinateMapKey(1)
    for ts in E.LEVELS[1:]:
        nxt = m2.stride(key, 2)
        assert np.array_equal(_np(m2.stride_map(key, nxt)), ref["i2o"][ts]), ts
        key = nxt
    _check_levels(m2, ref, "on demand")
    # the single-level path on the field itself (no ascending shortcut there: always the hash insert)
    m3 = CoordinateManager(device=t.device)
    lev, uidx, inv = m3._unique(t, 1 if field.dtype == np.int32 else 0, len(field), 1)
    assert lev.n == len(ref["ui"]) and np.array_equal(_np(uidx), ref["ui"]) and np.array_equal(_np(inv), ref["inv"])
    assert np.array_equal(_np(lev.coords), ref["coords"][1])
    check_block_index_overflow()
    return m, ref


def _check_tables(oracle_maps, m, ref, twins=()):
    """All tables of OPS through the batched block-index builder (3^3 kernel with and without the transposed table, small-K
    kernel for 2^3 and 1^3) and through mink_kernel_map on the per-voxel hash; -> {(ts_in, ts_out, ks): oracle table}."""
    from nerf_downstream_amd._lib import check, lib
    from nerf_downstream_amd.minkowski.coords import check_block_index_overflow, kernel_offsets

    m._build_tables_batched(OPS)
    torch.cuda.synchronize()
    assert len(m.tables) == len(OPS)
    want = {}
    for _, ts_in, ts_out, ks, dil, tr in OPS:
        cin, cout = ref["coords"][ts_in], ref["coords"][ts_out]
        off = oracle_maps.kernel_offsets(ks, ts_in)
        assert np.array_equal(off, kernel_offsets(ks, ts_in, 1))
        t = oracle_maps.kernel_map_table(cin, cout, off)
        if (ts_in, ts_out, ks) in ref["tables"]:
            assert np.array_equal(t, ref["tables"][(ts_in, ts_out, ks)])  # (held to the brute force by reference_maps)
        else:
            assert np.array_equal(t, oracle_maps.kernel_map_bruteforce(cin, cout, off))
        want[(ts_in, ts_out, ks)] = t
        t_t = E.transposed(t, len(cin))
        nbr, nbr_t = m.tables[(ts_in, ts_out, ks, dil)]
        assert np.array_equal(_np(nbr), t), ("block index", ts_in, ts_out, ks)
        assert (nbr_t is not None) == tr
        if tr:
            assert np.array_equal(_np(nbr_t), t_t), ("block index, transposed", ts_in, ts_out, ks)
        # the per-voxel hash (level 0 of an ascending field: filled on demand by hash_map)
        tkeys, tvals, cap = m.hash_map(ts_in)
        lout = m.levels[ts_out]
        K = off.shape[0]
        got = torch.empty(lout.n, K, dtype=torch.int32, device="cuda")
        got_t = torch.full((m.levels[ts_in].n, K), -1, dtype=torch.int32, device="cuda")
        check(lib().mink_kernel_map(tkeys.data_ptr(), tvals.data_ptr(), cap, lout.coords.data_ptr(), lout.n,
                                    np.ascontiguousarray(off, np.int32).ctypes.data, K, got.data_ptr(), got_t.data_ptr(), None))
        torch.cuda.synchronize()
        assert np.array_equal(_np(got), t), ("hash", ts_in, ts_out, ks)
        assert np.array_equal(_np(got_t), t_t), ("hash, transposed", ts_in, ts_out, ks)
        if twins and (ts_in, ts_out, ks) == (1, 1, 3):
            row = {tuple(c): i for i, c in enumerate(cin.tolist())}
            for a, d, tw in twins:  # a + d is outside the key space: no entry, and above all not the row a wrong key names
                k = (d[0] + 1) + 3 * (d[1] + 1) + 9 * (d[2] + 1)
                for name, tab in (("block index", _np(nbr)), ("hash", _np(got))):
                    assert tab[row[a], k] != row[tw], (name, a, d, tw)
                    assert tab[row[a], k] == -1, (name, a, d)
    check_block_index_overflow()
    assert m.block_index_ok()
    return want


def _check_pairs_partitions_offsets(oracle_maps, m, ref, want):
    ME = _me()
    keys = {ts: ME.CoordinateMapKey(ts) for ts in E.LEVELS}
    for ts_in, ts_out, ks in ((1, 1, 3), (1, 2, 2), (2, 4, 3), (2, 4, 1), (4, 4, 3)):
        km = m.kernel_map(keys[ts_in], keys[ts_out], kernel_size=ks)
        lists = oracle_maps.table_to_lists(want[(ts_in, ts_out, ks)])
        assert sorted(km.keys()) == sorted(lists.keys())
        for k, v in km.items():
            assert v.dtype == torch.int32 and np.array_equal(_np(v), lists[k]), (ts_in, ts_out, ks, k)
    for ts in (1, 2, 4):  # parity classes of negative cells
        perm = _np(m.class_perm(keys[ts], 128))
        assert np.array_equal(perm, oracle_maps.class_partition(ref["coords"][ts], ts, 128)), ts
    B = m.batch_size()
    assert B == int(ref["coords"][1][-1, 0]) + 1
    for ts in (1, 4):
        assert np.array_equal(_np(m.batch_offsets(keys[ts])), np.searchsorted(ref["coords"][ts][:, 0], np.arange(B + 1))), ts


# ------------------------------------------------------------------------------------------------------------ legal edges
@pytest.mark.parametrize("form", ["int32", "float32"])
def test_corner_cubes(oracle_maps, form):
    rows, twins = E.corner_cubes()
    field = rows if form == "int32" else rows.astype(np.float32)  # (every legal value is exact in float32)
    m, ref = _check_field_paths(oracle_maps, field, rows)
    c1 = ref["coords"][1]
    assert c1[:, 1:].min() == E.LO and c1[:, 1:].max() == E.HI and c1[:, 0].max() == E.BMAX
    want = _check_tables(oracle_maps, m, ref, twins)
    _check_pairs_partitions_offsets(oracle_maps, m, ref, want)
    # every entry of a face row that steps over the face is empty, in every table at every level
    for (ts_in, ts_out, ks), t in want.items():
        off = oracle_maps.kernel_offsets(ks, ts_in)
        tgt = ref["coords"][ts_out][:, None, 1:].astype(np.int64) + off[None].astype(np.int64)
        outside = ((tgt < E.LO) | (tgt > E.HI)).any(2)
        got = _np(m.tables[(ts_in, ts_out, ks, 1)][0])
        assert (got[outside] == -1).all(), (ts_in, ts_out, ks)
        if ks == 3 and ts_in == 1:
            assert outside.any()


@pytest.mark.parametrize("name", sorted(_DENSE))
def test_dense_cubes(oracle_maps, name):
    side, org, rows = _DENSE[name]
    m, ref = _check_field_paths(oracle_maps, rows, rows)
    assert m.levels[1].hash_empty  # scan order is ascending
    want = _check_tables(oracle_maps, m, ref)
    assert int((want[(1, 1, 3)] >= 0).sum()) == (3 * side - 2) ** 3
    _check_pairs_partitions_offsets(oracle_maps, m, ref, want)
    # the same cube with its rows shuffled (no ascending shortcut; block inserts meet the cells of a block in any order) and
    # as a float field
    perm = np.random.default_rng(side).permutation(len(rows))
    shuffled = np.ascontiguousarray(rows[perm])
    m, ref = _check_field_paths(oracle_maps, shuffled.astype(np.float32), shuffled)
    assert not m.levels[1].hash_empty
    _check_tables(oracle_maps, m, ref)


@pytest.mark.parametrize("name", sorted(_RUNS))
def test_runs(oracle_maps, name):
    case = _RUNS[name]
    for field in (case["rows"], case["field"]):  # int32 rows, and the float field with jitter inside the voxel
        m, ref = _check_field_paths(oracle_maps, field, case["rows"])
        assert m.levels[1].hash_empty == case["ascending"]
        if case["plan"] is not None:
            assert np.array_equal(ref["ui"], E.run_starts(case["plan"]))
        _check_tables(oracle_maps, m, ref)


@pytest.mark.parametrize("n", E.SIZES)
def test_sizes(oracle_maps, n):
    rows = _SIZES[n]
    for field in (rows, rows.astype(np.float32)):
        m, ref = _check_field_paths(oracle_maps, field, rows)
        _check_tables(oracle_maps, m, ref)


def test_float_edges(oracle_maps):
    field, floors = E.float_edges()
    assert np.array_equal(oracle_maps.quantize(field), floors)
    m, ref = _check_field_paths(oracle_maps, field, floors)
    assert np.array_equal(_np(m.levels[1].coords), floors[ref["ui"]])
    _check_tables(oracle_maps, m, ref)


# ----------------------------------------------------------------------------------------------------------- illegal rows
def _legal_builds_right(oracle_maps):
    legal = E.legal_field()
    q = oracle_maps.quantize(legal)
    ref = E.reference_maps(oracle_maps, q, brute=False)
    _check_levels(_pyramid(legal), ref, "after an illegal field")


@pytest.mark.parametrize("name", sorted(E.ILLEGAL))
def test_illegal_rows_raise_on_every_path_and_leave_no_status_behind(oracle_maps, name):
    """One illegal value alone, first, last and in the middle of a legal field: ValueError from TensorField, from the deferred
    pyramid and from the single-level path (the kernels set a status word, put key 0 in the row's place and carry on: nothing
    is indexed with the refused value); a legal field built right afterwards is correct."""
    ME = _me()
    from nerf_downstream_amd.minkowski.coords import CoordinateManager

    fields = [(pos, f) for nm, pos, f in E.illegal_fields() if nm == name]
    assert [pos for pos, _ in fields] == list(E.POSITIONS)
    for pos, f in fields:
        t = torch.from_numpy(f).cuda()
        with pytest.raises(ValueError, match="outside the supported range"):
            ME.TensorField(coordinates=t, features=torch.zeros(len(f), 4, device="cuda"))
        m = CoordinateManager()
        m.insert_field(t, ahead_strides=(2, 2), defer=True)  # (launched; nothing read back yet)
        with pytest.raises(ValueError, match="outside the supported range"):
            m.finish_field()
        assert not m.levels  # nothing was published
        m = CoordinateManager(device=t.device)
        with pytest.raises(ValueError, match="outside the supported range"):
            m._unique(t, 0, len(f), 1)
        torch.cuda.synchronize()
        _legal_builds_right(oracle_maps)


def test_illegal_int32_rows_raise_and_the_limits_themselves_do_not(oracle_maps):
    ME = _me()
    for bad in ([0, E.HI + 1, 0, 0], [0, 0, E.LO - 1, 0], [0, 0, 0, 1 << 16], [E.BMAX + 1, 0, 0, 0], [-1, 0, 0, 0],
                [0, -(1 << 31), 0, 0], [0, (1 << 31) - 1, 0, 0]):
        t = torch.tensor([[0, 1, 2, 3], bad, [0, 4, 5, 6]], dtype=torch.int32).cuda()
        with pytest.raises(ValueError, match="outside the supported range"):
            ME.TensorField(coordinates=t, features=torch.zeros(3, 4, device="cuda"))
    edge = np.array([[0, E.LO, E.LO, E.LO], [0, E.HI, E.HI, E.HI], [E.BMAX, E.LO, E.HI, 0], [E.BMAX, E.HI, E.LO, -1]], np.int32)
    for field in (edge, edge.astype(np.float32)):
        m, ref = _check_field_paths(oracle_maps, field, edge)
        assert np.array_equal(_np(m.levels[1].coords), edge)
    _legal_builds_right(oracle_maps)


# ------------------------------------------------------------------- convolutions on dense cubes against torch conv3d
def _close(got, ref, scale=1.0):
    return torch.allclose(got.detach().cpu().double(), ref, atol=ATOL * scale, rtol=RTOL)


def _dense_w(kernel, ks, transpose=False):
    """(K, Cin, Cout) with x fastest in K -> conv3d weights [Cout, Cin, x, y, z] (conv_transpose3d: [Cin, Cout, x, y, z])."""
    K, cin, cout = kernel.shape
    w = kernel.detach().cpu().double().view(ks, ks, ks, cin, cout)  # [z, y, x, Cin, Cout]
    return (w.permute(3, 4, 2, 1, 0) if transpose else w.permute(4, 3, 2, 1, 0)).contiguous().requires_grad_(True)


def _sparse_w_grad(w, ks, transpose=False):
    g = w.grad.permute(4, 3, 2, 0, 1) if transpose else w.grad.permute(4, 3, 2, 1, 0)  # -> [z, y, x, Cin, Cout]
    return g.reshape(ks ** 3, g.shape[3], g.shape[4])


@pytest.mark.parametrize("name", sorted(_DENSE))
def test_convolutions_on_dense_cubes_match_torch_conv3d_in_float64(name):
    """MinkowskiConvolution 3^3 stride 1 (28 -> 64 and 64 -> 64) on every cube, 2^3 stride 2 and its
    MinkowskiConvolutionTranspose on the cubes with an even origin: forward, input gradient and weight gradient against
    torch.nn.functional.conv3d / conv_transpose3d in float64 on the densified, zero-padded cube with the same weights.
    Bounds: ATOL / RTOL of test_convolution, the weight gradient's ATOL scaled by the reference's largest entry as there."""
    import torch.nn.functional as F

    ME = _me()
    side, org, rows = _DENSE[name]
    S, n = side, side ** 3
    coords = torch.from_numpy(rows).cuda()
    gen = torch.Generator().manual_seed(side * 1000 + sum(abs(o) for o in org) % 997)

    def field(c):
        feats = torch.randn(n, c, generator=gen)
        x = ME.TensorField(coordinates=coords, features=feats.cuda()).sparse()
        assert np.array_equal(_np(x.C), rows)  # scan order: row i of the map is cell i of the cube
        F_g = x.F.detach().clone().requires_grad_(True)
        D = feats.double().t().reshape(1, c, S, S, S).clone().requires_grad_(True)
        return x, F_g, D

    for cin, cout in ((28, 64), (64, 64)):
        x, F_g, D = field(cin)
        conv = ME.MinkowskiConvolution(cin, cout, kernel_size=3, stride=1, dimension=3).cuda()
        with torch.no_grad():
            conv.kernel.copy_(torch.randn(27, cin, cout, generator=gen).cuda() / (27 * cin) ** 0.5)
        y = conv(ME.SparseTensor(F_g, x.coordinate_map_key, x.coordinate_manager))
        assert np.array_equal(_np(y.C), rows)
        w = _dense_w(conv.kernel, 3)
        ref = F.conv3d(D, w, padding=1)[0].reshape(cout, n).t()
        assert _close(y.F, ref), (cin, cout, "forward")
        g = torch.randn(n, cout, generator=gen)
        y.F.backward(g.cuda())
        (ref * g.double()).sum().backward()
        assert _close(F_g.grad, D.grad[0].reshape(cin, n).t()), (cin, cout, "input gradient")
        gw = _sparse_w_grad(w, 3)
        assert _close(conv.kernel.grad, gw, max(1.0, float(gw.abs().max()))), (cin, cout, "weight gradient")
    if any(o % 2 for o in org):
        return
    # ---- 2^3 stride 2 (the cube padded with zeros to an even side) and the transposed convolution back
    cin, cout = 64, 64
    Sp = S + S % 2
    H = Sp // 2
    x, F_g, D = field(cin)
    conv = ME.MinkowskiConvolution(cin, cout, kernel_size=2, stride=2, dimension=3).cuda()
    y = conv(ME.SparseTensor(F_g, x.coordinate_map_key, x.coordinate_manager))
    c2 = _np(y.C).astype(np.int64)
    assert y.tensor_stride[0] == 2 and len(c2) == H ** 3
    ix = torch.from_numpy((c2[:, 1:] - np.asarray(org)) // 2)  # coarse cell of every output row
    assert int(ix.min()) == 0 and int(ix.max()) == H - 1
    w = _dense_w(conv.kernel, 2)
    ref = F.conv3d(F.pad(D, (0, Sp - S) * 3), w, stride=2)[0][:, ix[:, 0], ix[:, 1], ix[:, 2]].t()
    assert _close(y.F, ref), "2^3 stride 2 forward"
    g = torch.randn(len(c2), cout, generator=gen)
    y.F.backward(g.cuda())
    (ref * g.double()).sum().backward()
    assert _close(F_g.grad, D.grad[0].reshape(cin, n).t()), "2^3 stride 2 input gradient"
    gw = _sparse_w_grad(w, 2)
    assert _close(conv.kernel.grad, gw, max(1.0, float(gw.abs().max()))), "2^3 stride 2 weight gradient"
    # transposed: coarse rows (random features) up onto the cube's own map
    up = ME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=2, stride=2, dimension=3).cuda()
    f2 = torch.randn(len(c2), cin, generator=gen)
    F2_g = f2.cuda().requires_grad_(True)
    z = up(ME.SparseTensor(F2_g, y.coordinate_map_key, y.coordinate_manager))
    assert z.tensor_stride[0] == 1 and np.array_equal(_np(z.C), rows)
    f2d = f2.double().requires_grad_(True)
    D2 = torch.zeros(cin, H, H, H, dtype=torch.float64)
    D2[:, ix[:, 0], ix[:, 1], ix[:, 2]] = f2d.t()
    wt = _dense_w(up.kernel, 2, transpose=True)
    ref = F.conv_transpose3d(D2[None], wt, stride=2)[0][:, :S, :S, :S].reshape(cout, n).t()
    assert _close(z.F, ref), "transposed forward"
    g = torch.randn(n, cout, generator=gen)
    z.F.backward(g.cuda())
    (ref * g.double()).sum().backward()
    assert _close(F2_g.grad, f2d.grad), "transposed input gradient"
    gw = _sparse_w_grad(wt, 2, transpose=True)
    assert _close(up.kernel.grad, gw, max(1.0, float(gw.abs().max()))), "transposed weight gradient"
