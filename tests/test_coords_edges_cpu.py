"""The C oracle of the coordinate maps against the brute-force maps (which pack no keys), bit for bit, on the inputs of
tests/edge_coords.py -- the reference tests/test_gpu_coords_edges.py holds the HIP kernels to -- and self-checks that every
generator really carries the edge it is named after, so a later edit cannot quietly take it out."""
import numpy as np
import pytest

import edge_coords as E


@pytest.fixture(scope="module")
def maps():
    from oracle import maps as M

    M.build()
    return M


_DENSE = {name: (side, org, rows) for name, side, org, rows in E.dense_cubes()}
_RUNS = E.runs()
_SIZES = E.sizes()


# ----------------------------------------------------------------------------------------- oracle == brute force
def test_corner_cubes_oracle_equals_brute_force(maps):
    rows, _ = E.corner_cubes()
    ref = E.reference_maps(maps, rows, brute=True)
    assert len(ref["ui"]) == len(rows)  # (no duplicates: every row is a voxel)


@pytest.mark.parametrize("name", sorted(_DENSE))
def test_dense_cubes_oracle_equals_brute_force(maps, name):
    side, _, rows = _DENSE[name]
    ref = E.reference_maps(maps, rows, brute=True)
    assert len(ref["ui"]) == side ** 3
    # a dense cube has every neighbour except across its faces: (side - 2)^3 rows with all 27, and 3^3 table entries
    # missing exactly where a face is crossed
    t = ref["tables"][(1, 1, 3)]
    assert int((t >= 0).all(1).sum()) == (side - 2) ** 3
    assert int((t >= 0).sum()) == (3 * side - 2) ** 3


@pytest.mark.parametrize("name", sorted(_RUNS))
def test_runs_oracle_equals_brute_force(maps, name):
    case = _RUNS[name]
    q = maps.quantize(case["field"])
    assert np.array_equal(q, case["rows"])  # the jitter stays inside the voxel
    ref = E.reference_maps(maps, q, brute=True)
    if case["plan"] is not None:
        assert np.array_equal(ref["ui"], E.run_starts(case["plan"]))  # first occurrences = the heads of the runs
        assert np.array_equal(ref["inv"], np.repeat(np.arange(len(case["plan"])), case["plan"]))
    else:
        assert np.array_equal(ref["ui"], np.arange(len(q)))


@pytest.mark.parametrize("n", E.SIZES)
def test_sizes_oracle_equals_brute_force(maps, n):
    rows = _SIZES[n]
    assert rows.shape == (n, 4) and rows.dtype == np.int32
    E.reference_maps(maps, rows, brute=True)


def test_float_edges_quantise_to_the_stated_floors(maps):
    field, want = E.float_edges()
    assert np.array_equal(maps.quantize(field), want)
    assert np.array_equal(np.floor(field.astype(np.float64)).astype(np.int64), want)
    E.reference_maps(maps, want, brute=True)
    # the values are what they claim to be in float32
    d = np.array(E.DELICATE, np.float32)
    assert d[2] < 5 and np.nextafter(d[2], np.float32(np.inf)) == 5
    assert d[3] < -5 and np.nextafter(d[3], np.float32(np.inf)) == -5
    assert d[4] < 32767 and np.nextafter(d[4], np.float32(np.inf)) == 32767
    assert 32767 < d[5] < 32768 and np.signbit(d[1]) and d[1] == 0 and d[6] == E.LO
    assert set(field[:, 0].tolist()) == {0.0, 1.0}


# --------------------------------------------------------------------------------------------------- self-checks
def _corner_claims(rows, twins):
    """The claims of corner_cubes, as a list of failures (empty = all hold)."""
    bad = []
    have = set(map(tuple, rows.tolist()))
    if np.any(np.diff(rows[:, 0]) < 0):
        bad.append("batch order")
    for b in (0, E.BMAX):
        r = rows[rows[:, 0] == b]
        for corner in range(8):
            c = tuple(E.HI if corner >> a & 1 else E.LO for a in range(3))
            if (b, *c) not in have:
                bad.append(f"corner {b} {c}")
        for axis in range(3):
            for v, step in ((E.LO, -1), (E.HI, 1)):
                if not np.any(r[:, 1 + axis] == v):  # a neighbour of such a row steps outside the range over this face
                    bad.append(f"face {b} axis {axis} at {v}")
    for a, d, t in twins:
        if a not in have or t not in have:
            bad.append(f"twin {a} {t} missing")
        outside = [a[1 + i] + d[i] for i in range(3)]
        if all(E.LO <= v <= E.HI for v in outside):
            bad.append(f"twin {a} + {d} stays inside")
    kinds = {(d, a[0] == t[0]) for a, d, t in twins}
    if len(kinds) != 6 + 2:  # six faces with the wrap twin; the borrow into the batch field over the two x faces
        bad.append(f"twin kinds {sorted(kinds)}")
    return bad


def test_corner_cubes_touch_every_face_and_hold_their_twins():
    rows, twins = E.corner_cubes()
    assert _corner_claims(rows, twins) == []
    assert rows[:, 0].min() == 0 and rows[:, 0].max() == E.BMAX
    assert rows[:, 1:].min() == E.LO and rows[:, 1:].max() == E.HI
    fill = sum(1 for r in rows.tolist() if all(v <= E.LO + 7 for v in r[1:]) and r[0] == 0) / 8 ** 3
    assert 0.6 < fill < 0.8
    # one cell inward and the claims fail: the check has teeth
    assert _corner_claims(*E.corner_cubes(inward=1)) != []


@pytest.mark.parametrize("name", sorted(_DENSE))
def test_dense_cubes_fill_whole_blocks(name):
    side, org, rows = _DENSE[name]
    counts = E.block_cell_counts(rows)
    full = sum(1 for n in counts.values() if n == 64)
    per_axis = [sum(1 for k in range(-(-side // 4) + 1) if org[a] <= (org[a] // 4 + k) * 4 and (org[a] // 4 + k) * 4 + 3 <= org[a] + side - 1)
                for a in range(3)]
    assert full == per_axis[0] * per_axis[1] * per_axis[2] and full >= 1
    if side % 4 == 0 and all(o % 4 == 0 for o in org):
        assert set(counts.values()) == {64} and len(counts) == (side // 4) ** 3  # on the block grid: every block is full
    else:
        assert min(counts.values()) < 64
    assert np.array_equal(rows, rows[np.lexsort((rows[:, 3], rows[:, 2], rows[:, 1], rows[:, 0]))])  # scan order


def test_dense_cases_cover_the_block_grid_offsets():
    offs = {tuple(o % 4 for o in org) for _, org, _ in _DENSE.values()}
    assert (0, 0, 0) in offs
    assert {o for t in offs for o in t} == {0, 1, 2, 3}
    assert any(min(org) < 0 and any(o % 4 for o in org) for _, org, _ in _DENSE.values())  # negative and off the grid
    assert {side for side, _, _ in _DENSE.values()} == {8, 9, 16}
    assert (-6, 3, E.LO) in {org for _, org, _ in _DENSE.values()}
    assert sum(all(o % 2 == 0 for o in org) for _, org, _ in _DENSE.values()) >= 4  # (the stride-2 dense check needs these)


def _run_claims(cases):
    bad = []
    plans = [c["plan"] for c in cases.values() if c["plan"] is not None]
    lengths = {p for plan in plans for p in plan}
    if not set(E.RUN_LENGTHS) <= lengths:
        bad.append(f"run lengths {sorted(lengths)}")
    crossed = {bd: set() for bd in E.RUN_BOUNDARIES}
    for plan in plans:
        for s, p in zip(E.run_starts(plan).tolist(), plan):
            for bd in E.RUN_BOUNDARIES:
                if p > 1 and s < bd < s + p:  # rows bd - 1 and bd are in the same run
                    crossed[bd].add(p)
    for bd, ps in crossed.items():
        if not ps:
            bad.append(f"no run crosses row {bd}")
    if not any(p > 256 for plan in plans for p in plan):
        bad.append("no run longer than a workgroup")
    if 2 not in crossed[64] or 2 not in crossed[256]:
        bad.append("no two-row run across rows 63|64 and 255|256")
    return bad


def test_runs_cross_the_wave_and_workgroup_boundaries():
    cases = E.runs()
    assert _run_claims(cases) == []
    for name, c in cases.items():
        rows = c["rows"]
        key = rows.astype(np.int64) @ np.array([1 << 48, 1 << 32, 1 << 16, 1])
        if c["ascending"]:
            assert np.all(np.diff(key) > 0), name
        else:
            assert np.all(np.diff(key) >= 0) and np.any(np.diff(key) == 0), name  # sorted, with equal neighbours
            f = c["field"]
            assert not np.all(np.diff(f[:, 3]) >= 0)  # jitter: the float rows themselves are not in order
        if c["plan"] is not None:  # the rows really hold the planned runs
            same = np.concatenate([[False], np.all(rows[1:] == rows[:-1], axis=1)])
            assert np.array_equal(np.nonzero(~same)[0], E.run_starts(c["plan"])), name
    one = cases["one_key_1000"]["rows"]
    assert len(one) == 1000 and len(np.unique(one, axis=0)) == 1
    assert cases["long_runs"]["rows"][63].tolist() == cases["long_runs"]["rows"][64].tolist()
    assert cases["long_runs"]["rows"][255].tolist() == cases["long_runs"]["rows"][256].tolist()
    # shortened runs no longer reach over the boundaries: the check has teeth
    assert _run_claims(E.runs(shorten=40)) != []


def test_sizes_sit_on_the_table_wave_and_workgroup_boundaries():
    assert set(E.SIZES) == set(_SIZES)
    for n in (32, 64, 256, 1024, 4096):  # cap = 2^k >= 2 n changes between n and n + 1; n - 1 .. n + 1 straddle 64 / 256
        assert {n - 1, n, n + 1} <= set(E.SIZES) or n == 4096 and {n, n + 1} <= set(E.SIZES)
    for n, rows in _SIZES.items():
        assert np.all(np.diff(rows[:, 0]) >= 0) and rows[:, 0].min() >= 0


def test_illegal_fields_hold_exactly_one_illegal_value_each():
    fields = E.illegal_fields()
    assert len(fields) == len(E.ILLEGAL) * 4
    assert {"coord_32768", "coord_-32768.5", "batch_65535", "batch_-1", "coord_nan", "coord_+inf", "coord_-inf", "coord_1e20",
            "coord_-1e20"} <= set(E.ILLEGAL)
    for name, pos, f in fields:
        fl = np.floor(f.astype(np.float64))
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(fl) & np.concatenate([(fl[:, :1] >= 0) & (fl[:, :1] <= E.BMAX), (fl[:, 1:] >= E.LO) & (fl[:, 1:] <= E.HI)], 1)
        assert int((~ok).sum()) == 1, (name, pos)
        i = int(np.nonzero(~ok)[0][0])
        assert len(f) == (1 if pos == "alone" else 301)
        assert i == {"alone": 0, "first": 0, "last": 300, "middle": 150}[pos], (name, pos)
    legal = np.floor(E.legal_field().astype(np.float64))
    assert legal[:, 0].min() >= 0 and np.abs(legal).max() < 100
