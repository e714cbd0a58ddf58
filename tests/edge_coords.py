"""Seeded coordinate inputs at the limits of the 16|16|16|16-bit key space and at wave / workgroup boundaries.

Plain numpy, no torch, no GPU: shared by tests/test_coords_edges_cpu.py (C oracle against the brute-force maps, and the
self-checks that keep the edge in every generator) and tests/test_gpu_coords_edges.py (HIP kernels against both).
Every generator returns int32 rows ``[b, x, y, z]`` or a float32 field, with the batch column non-decreasing.
"""
import numpy as np

LO, HI = -32768, 32767  # legal coordinates after quantisation
BMAX = 65534            # largest legal batch index (65535 would pack into the empty-slot key)
SIZES = (1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4096, 4097)
RUN_LENGTHS = (1, 2, 63, 64, 65, 130, 300)
RUN_BOUNDARIES = (64, 128, 256, 512)


def _batch_sorted(rows):
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, 4)
    return np.ascontiguousarray(rows[np.argsort(rows[:, 0], kind="stable")], dtype=np.int32)


# --------------------------------------------------------------------------------------------------------------- corners
def corner_cubes(seed=0, side=8, fill=0.7, inward=0):
    """Partly filled cubes touching the eight corners of [LO, HI]^3 at batch 0 and BMAX, single rows at LO and HI on each
    axis, and twin rows that differ only by what a masking bug would do to a neighbour stepping over a face:

    * wrap:   (b, HI, y, z) with (b, LO, y, z) -- the 16-bit field wraps round;
    * borrow: (b, LO, y, z) with (b - 1, HI, y, z), (b, x, LO, z) with (b, x - 1, HI, z), (b, x, y, LO) with
              (b, x, y - 1, HI) -- the step carries into the next field of the packed key.

    -> (rows int32 [n, 4], twins): `twins` lists (row a, unit step d, row t): a + d is outside the range, and t is the row
    a wrong key would find there.  `inward` shifts everything off the faces by that many cells (the self-checks of the
    CPU tests must notice)."""
    rng = np.random.default_rng(seed)
    lo, hi = LO + inward, HI - inward
    rows, twins = [], []
    for b in (0, BMAX):
        for corner in range(8):
            occ = rng.random((side, side, side)) < fill
            occ[tuple(-(corner >> a & 1) for a in range(3))] = True  # the corner cell itself
            xyz = np.stack(np.nonzero(occ), 1)
            org = [hi - side + 1 if corner >> a & 1 else lo for a in range(3)]
            rows.append(np.concatenate([np.full((len(xyz), 1), b), xyz + org], 1))
        for axis in range(3):  # single rows exactly at the limits
            for v in (lo, hi):
                p = [100 + axis, -200 - axis, 300 + axis]
                p[axis] = v
                rows.append([[b] + p])
        for axis in range(3):
            step = [0, 0, 0]
            step[axis] = 1
            neg = [-s for s in step]
            # wrap twins
            p = [-1000 - 7 * axis, 1001 + 5 * axis, -1002 - 3 * axis]
            a_lo, a_hi = list(p), list(p)
            a_lo[axis], a_hi[axis] = lo, hi
            rows += [[[b] + a_lo], [[b] + a_hi]]
            twins += [((b, *a_lo), tuple(neg), (b, *a_hi)), ((b, *a_hi), tuple(step), (b, *a_lo))]
            # borrow twins: the field above `axis` (batch above x, x above y, y above z) one lower on the HI side
            q = [2000 + 11 * axis, -2001 - 13 * axis, 2002 + 17 * axis]
            t_lo, t_hi = [b] + q, [b] + q
            t_lo[1 + axis], t_hi[1 + axis] = lo, hi
            t_hi[axis] -= 1  # (column `axis` of [b, x, y, z] is the field above coordinate `axis`)
            if t_hi[0] < 0:
                t_lo[0], t_hi[0] = 1, 0  # batch 0 has no batch below it: the pair (1, LO, ..) / (0, HI, ..)
            rows += [[t_lo], [t_hi]]
            twins += [(tuple(t_lo), tuple(neg), tuple(t_hi)), (tuple(t_hi), tuple(step), tuple(t_lo))]
    rows = _batch_sorted(np.concatenate([np.asarray(r).reshape(-1, 4) for r in rows]))
    return rows, twins


# ----------------------------------------------------------------------------------------------------------- dense cubes
DENSE_CASES = (  # (side, origin, batch)
    (8, (0, 0, 0), 0),
    (8, (-8, 4, LO), 0),
    (8, (1, 2, 3), 0),
    (8, (-1, -2, -3), 1),
    (9, (-6, 3, LO), 0),
    (9, (-6, 2, LO), 0),
    (9, (HI - 8, LO, 5), 3),
    (16, (0, -16, 16), 0),
    (16, (-5, 6, -7), 0),
    (16, (HI - 15, HI - 15, HI - 15), 2),
)


def dense_cubes():
    """Fully occupied cubes, rows in scan order (x slowest, z fastest: ascending keys).  Origins on the 4-cell block grid
    (every block full: `local` = 63, all 64 mask bits) and off it by 1, 2 and 3 cells in both directions.
    -> list of (name, side, origin, rows int32 [side^3, 4])."""
    out = []
    for side, org, b in DENSE_CASES:
        g = np.arange(side)
        x, y, z = np.meshgrid(g, g, g, indexing="ij")
        xyz = np.stack([x.ravel(), y.ravel(), z.ravel()], 1) + np.asarray(org)
        rows = np.concatenate([np.full((side ** 3, 1), b), xyz], 1).astype(np.int32)
        out.append((f"side{side}_at_{org[0]}_{org[1]}_{org[2]}", side, org, np.ascontiguousarray(rows)))
    return out


def block_cell_counts(rows, ts=1):
    """Occupied cells per 4^3-cell block of a map at tensor stride ts -> dict {(b, bx, by, bz): count}."""
    c = np.asarray(rows, dtype=np.int64)
    blk = np.concatenate([c[:, :1], np.floor_divide(np.floor_divide(c[:, 1:], ts), 4)], 1)
    keys, counts = np.unique(blk, axis=0, return_counts=True)
    return {tuple(k): int(n) for k, n in zip(keys.tolist(), counts)}


# ------------------------------------------------------------------------------------------------------------------ runs
def _ascending_voxels(rng, n, box=14):
    """n distinct rows in ascending key order: three batches, a box that straddles zero (so coarser levels merge rows)."""
    cells = rng.choice(3 * box ** 3, n, replace=False)
    cells.sort()
    b, r = np.divmod(cells, box ** 3)
    x, r = np.divmod(r, box * box)
    y, z = np.divmod(r, box)
    return np.stack([b, x - box // 2, y - box // 2, z - box // 2], 1).astype(np.int32)


RUN_PLANS = {
    # one run of every length, each long one laid across a boundary; singles in between
    "long_runs": [1] * 40 + [63] + [1] * 10 + [64] + [1] * 50 + [65] + [2] + [1] * 150 + [130] + [1] * 5 + [300] + [2, 1, 1],
    # the shortest run there is, exactly on lanes 63|64, 127|128, threads 255|256 and 511|512
    "pairs_on_boundaries": [1] * 63 + [2] + [1] * 62 + [2] + [1] * 126 + [2] + [1] * 254 + [2] + [1] * 10,
    # runs that END exactly on a boundary and start right behind one
    "aligned_runs": [64, 64, 128, 1, 63, 192, 65, 63, 2],
}


def run_starts(plan):
    return np.concatenate([[0], np.cumsum(plan)[:-1]]).astype(np.int64)


def runs(seed=3, shorten=0):
    """Sorted fields whose equal keys sit in runs of adjacent rows.
    -> dict name -> dict(rows=int32 [n, 4], field=float32 [n, 4] (the same rows with jitter inside the voxel),
                         plan=run lengths or None, ascending=bool).
    `shorten` takes that many rows off every run longer than it (for the self-checks)."""
    rng = np.random.default_rng(seed)
    out = {}
    for name, plan in RUN_PLANS.items():
        plan = [max(1, p - shorten) if p > 2 else p for p in plan]
        vox = _ascending_voxels(rng, len(plan))
        rows = np.repeat(vox, plan, axis=0)
        out[name] = dict(rows=rows, plan=plan, ascending=False)
    out["one_key_1000"] = dict(rows=np.tile(np.array([[2, -7, 5, LO]], np.int32), (1000, 1)), plan=[1000], ascending=False)
    for n in (700, 1024, 1025):  # no duplicates, ascending: level 0 takes the shortcut without its hash insert
        out[f"ascending_{n}"] = dict(rows=_ascending_voxels(rng, n), plan=None, ascending=True)
    for v in out.values():
        v["rows"] = np.ascontiguousarray(v["rows"], dtype=np.int32)
        f = v["rows"].astype(np.float32)
        f[:, 1:] += rng.uniform(0.0, 0.999, (len(f), 3)).astype(np.float32)
        v["field"] = f
    return out


# ----------------------------------------------------------------------------------------------------------------- sizes
def sizes(seed=5):
    """Random legal fields of n rows (duplicates allowed), n on the boundaries of the wave (64), the workgroup (256) and the
    hash-table capacity (2^k >= 2 n).  -> dict n -> int32 [n, 4]."""
    out = {}
    for n in SIZES:
        rng = np.random.default_rng(seed + n)
        box = max(2, int(round((1.6 * n) ** (1 / 3))))
        xyz = rng.integers(-(box // 2), box - box // 2, (n, 3))
        b = np.sort(rng.integers(0, 3, (n, 1)), axis=0)
        out[n] = np.ascontiguousarray(np.concatenate([b, xyz], 1), dtype=np.int32)
    return out


# ----------------------------------------------------------------------------------------------------------- float edges
def _f32(v):
    return np.float32(v)


DELICATE = (
    _f32(-0.5), _f32(-0.0), np.nextafter(_f32(5), _f32(-np.inf)), np.nextafter(_f32(-5), _f32(-np.inf)),
    np.nextafter(_f32(32767), _f32(-np.inf)), _f32(32767.996), _f32(-32768.0),
)
DELICATE_FLOORS = (-1, 0, 4, -6, 32766, 32767, -32768)

ILLEGAL = {  # name -> (column, value)
    "coord_32768": (2, _f32(32768.0)),
    "coord_-32768.5": (2, _f32(-32768.5)),
    "batch_65535": (0, _f32(65535)),
    "batch_-1": (0, _f32(-1)),
    "coord_nan": (1, _f32(np.nan)),
    "batch_nan": (0, _f32(np.nan)),
    "coord_+inf": (3, _f32(np.inf)),
    "coord_-inf": (1, _f32(-np.inf)),
    "coord_1e20": (2, _f32(1e20)),
    "coord_-1e20": (3, _f32(-1e20)),
}
POSITIONS = ("alone", "first", "last", "middle")


def float_edges():
    """Legal float rows whose floor is delicate, at batch 0.0 and 1.0.  -> (field float32 [n, 4], floors int32 [n, 4])."""
    rows, want = [], []
    for b in (0.0, 1.0):
        for i, (v, fl) in enumerate(zip(DELICATE, DELICATE_FLOORS)):
            for axis in range(3):
                r = [b, 10.25 + i, -20.75 - i, 30.5 + axis]
                w = [int(b), 10 + i, -21 - i, 30 + axis]
                r[1 + axis], w[1 + axis] = v, fl
                rows.append(r)
                want.append(w)
    return np.asarray(rows, np.float32), np.asarray(want, np.int32)


def legal_field(n=300, seed=9):
    rng = np.random.default_rng(seed)
    f = rng.uniform(-40, 40, (n, 4)).astype(np.float32)
    f[:, 0] = np.sort(rng.integers(0, 3, n)).astype(np.float32)
    return f


def illegal_fields():
    """Every illegal value alone, first, last and in the middle of a 300-row legal field.
    -> list of (name, position, field float32 [n, 4])."""
    base = legal_field()
    out = []
    for name, (col, v) in ILLEGAL.items():
        bad = np.array([1.0, 2.5, -3.5, 4.5], np.float32)
        bad[col] = v
        for pos in POSITIONS:
            if pos == "alone":
                f = bad[None].copy()
            else:
                i = {"first": 0, "last": len(base), "middle": len(base) // 2}[pos]
                f = np.insert(base, i, bad, axis=0)
            out.append((name, pos, np.ascontiguousarray(f, dtype=np.float32)))
    return out


# ------------------------------------------------------------------------------------------------- references, shared
LEVELS = (1, 2, 4, 8, 16)
TABLE_OPS = ((1, 1, 3), (2, 2, 3), (4, 4, 3), (1, 2, 2), (1, 2, 1), (2, 4, 1))  # (ts_in, ts_out, kernel size)


def reference_maps(maps, rows, brute=True):
    """Unique rows, the stride chain to ts 16 and the kernel tables of TABLE_OPS from the C oracle (`maps` = oracle.maps);
    with `brute`, every one of them asserted equal, bit for bit, to the brute-force functions that pack no keys.
    -> dict(ui, inv, coords {ts: rows}, i2o {ts: map from ts / 2}, tables {(ts_in, ts_out, ks): nbr})."""
    rows = np.ascontiguousarray(rows, dtype=np.int32)
    ui, inv = maps.unique(rows)
    if brute:
        bui, binv = maps.unique_bruteforce(rows)
        assert np.array_equal(ui, bui) and np.array_equal(inv, binv)
    coords, i2o = {1: rows[ui]}, {}
    for ts in LEVELS[1:]:
        coords[ts], i2o[ts] = maps.stride_map(coords[ts // 2], ts)
        if brute:
            bc, bi = maps.stride_map_bruteforce(coords[ts // 2], ts)
            assert np.array_equal(coords[ts], bc) and np.array_equal(i2o[ts], bi), ts
    tables = {}
    for ts_in, ts_out, ks in TABLE_OPS:
        off = maps.kernel_offsets(ks, ts_in)
        tables[(ts_in, ts_out, ks)] = t = maps.kernel_map_table(coords[ts_in], coords[ts_out], off)
        if brute:
            assert np.array_equal(t, maps.kernel_map_bruteforce(coords[ts_in], coords[ts_out], off)), (ts_in, ts_out, ks)
    return dict(ui=ui, inv=inv, coords=coords, i2o=i2o, tables=tables)


def transposed(ref, n_in):
    """nbr_t[i, k] = o for every nbr[o, k] = i (the way the existing map tests rebuild it)."""
    ref_t = np.full((n_in, ref.shape[1]), -1, np.int32)
    o, k = np.nonzero(ref >= 0)
    ref_t[ref[o, k], k] = o
    return ref_t
