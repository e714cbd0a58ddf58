"""Neighbour tables, operands and the float64 reference for the convolution kernels at the limits of their 32-bit addressing
(tests/test_gpu_big_tables.py on the GPU, tests/test_big_tables_cpu.py for the builders and the negative control).

The fast kernels form byte offsets in 32 bits: a 24-bit multiply of the row by the row pitch (`__umul24`), row 0xFFFFFF for "no
neighbour", buffer descriptors of at most 2^32 bytes.  The planners gate them by size (plan_gather / compact_operands in
csrc/conv.hip, wgrad_plan in csrc/conv_wgrad.hip).  A table built here NAMES the rows at which such arithmetic changes its
answer -- bits 22 and 23 of the row, the rows on both sides of byte 2^31 and 2^32, the last rows of the operand -- in every
column, next to missing neighbours, so a wrapped offset shows as a wrong output row; and the reference needs only the few
thousand rows a table names, never an operand of n_in or n_out rows in float64.

The thresholds ("2^24", "2^31", "2^32") are parameters: the CPU tests pass toy values and check the same code on operands small
enough to compare with a plain float64 convolution over the whole operand.  Importable without a GPU."""
import numpy as np
import torch

T24 = 1 << 24
BYTE_LIMITS = (1 << 31, 1 << 32)
ROW_TILES = (64, 128)  # rows per workgroup of the gather-GEMMs (compact: 64, dense: 128) and of the tiled weight gradient (128)


# ------------------------------------------------------------------------------------------------------------ rows
def crossing_rows(pitch_bytes, n, limits=BYTE_LIMITS):
    """For every byte limit: the last row that starts below it and the first that starts at or above it, of n rows of
    `pitch_bytes` bytes (those that exist)."""
    rows = []
    for lim in limits:
        first_at = -(-lim // pitch_bytes)  # smallest r with r * pitch >= lim
        rows += [r for r in (first_at - 1, first_at) if 0 <= r < n]
    return rows


def probe_rows(n_in, ldx, esz=4, t24=T24, limits=BYTE_LIMITS, n_random=300, seed=0):
    """The rows of an [n_in][ldx] operand of `esz`-byte elements a table must name, ascending, distinct (int64 numpy):
    both ends, the rows around bits 22 / 23 / 24 of the index (`t24` stands for 2^24), the rows on both sides of every byte
    limit, and `n_random` seeded random rows."""
    assert n_in >= 4
    rows = [0, 1, n_in - 2, n_in - 1]
    rows += [t24 // 4 - 1, t24 // 4, t24 // 2 - 1, t24 // 2, t24 - 3, t24 - 2, t24 - 1, t24]
    rows += crossing_rows(esz * ldx, n_in, limits)
    rng = np.random.default_rng(seed)
    rows += rng.integers(0, n_in, size=n_random).tolist()
    return np.unique(np.array([r for r in rows if 0 <= r < n_in], dtype=np.int64))


# ---------------------------------------------------------------------------------------------------------- tables
def check_probe_table(table, rows):
    """What probe_table promises (asserted, so a test cannot pass by never touching the probes): entries are -1 or probe rows;
    every probe row appears in every column; every column holds a -1; one row is all -1; the row count is no multiple of the
    kernels' row tiles, so the last tile is ragged."""
    t = table.numpy() if isinstance(table, torch.Tensor) else np.asarray(table)
    rows = np.asarray(rows, dtype=np.int64)
    n_out, K = t.shape
    assert all(n_out % tile for tile in ROW_TILES), f"{n_out} rows: the last tile must be ragged"
    assert np.isin(t, np.concatenate([rows, [-1]])).all(), "an entry that is neither -1 nor a probe row"
    for k in range(K):
        col = t[:, k]
        missing = np.setdiff1d(rows, col)
        assert missing.size == 0, f"column {k} lacks probe rows {missing[:8].tolist()}"
        assert (col == -1).any(), f"column {k} has no missing neighbour"
    assert (t == -1).all(axis=1).any(), "no row without any neighbour"


def probe_table(n_out, K, rows, p_missing=0.3, seed=0):
    """[n_out][K] int32 (host): entries drawn from `rows` (the probe rows: ints that fit int32), -1 at share `p_missing`;
    every probe row placed once in every column at a random output row; output row n_out // 2 has no neighbour at all."""
    rows = np.asarray(rows, dtype=np.int64)
    assert rows.size + 1 <= n_out, f"{rows.size} probe rows do not fit {n_out} output rows"
    assert rows.min() >= 0 and rows.max() < (1 << 31)
    rng = np.random.default_rng(seed)
    t = rows[rng.integers(0, rows.size, size=(n_out, K))]
    t[rng.random((n_out, K)) < p_missing] = -1
    dead = n_out // 2
    others = np.delete(np.arange(n_out), dead)
    for k in range(K):
        t[rng.permutation(others)[: rows.size], k] = rows
    t[dead] = -1
    table = torch.from_numpy(t.astype(np.int32))
    check_probe_table(table, rows)
    return table


def tile_windows(n_out, row_bytes, tile=128, limits=BYTE_LIMITS):
    """Row windows [start, stop) of an n_out-row launch: the first tile, the last (ragged) tile, and for every pitch in
    `row_bytes` (bytes per row of y / dy, of the table) and every byte limit the two tiles around the row whose offset crosses it."""
    assert n_out % tile, "the last tile must be ragged"
    wins = {(0, min(tile, n_out)), (n_out // tile * tile, n_out)}
    for pitch in row_bytes:
        for r in crossing_rows(pitch, n_out, limits):
            t0 = r // tile * tile
            wins.add((t0, min(t0 + tile, n_out)))
    return sorted(wins)


def window_rows(windows, device="cpu"):
    return torch.cat([torch.arange(a, b, device=device) for a, b in windows])


def window_table(n_out, K, n_in, windows, seed=0, device="cpu", p_missing=0.3):
    """[n_out][K] int32 made ON `device` (never on the host: n_out is the large side): -1 everywhere, and inside every window
    random rows of [0, n_in) with -1 at share `p_missing`; the first row of every window keeps all its neighbours, the second none."""
    g = torch.Generator(device=device).manual_seed(seed)
    table = torch.full((n_out, K), -1, dtype=torch.int32, device=device)
    for a, b in windows:
        assert 0 <= a < b <= n_out
        blk = torch.randint(0, n_in, (b - a, K), generator=g, device=device, dtype=torch.int32)
        blk[torch.rand(b - a, K, generator=g, device=device) < p_missing] = -1
        blk[0] = torch.randint(0, n_in, (K,), generator=g, device=device, dtype=torch.int32)
        if b - a > 1:
            blk[1] = -1
        table[a:b] = blk
    return table


# -------------------------------------------------------------------------------------------------------- operands
def fill_rows(n, c, ld, seed, device, bf16=False, chunk=1 << 21):
    """[n][c] fp32 view at row pitch `ld` of a fresh device tensor: seeded O(1) values written in chunks (no host copy, no
    temporary of n rows), rounded to bf16-representable values on request; the pad columns of a pitched operand hold NaN."""
    assert ld >= c
    buf = torch.empty(n, ld, dtype=torch.float32, device=device)
    g = torch.Generator(device=device).manual_seed(seed)
    for a in range(0, n, chunk):
        b = min(n, a + chunk)
        v = torch.randn(b - a, c, generator=g, device=device)
        buf[a:b, :c] = v.bfloat16().float() if bf16 else v
        del v
    if ld > c:
        buf[:, c:] = float("nan")
    return buf[:, :c]


# ------------------------------------------------------------------------------------------------------- reference
def gathered(table):
    """(rows, local): the distinct rows a table names, ascending (int64), and the table re-indexed into them (-1 kept)."""
    t = table.long()
    rows = torch.unique(t[t >= 0])
    local = torch.searchsorted(rows, t.clamp_min(0))
    return rows, torch.where(t >= 0, local, torch.full_like(local, -1))


def reference(xs, local, w=None, dy=None, w_transposed=False, flip_k=False, bias=None):
    """float64 (y, dw) of one convolution call from the gathered rows alone.  xs [m][cin]: the rows `gathered(table)` names, in
    its order; local [n_out][K]: the table re-indexed into them.
      y  (w given):  y[o] = sum_k xs[local[o, k]] @ W[k'] (+ bias), k' = K-1-k with flip_k, W[k'] = w[k'] as [cin][cout], or
                     w[k']^T of a [cout][cin] block with w_transposed -- the data gradients are this with xs = rows of dY;
      dw (dy given): dw[k] = xs[local[:, k]]^T @ dy over the valid pairs.
    A row without neighbours comes out as exactly the bias (or 0)."""
    xs = xs.double()
    ok = (local >= 0)
    gx = xs[local.clamp_min(0)] * ok[:, :, None].double()  # [n_out][K][cin], zeros where there is no neighbour
    y = dw = None
    if w is not None:
        wk = w.double()
        if flip_k:
            wk = wk.flip(0)
        if w_transposed:
            wk = wk.transpose(1, 2)
        y = torch.einsum("okc,kcd->od", gx, wk)
        if bias is not None:
            y = y + bias.double()
    if dy is not None:
        dw = torch.einsum("okc,od->kcd", gx, dy.double())
    return y, dw


def worst_over_bound(got, ref, atol, rtol):
    """max |got - ref| / (atol + rtol |ref|): <= 1 passes (torch.allclose's bound); NaN in `got` counts as infinitely far."""
    got, ref = got.double(), ref.double()
    q = (got - ref).abs() / (atol + rtol * ref.abs())
    q = torch.where(torch.isnan(q), torch.full_like(q, float("inf")), q)
    return float(q.max()) if q.numel() else 0.0
