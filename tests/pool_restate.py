"""float64 restatement of the sparse pooling family (csrc/pool.hip), written from the definitions and independent of the
backend's coordinate maps and tables (tests/test_pool_cpu.py holds it to autograd and to hand cases, tests/test_gpu_pool.py
holds the kernels to it).

Maps.  Coordinates are integer rows (b, x, y, z) at tensor stride ts.  A pooling of stride s has the output coordinates
floor(c / (ts s)) (ts s), unique, in first-occurrence order (the backend's order: minkowski/coords.py); a Python dict
(b, x, y, z) -> row finds the inputs.  The window of an output o holds the inputs at o + offset for the offsets of
`coords.kernel_offsets(k, ts)` (already multiplied by ts), in that order; table[o][j] is the input row at offset j, or -1.

Operators, all float64 torch (the forwards are differentiable, the backwards are the explicit formulas):
  sum    y[o] = sum of the present x[table[o][j]]                         dx[i] = sum over (o, j) with table[o][j] = i of dy[o]
  avg    y[o] = that sum / cnt[o], cnt[o] = number of present entries     dx[i] = sum ... of dy[o] / cnt[o]
  max    y[o][c] = max over the present entries, arg[o][c] = its row, the lowest j on a tie; no entry: 0 / -1; a NaN is the
         maximum (torch's max_pool1d, amax, max(dim)) and the first NaN the arg (torch's max(dim))
         dx[i][c] = sum over the windows o that contain i of dy[o][c] where arg[o][c] = i
  global max / sum over the row ranges [off[b], off[b+1]): the lowest row wins a tie; an empty sample gives 0 / -1
`*_abs` return the sum of the absolute values entering every output entry -- what an fp32 summation's rounding is
proportional to, and what the tests' bounds are computed from."""
import torch

from nerf_downstream_amd.minkowski.coords import kernel_offsets

F64 = torch.float64
EPS32 = 2.0 ** -24  # unit roundoff of fp32


# ------------------------------------------------------------------------------------------------ maps
def strided_coords(coords, ts, s):
    """-> (out [m, 4] int64, in2out [n] int64): floor(c / (ts s)) (ts s), unique, first-occurrence order."""
    t = int(ts) * int(s)
    seen, out, i2o = {}, [], []
    for b, x, y, z in coords.tolist():
        key = (b, x // t * t, y // t * t, z // t * t)  # (Python's // floors: negative coordinates round down)
        if key not in seen:
            seen[key] = len(out)
            out.append(key)
        i2o.append(seen[key])
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 4), torch.tensor(i2o, dtype=torch.int64)


def window_table(coords, out, ts, k):
    """table [m, k^3] int64: the input row at out[o] + offset j (offsets of kernel_offsets(k, ts), in order), or -1."""
    lut = {tuple(c): i for i, c in enumerate(coords.tolist())}
    assert len(lut) == coords.shape[0], "duplicate coordinates"
    offs = kernel_offsets(k, ts).tolist()
    rows = [[lut.get((b, x + dx, y + dy, z + dz), -1) for dx, dy, dz in offs] for b, x, y, z in out.tolist()]
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), len(offs))


def pooling_maps(coords, ts, k, s):
    """-> (out coordinates, table) of a pooling layer (kernel k, stride s) on `coords` at tensor stride ts."""
    out = coords.long() if s == 1 else strided_coords(coords, ts, s)[0]
    return out, window_table(coords, out, ts, k)


def offsets_of(coords, B):
    """Row ranges of the samples: off[b] .. off[b+1] (rows sorted by batch index)."""
    cnt = torch.bincount(coords[:, 0].long(), minlength=B).tolist()
    off = [0]
    for c in cnt:
        off.append(off[-1] + c)
    return off


# ------------------------------------------------------------------------------------------------ local pools
def _gather(x, table):
    """[m, K, C]: the window rows of x, zeros where the entry is empty."""
    xp = torch.cat([x.to(F64), torch.zeros(1, x.shape[1], dtype=F64)], 0)
    return xp[table]  # (-1 indexes the zero row)


def counts(table):
    return (table >= 0).sum(1)


def sum_fwd(x, table):
    return _gather(x, table).sum(1)


def avg_fwd(x, table):
    return _gather(x, table).sum(1) / counts(table).clamp_min(1).to(F64)[:, None]


def _scatter(terms, table, n_in):
    """dx[i] = sum over (o, j) with table[o][j] = i of terms[o] ([m, C]) or terms[o][j] ([m, K, C])."""
    dx = torch.zeros(n_in, terms.shape[-1], dtype=F64)
    for j in range(table.shape[1]):
        o = torch.nonzero(table[:, j] >= 0).squeeze(1)
        if o.numel():
            dx.index_add_(0, table[o, j], terms[o] if terms.dim() == 2 else terms[o, j])
    return dx


def sum_bwd(dy, table, n_in):
    return _scatter(dy.to(F64), table, n_in)


def avg_bwd(dy, table, n_in):
    return _scatter(dy.to(F64) / counts(table).clamp_min(1).to(F64)[:, None], table, n_in)


def sum_fwd_abs(x, table, avg=False):
    a = _gather(x.abs(), table).sum(1)
    return a / counts(table).clamp_min(1).to(F64)[:, None] if avg else a


def sum_bwd_abs(dy, table, n_in, avg=False):
    a = dy.to(F64).abs()
    return _scatter(a / counts(table).clamp_min(1).to(F64)[:, None] if avg else a, table, n_in)


def max_fwd(x, table):
    """-> (y [m, C], arg [m, C] int64): the lowest j wins a tie; a window without entries gives 0 / -1."""
    m, K = table.shape
    v = _gather(x, table)
    v = torch.where((table >= 0)[:, :, None], v, torch.full_like(v, -float("inf")))
    y = v.max(1).values
    # the lowest present j attaining the maximum; a NaN is the maximum (torch's rule) and `==` does not find it
    hit = ((v == y[:, None, :]) | (torch.isnan(v) & torch.isnan(y)[:, None, :])) & (table >= 0)[:, :, None]
    first = torch.where(hit, torch.arange(K)[None, :, None], K).min(1).values
    empty = counts(table) == 0
    arg = torch.gather(table, 1, first.clamp_max(K - 1))
    y = torch.where(empty[:, None], torch.zeros_like(y), y)
    arg = torch.where(empty[:, None], torch.full_like(arg, -1), arg)
    return y, arg


def max_fwd_forced(x, arg):
    """y[o][c] = x[arg[o][c]][c] (0 where arg = -1): the maximum under GIVEN decisions, differentiable in x."""
    cols = torch.arange(x.shape[1])[None, :].expand_as(arg)
    y = x[arg.clamp_min(0), cols]
    return torch.where(arg >= 0, y, torch.zeros_like(y))


def max_bwd(dy, arg, table, n_in):
    """dx[i][c] = sum over the windows o containing i of dy[o][c] where arg[o][c] = i."""
    g = dy.to(F64)[:, None, :]
    terms = torch.where(arg[:, None, :] == table[:, :, None], g, torch.zeros_like(g))  # (a row not chosen receives 0, not 0 x dy)
    return _scatter(terms, table, n_in)


def max_bwd_abs(dy, arg, table, n_in):
    return max_bwd(dy.abs(), arg, table, n_in)


# ------------------------------------------------------------------------------------------------ global pools
def global_max_fwd(x, off):
    """-> (y [B, C], arg [B, C] int64 rows of x): the lowest row wins a tie; an empty sample gives 0 / -1."""
    B, C = len(off) - 1, x.shape[1]
    y, arg = torch.zeros(B, C, dtype=F64), torch.full((B, C), -1, dtype=torch.int64)
    for b in range(B):
        lo, hi = off[b], off[b + 1]
        if hi > lo:
            seg = x[lo:hi].to(F64)
            y[b] = seg.max(0).values
            hit = (seg == y[b][None]) | (torch.isnan(seg) & torch.isnan(y[b])[None])  # (a NaN is the maximum, the first one the arg)
            arg[b] = torch.where(hit, torch.arange(hi - lo)[:, None], hi - lo).min(0).values + lo
    return y, arg


def global_max_bwd(dy, arg, n):
    """dx is zero except dx[arg[b][c]][c] = dy[b][c]."""
    dx = torch.zeros(n, dy.shape[1], dtype=F64)
    b, c = torch.nonzero(arg >= 0, as_tuple=True)
    dx[arg[b, c], c] = dy.to(F64)[b, c]
    return dx


def global_sum_fwd(x, off):
    return torch.stack([x[off[b]:off[b + 1]].to(F64).sum(0) for b in range(len(off) - 1)])


def global_sum_bwd(dy, off):
    return torch.cat([dy.to(F64)[b][None].expand(off[b + 1] - off[b], -1) for b in range(len(off) - 1)])


def global_avg_fwd(x, off):
    """Mean of the sample's rows; an empty sample gives 0 (MinkowskiGlobalAvgPooling)."""
    return torch.stack([x[off[b]:off[b + 1]].to(F64).sum(0) / max(off[b + 1] - off[b], 1) for b in range(len(off) - 1)])
