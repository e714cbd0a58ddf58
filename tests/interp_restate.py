"""float64 restatement of trilinear interpolation and splat on sparse tensors (csrc/interp.hip), written from the definitions
and independent of the backend's hash maps (tests/test_interp_cpu.py holds it to a dense grid_sample, to linear functions and to
adjointness; tests/test_gpu_interp.py holds the kernels to it).

A query is a float32 row (b, x, y, z) read against integer coordinates at tensor stride ts.  Per axis lo = floor(x / ts) ts,
made to satisfy lo <= x < lo + ts exactly, d = (x - lo) / ts.  Corner c in 0..7 has bit 0 = x, bit 1 = y, bit 2 = z: a set bit
means coordinate lo + ts and factor d, a clear bit lo and 1 - d; its weight is the product of the three factors.  A Python dict
(b, x, y, z) -> row finds the corners; imap[q][c] = the row or -1.  The batch index is int(b).  The weights are computed in
float64 from the float32 inputs (the conversion is exact).

  interp_fwd   y[q]  = sum_c w[q][c] x[imap[q][c]] over the present corners
  interp_bwd   dx[i] = sum over the pairs (q, c) with imap[q][c] = i of w[q][c] dy[q]
  splat_coords the eight corners of floor(coords) of every row at tensor stride 1, listed (point 0, corners 0..7), (point 1,
               ...), unique in first-occurrence order, and imap[p][c] = the row of corner c of point p
  splat_fwd    F_s[v] = sum over (p, c) -> v of w[p][c] F[p]  (= interp_bwd over the splat's map)
`*_abs` return the sums of absolute values entering every output row (sum |x_c| over the found corners -- weights NOT
applied, as the tests' bounds are stated -- and sum |dy_q| over the pairs) and the pair count per row."""
import numpy as np
import torch

F64 = torch.float64
EPS32 = 2.0 ** -24  # unit roundoff of fp32


def cells(tfield, ts):
    """-> (b int64 [n], lo int64 [n, 3], d float64 [n, 3]) of float32 queries [n, 4]."""
    assert tfield.dtype == torch.float32
    q = tfield.double().numpy()
    ts = int(ts)
    xyz = q[:, 1:]
    lo = np.floor(xyz / ts) * ts
    lo = np.where(lo > xyz, lo - ts, lo)
    lo = np.where(xyz >= lo + ts, lo + ts, lo)
    assert bool(np.all((lo <= xyz) & (xyz < lo + ts)))
    d = (xyz - lo) / ts  # (x - lo is exact in float64: both are float32 values of magnitude below 2^16)
    return torch.from_numpy(q[:, 0].astype(np.int64)), torch.from_numpy(lo.astype(np.int64)), torch.from_numpy(d)


def corner_weights(d):
    """w float64 [n, 8] from d [n, 3]: corner c takes d where its bit is set, 1 - d where it is clear."""
    cols = []
    for c in range(8):
        f = [d[:, a] if (c >> a) & 1 else 1.0 - d[:, a] for a in range(3)]
        cols.append(f[0] * f[1] * f[2])
    return torch.stack(cols, 1)


def corner_coords(b, lo, ts):
    """int64 [n, 8, 4]: (b, x, y, z) of the eight corners."""
    bits = torch.tensor([[(c >> a) & 1 for a in range(3)] for c in range(8)], dtype=torch.int64)
    xyz = lo[:, None, :] + bits[None] * int(ts)
    return torch.cat([b[:, None, None].expand(-1, 8, 1), xyz], 2)


def map_weight(coords_of_map, ts, tfield):
    """-> (imap int64 [n, 8], w float64 [n, 8]) of the queries `tfield` against the integer rows `coords_of_map`."""
    lut = {tuple(c): i for i, c in enumerate(coords_of_map.tolist())}
    assert len(lut) == coords_of_map.shape[0], "duplicate coordinates"
    b, lo, d = cells(tfield, ts)
    cc = corner_coords(b, lo, ts)
    imap = torch.tensor([[lut.get(tuple(c), -1) for c in row] for row in cc.tolist()], dtype=torch.int64).reshape(-1, 8)
    return imap, corner_weights(d)


def _rows(x, imap):
    """[n, 8, C]: the corner rows of x, zeros where absent."""
    xp = torch.cat([x.to(F64), torch.zeros(1, x.shape[1], dtype=F64)], 0)
    return xp[imap]  # (-1 indexes the zero row)


def interp_fwd(x, imap, w):
    return (_rows(x, imap) * w[:, :, None]).sum(1)


def interp_fwd_abs(x, imap):
    """sum over the found corners of |x_c| per (query, channel)."""
    return _rows(x.abs(), imap).sum(1)


def _scatter(vals, imap, n_in):
    """sum of vals[q, c, :] into row imap[q, c] (absent pairs dropped) -> [n_in, C]."""
    C = vals.shape[2]
    out = torch.zeros(n_in + 1, C, dtype=F64)
    idx = torch.where(imap >= 0, imap, torch.full_like(imap, n_in)).reshape(-1)
    out.index_add_(0, idx, vals.reshape(-1, C))
    return out[:n_in]


def interp_bwd(dy, imap, w, n_in):
    return _scatter(dy.to(F64)[:, None, :] * w[:, :, None], imap, n_in)


def interp_bwd_abs(dy, imap, n_in):
    """(sum over the pairs of |dy_q| per (row, channel), pair count per row)."""
    s = _scatter(dy.to(F64).abs()[:, None, :].expand(-1, 8, -1), imap, n_in)
    cnt = _scatter(torch.ones(imap.shape[0], 8, 1, dtype=F64), imap, n_in)[:, 0].long()
    return s, cnt


def splat_coords(tfield):
    """-> (coords int64 [m, 4] in first-occurrence order, imap int64 [n, 8], w float64 [n, 8])."""
    b, lo, d = cells(tfield, 1)
    seen, out, imap = {}, [], []
    for row in corner_coords(b, lo, 1).tolist():
        for c in row:
            key = tuple(c)
            if key not in seen:
                seen[key] = len(out)
                out.append(key)
            imap.append(seen[key])
    return (torch.tensor(out, dtype=torch.int64).reshape(-1, 4), torch.tensor(imap, dtype=torch.int64).reshape(-1, 8),
            corner_weights(d))


def splat_fwd(F, imap, w, n_rows):
    return interp_bwd(F, imap, w, n_rows)


def splat_fwd_abs(F, imap, n_rows):
    return interp_bwd_abs(F, imap, n_rows)
