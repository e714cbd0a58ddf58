"""float64 restatement of the point stage of the point-based classifiers (csrc/field.hip, the TensorField side of
nerf_downstream_amd/minkowski) and of the three networks built on it, written from the definitions and independent of the
backend: Python dicts find voxels, torch float64 autograd differentiates.  Nothing here calls the code under test.

Field map.  A field row (b, x, y, z) in float32 lies in the voxel of tensor stride ts with the key
(int(b), floor(floor(x) / ts) ts, ...) -- Python's // floors, negative values included.  `field_map` looks the key up among
the integer rows of a level; `field_map_brute` compares every point with every voxel instead (b equal and
v <= floor(x) < v + ts per axis), which is what tests/test_point_cpu.py holds the former to.

Networks.  `fcnn_forward` / `pointnet_forward` take the parameters by their state-dict names (float64 leaves) and run the
reference's forward (models/mink/fcnn.py:142-208, pointnet.py:100-109) in train mode without dropout: Linear, batch norm
with batch statistics (biased variance, eps 1e-5), LeakyReLU(0.01) / ReLU, convolution and max pooling over the window
tables of pool_restate (offsets of coords.kernel_offsets, in order), per-voxel mean, slice, splat / interpolation through
interp_restate, global max and average per batch sample."""
import math

import torch

import interp_restate as IR
import pool_restate as PR

F64 = torch.float64
EPS32 = PR.EPS32
BN_EPS = 1e-5


# ------------------------------------------------------------------------------------------------ the shared small case
def two_clouds(seed=5):
    """-> (coords float32 [260, 4] = (b, x, y, z), feats float32 [260, 3]): B = 2 samples of 193 and 67 points, uniform in
    [-24, 24)^3; 15 rows of each sample overwritten by copies of other rows moved inside their cell (duplicate voxels); row 0
    has x = -16.0 (on a cell boundary of every stride up to 16), row 1 x = -0.25 (floor differs from truncation)."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b, n in enumerate((193, 67)):
        xyz = torch.rand(n, 3, generator=g) * 48 - 24
        perm = torch.randperm(n - 2, generator=g) + 2
        dst, src = perm[:15], perm[15:30]
        xyz[dst] = xyz[src].floor() + torch.rand(15, 3, generator=g) * 0.98
        if b == 0:
            xyz[0, 0], xyz[1, 0] = -16.0, -0.25
        rows.append(torch.cat([torch.full((n, 1), float(b)), xyz], 1))
    coords = torch.cat(rows).float()
    feats = torch.randn(coords.shape[0], 3, generator=g).float()
    return coords, feats


def quantise(coords):
    """-> (voxels int64 [m, 4] in first-occurrence order, inverse int64 [n]) of the float rows: (int(b), floor(x), ...)."""
    q = torch.cat([coords[:, :1].double().trunc(), coords[:, 1:].double().floor()], 1).long()
    seen, out, inv = {}, [], []
    for row in q.tolist():
        key = tuple(row)
        if key not in seen:
            seen[key] = len(out)
            out.append(key)
        inv.append(seen[key])
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 4), torch.tensor(inv, dtype=torch.int64)


def level(coords, ts):
    """The integer rows of the level of tensor stride ts (a power of two) derived from the field by repeated striding by 2."""
    vox, t = quantise(coords)[0], 1
    while t < ts:
        vox, t = PR.strided_coords(vox, t, 2)[0], t * 2
    return vox


def field_key(row, ts):
    b, x, y, z = row
    return (int(b), math.floor(x) // ts * ts, math.floor(y) // ts * ts, math.floor(z) // ts * ts)


def field_map(coords, voxels, ts):
    """idx int64 [n]: the row of `voxels` (integer rows of tensor stride ts) containing every float row, -1 where none."""
    lut = {tuple(v): i for i, v in enumerate(voxels.tolist())}
    assert len(lut) == voxels.shape[0], "duplicate coordinates"
    return torch.tensor([lut.get(field_key(r, ts), -1) for r in coords.double().tolist()], dtype=torch.int64)


def field_map_brute(coords, voxels, ts):
    """The same by comparing every point with every voxel: b equal and v <= floor(x) < v + ts on every axis."""
    c = coords.double()
    b, p = c[:, 0].trunc().long(), c[:, 1:].floor().long()
    hit = (b[:, None] == voxels[None, :, 0]) & ((p[:, None, :] >= voxels[None, :, 1:]) & (p[:, None, :] < voxels[None, :, 1:] + ts)).all(2)
    assert int(hit.sum(1).max()) <= 1
    return torch.where(hit.any(1), hit.long().argmax(1), torch.full_like(b, -1))


# ------------------------------------------------------------------------------------------------ slice / mean, explicit
def gather_fwd(x, idx):
    """y[i] = x[idx[i]], zeros where idx < 0."""
    xp = torch.cat([x.to(F64), torch.zeros(1, x.shape[1], dtype=F64)], 0)
    return xp[idx]


def gather_bwd(dy, idx, n_rows):
    """dx[r] = the sum of dy[i] over the rows with idx[i] = r (index_add in float64)."""
    dx = torch.zeros(n_rows + 1, dy.shape[1], dtype=F64)
    dx.index_add_(0, torch.where(idx >= 0, idx, torch.full_like(idx, n_rows)), dy.to(F64))
    return dx[:n_rows]


def gather_bwd_abs(dy, idx, n_rows):
    """(sum of |dy[i]| entering every entry of dx, the largest segment length)."""
    live = idx[idx >= 0]
    m = int(torch.bincount(live, minlength=max(n_rows, 1)).max()) if live.numel() else 0
    return gather_bwd(dy.abs(), idx, n_rows), m


def mean_bwd(dy, inverse, n_unique):
    """Backward of the per-voxel mean: dx[i] = dy[inverse[i]] / count[inverse[i]]."""
    cnt = torch.bincount(inverse, minlength=n_unique).to(F64)
    return dy.to(F64)[inverse] / cnt[inverse][:, None]


# ------------------------------------------------------------------------------------------------ layers (differentiable)
def linear(x, w, b=None):
    y = x @ w.t()
    return y if b is None else y + b


def batch_norm(x, gamma, beta):
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return (x - mean) / torch.sqrt(var + BN_EPS) * gamma + beta


def leaky(x):
    return torch.where(x > 0, x, 0.01 * x)


def conv(x, coords, ts, w, k, s):
    """-> (y, out coordinates, out tensor stride): y[o] = sum_j x[table[o][j]] @ w[j] over the window of out[o]."""
    out = coords if s == 1 else PR.strided_coords(coords, ts, s)[0]
    table = PR.window_table(coords, out, ts, k)
    xp = torch.cat([x, torch.zeros(1, x.shape[1], dtype=F64)], 0)
    y = torch.einsum("okc,kcd->od", xp[table], w)
    return y, out, ts * s


def max_pool(x, coords, ts, k=3, s=2):
    out, table = PR.pooling_maps(coords, ts, k, s)
    xp = torch.cat([x, torch.full((1, x.shape[1]), -float("inf"), dtype=F64)], 0)
    assert int(PR.counts(table).min()) >= 1
    return xp[table].max(1).values, out, ts * s


def voxel_mean(F, inverse, n_unique):
    s = torch.zeros(n_unique, F.shape[1], dtype=F64).index_add(0, inverse, F)
    return s / torch.bincount(inverse, minlength=n_unique).to(F64)[:, None]


def global_max(x, off):
    return torch.stack([x[off[b]:off[b + 1]].max(0).values for b in range(len(off) - 1)])


def global_avg(x, off):
    return torch.stack([x[off[b]:off[b + 1]].mean(0) for b in range(len(off) - 1)])


def _mlp(p, name, x, act=leaky):
    return act(batch_norm(linear(x, p[name + ".0.linear.weight"]), p[name + ".1.bn.weight"], p[name + ".1.bn.bias"]))


def _conv_block(p, name, x, coords, ts, k, s):
    y, out, ts = conv(x, coords, ts, p[name + ".0.kernel"], k, s)
    return leaky(batch_norm(y, p[name + ".1.bn.weight"], p[name + ".1.bn.bias"])), out, ts


def fcnn_forward(p, coords, feats, kernel_size=3, splat=False):
    """Logits [B, classes] of MinkowskiFCNN (splat=False) / MinkowskiSplatFCNN (splat=True) in train mode, dropout off."""
    B = int(coords[:, 0].max()) + 1
    x = _mlp(p, "mlp1", feats.to(F64))
    vox, inv = quantise(coords)
    if splat:
        sc, imap, w = IR.splat_coords(coords)
        y, cur = IR.splat_fwd(x, imap, w, sc.shape[0]), sc
    else:
        y, cur = voxel_mean(x, inv, vox.shape[0]), vox
    ts, reads = 1, []
    for i, s in enumerate((1, 2, 2, 2), start=1):
        y, cur, ts = _conv_block(p, f"conv{i}", y, cur, ts, kernel_size, s)
        y, cur, ts = max_pool(y, cur, ts)
        if splat:
            im, wt = IR.map_weight(cur, ts, coords)
            reads.append(IR.interp_fwd(y, im, wt))
        else:
            reads.append(gather_fwd(y, field_map(coords, cur, ts)))
    y, cur, ts = voxel_mean(torch.cat(reads, 1), inv, vox.shape[0]), vox, 1
    for j in range(3):
        y, cur, ts = _conv_block(p, f"conv5.{j}", y, cur, ts, 3, 2)
    off = PR.offsets_of(cur, B)
    y = torch.cat([global_max(y, off), global_avg(y, off)], 1)
    y = _mlp(p, "final.3", _mlp(p, "final.1", y))
    return linear(y, p["final.4.linear.weight"], p["final.4.linear.bias"])


def pointnet_forward(p, coords, feats):
    """Logits [B, classes] of MinkowskiPointNet in train mode, dropout off."""
    B = int(coords[:, 0].max()) + 1
    x = feats.to(F64)
    for i in range(1, 6):
        x = _mlp(p, f"conv{i}", x, act=torch.relu)
    off = PR.offsets_of(coords, B)
    x = _mlp(p, "linear1", global_max(x, off), act=torch.relu)
    return linear(x, p["linear2.linear.weight"], p["linear2.linear.bias"])
