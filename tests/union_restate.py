"""Restatement of the union of sparse tensors, written from its definition (include/mink_hip.h "union of tensors on different
maps", INTEGRATION.md "Generative layers") and never calling the code under test: the union order through a Python dict of
coordinate tuples, in2out / out2in / batch offsets, the sum in numpy float32 added in ascending input order from a copy of the
first present row, the gradient, and -- from oracle layers, tests/gen_restate.py and these -- the CompletionUNet forward pass.

Fixed-order IEEE fp32 addition involves no multiplication, so nothing can be contracted: the GPU result must equal `union_sum`
bit for bit.

Shared by tests/test_union_cpu.py, tests/test_gpu_union.py and tests/test_gpu_guard_union.py."""
import numpy as np
import torch

import gen_restate as R


# ------------------------------------------------------------------------------------------------------------------- the map
def union_map(coord_lists, B):
    """coord_lists: k int arrays [n_i, 4] = (b, x, y, z), unique rows each, batch column non-decreasing ->
    (coordinates int32 [N, 4], in2out: k int32 [n_i], out2in int32 [k, N] with -1 = absent, batch offsets int32 [B + 1]).
    Order: sample-major; inside a sample the rows of input 0 in their order, then the rows of input 1 that no earlier input
    holds, in their order, and so on."""
    lists = [np.asarray(c, np.int64) for c in coord_lists]
    row_of, out = {}, []
    in2out = [np.full(c.shape[0], -1, np.int32) for c in lists]
    for b in range(B):
        for i, c in enumerate(lists):
            for r in np.nonzero(c[:, 0] == b)[0].tolist():
                key = tuple(c[r].tolist())
                if key not in row_of:
                    row_of[key] = len(out)
                    out.append(key)
                in2out[i][r] = row_of[key]
    assert all((m >= 0).all() for m in in2out), "a batch index outside [0, B)"
    out2in = np.full((len(lists), len(out)), -1, np.int32)
    for i, m in enumerate(in2out):
        out2in[i, m] = np.arange(m.shape[0], dtype=np.int32)
    coords = np.array(out, np.int32).reshape(-1, 4)
    return coords, in2out, out2in, R.batch_offsets(coords, B)


# ------------------------------------------------------------------------------------------------------------------- the sum
def union_sum(feats, out2in):
    """feats: k float32 arrays [n_i, C] -> float32 [N, C]: per union row the first present input's row COPIED, the later present
    ones added to it in ascending input index, in float32."""
    feats = [np.asarray(f, np.float32) for f in feats]
    N, C = out2in.shape[1], feats[0].shape[1]
    y = np.zeros((N, C), np.float32)
    seen = np.zeros(N, bool)
    for f, rows in zip(feats, out2in):
        have = rows >= 0
        first, later = have & ~seen, have & seen
        y[first] = f[rows[first]]
        y[later] = y[later] + f[rows[later]]  # one float32 addition per element
        seen |= have
    assert seen.all()
    return y


def union_grad(g, in2out):
    """The gradient of every input: dx_i[r] = g[in2out[i][r]]."""
    g = np.asarray(g)
    return [g[m] for m in in2out]


# ------------------------------------------------------------------------------------------------------------ the whole model
class _Union(torch.nn.Module):
    """The union of oracle tensors, differentiable (float64: the order of the additions is of no account here)."""

    def forward(self, OME, B, *xs):
        ts = xs[0].coordinate_map_key.ts
        coords, in2out, _, _ = union_map([x.C.numpy() for x in xs], B)
        out = torch.zeros(coords.shape[0], xs[0].F.shape[1], dtype=xs[0].F.dtype)
        for x, rows in zip(xs, in2out):
            out = out.index_add(0, torch.from_numpy(rows.astype(np.int64)), x.F)
        return R.derived_tensor(OME, out, coords, ts)


class RefCompletionUNet(torch.nn.Module):
    """CompletionUNet (models/mink/completion.py) from oracle layers, tests/gen_restate.py and the restatements above; same
    parameter names, so `load_state_dict(model.state_dict())` carries the weights over.  forward -> [(logits [n, 1], occupancy
    bool [n] or None, coordinates int32 [n, 4] of the level (the union), logits > 0 bool [n], (rows the decoder generated, rows
    of the skip, rows of their union))] per decoder block, and the final (features, coordinates).  `skip=False`: every block
    goes on with the decoder tensor alone -- what the net would be if the union were a no-op."""

    def __init__(self, OME, in_channel, channels=(16, 16, 32, 64), skip=True):
        super().__init__()
        self.OME, self.skip = OME, skip
        c0, c1, c2, c3 = channels
        self.stem = OME.MinkowskiConvolution(in_channel, c0, kernel_size=3, stride=1, dimension=3)
        self.stem_bn = OME.MinkowskiBatchNorm(c0)
        self.enc1 = OME.MinkowskiConvolution(c0, c1, kernel_size=3, stride=2, dimension=3)
        self.enc_bn1 = OME.MinkowskiBatchNorm(c1)
        self.enc2 = OME.MinkowskiConvolution(c1, c2, kernel_size=3, stride=2, dimension=3)
        self.enc_bn2 = OME.MinkowskiBatchNorm(c2)
        self.enc3 = OME.MinkowskiConvolution(c2, c3, kernel_size=3, stride=2, dimension=3)
        self.enc_bn3 = OME.MinkowskiBatchNorm(c3)
        self.dec1, self.dec2, self.dec3 = R._RefBlock(OME, c3, c2), R._RefBlock(OME, c2, c1), R._RefBlock(OME, c1, c0)
        self.union = _Union()

    def forward(self, x, target_coords=None):
        OME, relu = self.OME, self.OME.MinkowskiReLU()
        B = int(x.C[:, 0].max()) + 1
        s1 = relu(self.stem_bn(self.stem(x)))
        s2 = relu(self.enc_bn1(self.enc1(s1)))
        s4 = relu(self.enc_bn2(self.enc2(s2)))
        y = relu(self.enc_bn3(self.enc3(s4)))
        levels = []
        for blk, skip in ((self.dec1, s4), (self.dec2, s2), (self.dec3, s1)):
            y = relu(blk.bn1(blk.up(OME, y)))
            n_dec = y.F.shape[0]
            if self.skip:
                y = self.union(OME, B, y, skip)
            y = relu(blk.bn2(blk.conv(y)))
            logits = blk.cls(y)
            ts, c = y.coordinate_map_key.ts, y.C.numpy()
            pred = (logits.F.detach()[:, 0] > 0).numpy()
            if target_coords is None:  # no target: the classifier decides
                occ, keep = None, pred
            else:
                occ = R.occupancy(c, target_coords, ts)
                keep = occ | pred if self.training else occ
            levels.append((logits.F, occ, c, pred, (n_dec, skip.F.shape[0], c.shape[0])))
            y = R.derived_tensor(OME, y.F[torch.from_numpy(np.nonzero(keep)[0])], c[keep], ts)
        return levels, (y.F, y.C.numpy())


# ------------------------------------------------------------------------------------------------------------------ the cases
def related_lists(rng, relation, n, k, B, ts, edges=False):
    """k coordinate lists of about n rows each at tensor stride ts over B samples, related as `relation` says:
      disjoint  : no voxel in two lists          identical : every list the same rows
      contained : list i + 1 is every other row of list i (list 0 holds them all)
      partial   : neighbouring lists share about half of their rows
      twice     : list 1 IS list 0 (one input given twice), the others partial
      lonely    : sample B - 1 is held by list 0 alone (B >= 2)
      emptied   : the middle sample of three is empty in every list
    Every list keeps at least one row.  `edges`: list 0 also holds voxels at both ends of the 16-bit key range."""
    side = 22
    pool_n = max(2 * n * k, 8)
    assert side ** 3 >= pool_n
    cells = rng.choice(side ** 3, size=pool_n, replace=False)  # distinct positions: distinct rows whatever their sample
    pool = np.stack([rng.integers(0, B, size=pool_n), cells % side - 11, (cells // side) % side - 11, cells // side ** 2 - 11], 1)
    pool[:, 1:] *= ts
    pool[:B, 0] = np.arange(B)
    if relation == "emptied":
        assert B == 3
        pool = pool[pool[:, 0] != 1]
    pick = []
    for i in range(k):
        if relation == "disjoint":
            rows = pool[i * n : (i + 1) * n]
        elif relation == "identical":
            rows = pool[:n]
        elif relation == "contained":
            rows = pool[:n][:: 2 ** i]
        else:  # partial overlap with the neighbour: windows of n rows that advance by n / 2 (by one row at least)
            step = max(n // 2, 1)
            rows = pool[i * step : i * step + n]
        pick.append(rows)
    if relation == "lonely":
        assert B >= 2
        pick = [p if i == 0 else p[p[:, 0] != B - 1] for i, p in enumerate(pick)]
        pick[0] = np.concatenate([pick[0], [[B - 1, 20 * ts, 0, 0]]])  # list 0 really holds that sample
    if edges:
        top, bottom = (32767 // ts) * ts, -(32768 // ts) * ts
        pick[0] = np.concatenate([pick[0], [[0, top, bottom, top], [B - 1, bottom, top, bottom]]])
    if relation == "twice":
        pick[1] = pick[0]
    if relation == "identical":
        pick = [pick[0].copy() for _ in range(k)]
    out, made = [], {}
    for p in pick:
        if id(p) not in made:  # (one input given twice stays ONE array)
            q = p if p.shape[0] else pool[:1]
            q = q[np.argsort(q[:, 0], kind="stable")]  # batch column non-decreasing, the order inside a sample kept
            made[id(p)] = np.ascontiguousarray(q, np.int32)
        out.append(made[id(p)])
    return out
