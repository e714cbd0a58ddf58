"""Float64 restatement of the generative layers, written from their definitions (include/mink_hip.h, INTEGRATION.md "Generative
layers") and never calling the code under test: children generation, pruning (values, order, batch offsets, gradient),
occupancy, the generative product, and -- from oracle layers plus these -- the CompletionNet forward pass.

Shared by tests/test_generative_cpu.py, tests/test_gpu_generative.py and tests/test_gpu_guard_generative.py."""
import numpy as np
import torch


# ---------------------------------------------------------------------------------------------------------------- coordinates
def child_offsets(half):
    """[8, 3] int64: the offsets of a size-2 kernel at tensor stride `half`: {0, 1}^3 * half, x fastest, z slowest."""
    return np.array([[(k & 1), (k >> 1) & 1, (k >> 2) & 1] for k in range(8)], np.int64) * int(half)


def children(coords, ts):
    """coords int [n, 4] = (b, x, y, z) at the even tensor stride ts -> int32 [8 n, 4], row 8 p + k = parent p + offset k."""
    coords = np.asarray(coords, np.int64)
    assert ts % 2 == 0 and (coords[:, 1:] % ts == 0).all()
    out = np.repeat(coords, 8, axis=0)
    out[:, 1:] += np.tile(child_offsets(ts // 2), (coords.shape[0], 1))
    return out.astype(np.int32)


def batch_offsets(coords, B):
    """int32 [B + 1]: rows of sample b are [off[b], off[b + 1]) (batch column non-decreasing; a sample may have none)."""
    b = np.asarray(coords)[:, 0]
    return np.searchsorted(b, np.arange(B + 1), side="left").astype(np.int32)


def random_parents(rng, n, ts, B, lo=-6, hi=6, top=False):
    """n distinct voxels at tensor stride ts spread over B samples (every sample gets at least one when n >= B), batch column
    non-decreasing, negative coordinates included; `top`: the last one sits at the top of the 16-bit key range."""
    side = hi - lo
    assert side ** 3 >= n
    r = rng.choice(side ** 3, size=n, replace=False)  # distinct positions: distinct rows whatever their sample
    b = np.sort(np.concatenate([np.arange(min(B, n)), rng.integers(0, B, size=max(n - B, 0))]))
    c = np.stack([b, lo + r % side, lo + (r // side) % side, lo + r // side ** 2], 1).astype(np.int64)
    c[:, 1:] *= ts
    if top:
        edge = (32767 // ts) * ts  # the largest multiple of ts in range: its children reach edge + ts / 2 <= 32767
        c[-1, 1:] = (edge, -32768 // ts * ts + 0, edge)
    return c.astype(np.int32)


def occupancy(out_coords, target_coords, ts):
    """bool [n]: is out_coords[i] a voxel of the target's map at tensor stride ts (= its coordinates floored to multiples of ts)?"""
    t = np.asarray(target_coords, np.int64).copy()
    t[:, 1:] = np.floor_divide(t[:, 1:], ts) * ts
    have = set(map(tuple, t.tolist()))
    return np.array([tuple(r) in have for r in np.asarray(out_coords, np.int64).tolist()], bool)


# -------------------------------------------------------------------------------------------------------------------- pruning
def prune(feats, coords, mask, B):
    """-> (kept features, kept coordinates, batch offsets [B + 1], kept rows, old row -> new row or -1): stable."""
    mask = np.asarray(mask, bool)
    kept = np.nonzero(mask)[0]
    old2new = np.full(mask.shape[0], -1, np.int64)
    old2new[kept] = np.arange(kept.shape[0])
    c = np.asarray(coords)[kept]
    return feats[torch.from_numpy(kept)], c, batch_offsets(c, B), kept.astype(np.int32), old2new.astype(np.int32)


def prune_grad(g_out, mask):
    """dX [n, C]: kept rows receive their gradient row, pruned rows zeros."""
    mask = torch.as_tensor(np.asarray(mask, bool))
    dx = torch.zeros(mask.shape[0], g_out.shape[1], dtype=g_out.dtype)
    dx[mask] = g_out
    return dx


# --------------------------------------------------------------------------------------------------------- generative product
def gen_product(x, kernel, bias=None):
    """out[8 p + k] = x[p] @ kernel[k] (+ bias): x [n, Cin], kernel [8, Cin, Cout] -> [8 n, Cout] (differentiable)."""
    out = torch.einsum("pi,kio->pko", x, kernel).reshape(8 * x.shape[0], kernel.shape[2])
    return out if bias is None else out + bias


# ------------------------------------------------------------------------------------------------------------ the whole model
def derived_tensor(OME, feats, coords, ts):
    """An oracle SparseTensor whose map is `coords` at tensor stride ts, on a manager of its own."""
    cm = OME.CoordinateManager()
    cm.coords[ts] = np.ascontiguousarray(coords, np.int32)
    return OME.SparseTensor(feats, OME.CoordinateMapKey(ts), cm)


class _GenUp(torch.nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.kernel = torch.nn.Parameter(torch.zeros(8, cin, cout))

    def forward(self, OME, x):
        ts = x.coordinate_map_key.ts
        return derived_tensor(OME, gen_product(x.F, self.kernel), children(x.C.numpy(), ts), ts // 2)


class _RefBlock(torch.nn.Module):
    def __init__(self, OME, cin, cout):
        super().__init__()
        self.up = _GenUp(cin, cout)
        self.bn1, self.bn2 = OME.MinkowskiBatchNorm(cout), OME.MinkowskiBatchNorm(cout)
        self.conv = OME.MinkowskiConvolution(cout, cout, kernel_size=3, stride=1, dimension=3)
        self.cls = OME.MinkowskiConvolution(cout, 1, kernel_size=1, stride=1, bias=True, dimension=3)


class RefCompletion(torch.nn.Module):
    """CompletionNet (models/mink/completion.py) from oracle layers and the restatements above; same parameter names, so
    `load_state_dict(model.state_dict())` carries the weights over.  forward -> [(logits [n, 1], occupancy bool [n], generated
    coordinates int32 [n, 4], logits > 0 bool [n])] per decoder block, and the final (features, coordinates)."""

    def __init__(self, OME, in_channel, channels=(16, 32)):
        super().__init__()
        self.OME = OME
        c1, c2 = channels
        self.enc1 = OME.MinkowskiConvolution(in_channel, c1, kernel_size=3, stride=2, dimension=3)
        self.enc_bn1 = OME.MinkowskiBatchNorm(c1)
        self.enc2 = OME.MinkowskiConvolution(c1, c2, kernel_size=3, stride=2, dimension=3)
        self.enc_bn2 = OME.MinkowskiBatchNorm(c2)
        self.dec1, self.dec2 = _RefBlock(OME, c2, c1), _RefBlock(OME, c1, c1)

    def forward(self, x, target_coords=None):
        OME, relu = self.OME, self.OME.MinkowskiReLU()
        y = relu(self.enc_bn1(self.enc1(x)))
        y = relu(self.enc_bn2(self.enc2(y)))
        levels = []
        for blk in (self.dec1, self.dec2):
            y = relu(blk.bn1(blk.up(OME, y)))
            y = relu(blk.bn2(blk.conv(y)))
            logits = blk.cls(y)
            ts, c = y.coordinate_map_key.ts, y.C.numpy()
            pred = (logits.F.detach()[:, 0] > 0).numpy()
            if target_coords is None:  # no target: the classifier decides
                occ, keep = None, pred
            else:
                occ = occupancy(c, target_coords, ts)
                keep = occ | pred if self.training else occ
            levels.append((logits.F, occ, c, pred))
            y = derived_tensor(OME, y.F[torch.from_numpy(np.nonzero(keep)[0])], c[keep], ts)
        return levels, (y.F, y.C.numpy())
