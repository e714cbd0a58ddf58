"""Restatement of farthest-point sampling in numpy float32 (include/mink_hip.h, mink_fps_scenes; reference transforms.py:603-626),
one operation at a time in the stated order, for tests/test_sampling_cpu.py and the GPU suites:

    dist[i] = 1e10;  cur = start
    m times:  emit cur;  d = ((dx dx) + (dy dy)) + (dz dz), every difference, product and sum an np.float32 operation of its own;
              dist[i] = d where d < dist[i];  cur = the first index of the largest dist (np.argmax, as torch.argmax)."""
import numpy as np

F = np.float32


def fps_scene(xyz, m, start):
    """xyz [n, >= 3] (columns 0..2 are read) -> int64 [m], scene-local rows in pick order."""
    p = np.asarray(xyz, dtype=F)
    x, y, z = (np.ascontiguousarray(p[:, c]) for c in range(3))
    n = len(p)
    assert n >= 1 and 0 <= start < n
    dist = np.full(n, 1e10, dtype=F)
    out = np.empty(m, dtype=np.int64)
    cur = int(start)
    for k in range(m):
        out[k] = cur
        dx, dy, dz = np.subtract(x, x[cur], dtype=F), np.subtract(y, y[cur], dtype=F), np.subtract(z, z[cur], dtype=F)
        xx, yy, zz = np.multiply(dx, dx, dtype=F), np.multiply(dy, dy, dtype=F), np.multiply(dz, dz, dtype=F)
        d = np.add(np.add(xx, yy, dtype=F), zz, dtype=F)
        closer = d < dist
        dist[closer] = d[closer]
        cur = int(np.argmax(dist))
    return out


def fps_batch(xyz, offsets, m, start):
    """The picks of every scene as GLOBAL rows: int64 [B, m]."""
    offsets = [int(o) for o in offsets]
    return np.stack([offsets[b] + fps_scene(np.asarray(xyz)[offsets[b]:offsets[b + 1]], m, int(start[b]))
                     for b in range(len(offsets) - 1)])
