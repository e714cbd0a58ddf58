"""Fixed-size sub-sampling of a scene for the point networks (counterpart of the reference's `FarthestPointSample` and
`RandomSample`, co3d_3d/src/data/transforms.py:597-651; the gin names and the `num_points` argument are kept).

A PeRFception-CO3D scene has about 50 k voxels, far more than a k-nearest-neighbour graph or a PAConv layer is meant to see.
The reference cuts it down per scene on the CPU in the DataLoader worker; here a sampler, like the transforms of
data/transforms.py, only DRAWS there -- `plan(n_rows)` returns what the batch needs to carry -- and the rows are taken on the
device when the batch reaches the model (`MinkowskiBaseModel.process_input`: after the compact form has been decoded, before
the augmentation program), by `mink_fps_scenes` for the farthest-point sampler and by a plain row gather for the random one.
Both keep exactly `num_points` rows of every scene, so no survivor count has to come back to the host.

These classes have no `draw` method and are no stages of the augmentation program: a recipe names at most one of them, only
`DensityBasedSample` may stand before it (the plan is drawn over the rows that filter keeps), and every drawing stage follows
it -- the reference would otherwise sample transformed coordinates, and the fused augmentation pass cannot be split around a
sampler (`split_recipe`).

Not carried over: `LabelBasedSample` needs per-voxel labels, and `collate_pointnet` builds dense [B, m, .] batches that the
point networks here do not take (they read the scenes of a field through its batch offsets); `DataModule` keeps refusing it."""
import numpy as np

from nerf_downstream_amd import gin_lite as gin


@gin.configurable()
class FarthestPointSample:
    """Keep `num_points` rows by farthest-point sampling of the voxel coordinates, starting from a random row."""

    def __init__(self, num_points):
        self.num_points = int(num_points)
        if self.num_points < 1:
            raise ValueError(f"FarthestPointSample.num_points = {num_points}")

    def plan(self, n_rows):
        return {"fps_start": int(np.random.randint(0, n_rows)), "sample_points": self.num_points}


@gin.configurable()
class RandomSample:
    """Keep `num_points` rows drawn uniformly: without replacement only when the scene has more rows than that."""

    def __init__(self, num_points):
        self.num_points = int(num_points)
        if self.num_points < 1:
            raise ValueError(f"RandomSample.num_points = {num_points}")

    def plan(self, n_rows):
        ind = np.random.choice(n_rows, self.num_points, replace=n_rows <= self.num_points)
        return {"sample_rows": ind.astype(np.int64), "sample_points": self.num_points}


SAMPLERS = ("FarthestPointSample", "RandomSample")


def split_recipe(names, prefilters=("DensityBasedSample",)):
    """A recipe's names -> (the names left for the augmentation program, the sampler's name or None).  Raises
    NotImplementedError unless at most one sampler is named and nothing but row filters stands before it."""
    at = [i for i, t in enumerate(names) if t in SAMPLERS]
    if not at:
        return list(names), None
    rule = ("a recipe takes at most one of FarthestPointSample / RandomSample, only DensityBasedSample may stand before it and "
            "every other stage follows it")
    if len(at) > 1:
        raise NotImplementedError(f"{[names[i] for i in at]}: {rule}")
    i = at[0]
    early = [t for t in names[:i] if t not in prefilters]
    late = [t for t in names[i + 1:] if t in prefilters]
    if early or late:
        raise NotImplementedError(f"{early or late} {'before' if early else 'after'} {names[i]}: {rule}")
    return list(names[:i]) + list(names[i + 1:]), names[i]


def fps_numpy(xyz, offsets, num_points, start):
    """The farthest-point picks on the host (numpy float32, the arithmetic and the tie rule of `mink_fps_scenes`): global rows,
    int64 [B, num_points].  For the CPU backend of the trainer tests; the product samples on the device."""
    xyz = np.ascontiguousarray(np.asarray(xyz, dtype=np.float32)[:, :3])
    offsets, start = np.asarray(offsets, dtype=np.int64), np.asarray(start, dtype=np.int64).reshape(-1)
    out = np.empty((len(offsets) - 1, int(num_points)), dtype=np.int64)
    for b in range(len(offsets) - 1):
        p = xyz[offsets[b]:offsets[b + 1]]
        if len(p) == 0 or not 0 <= start[b] < len(p):
            raise ValueError(f"scene {b}: {len(p)} rows, first pick {start[b]}")
        dist, cur = np.full(len(p), 1e10, dtype=np.float32), int(start[b])
        for k in range(int(num_points)):
            out[b, k] = offsets[b] + cur
            d = p - p[cur]
            d = d * d
            d = (d[:, 0] + d[:, 1]) + d[:, 2]
            np.minimum(dist, d, out=dist, where=d < dist)
            cur = int(np.argmax(dist))
    return out
