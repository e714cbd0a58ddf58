"""ModelNet40 point clouds, 2,048 points per shape (counterpart of the reference's co3d_3d/src/data/modelnet40.py:28-88).

A sample is {"coordinates": xyz / voxel_size, "features": xyz, "labels": [class]} -- continuous coordinates, so several
points may share a voxel and `TensorField.sparse()` averages their features.  The shards are the files of
modelnet40_ply_hdf5_2048: `ply_data_<phase>*.h5` with the arrays `data` [M, P, 3] float and `label` [M, 1], read with
h5py; a directory may instead hold `ply_data_<phase>*.npz` shards with the same two arrays (numpy only).  Nothing is
ever downloaded and no process is started: a missing directory is an error.

The three train-time transforms of the recipe (CoordinateUniformTranslation, RandomScale, CoordinateDropout) act on the
raw xyz of one shape, before coordinates and features are derived from it, so they are applied here, on the host, from
the stages the transform classes draw (transforms.Compose.draw) -- the batch-level GPU program transforms voxel
coordinates beside plenoxel feature columns and does not apply to a sample whose features ARE its coordinates."""
import glob
import os

import numpy as np
from torch.utils.data import Dataset

from nerf_downstream_amd import gin_lite as gin

from . import transforms


def apply_stages(xyz, stages):
    """One shape's drawn stage list applied to xyz [P, 3] in order, as the reference's transforms do (transforms.py:247-293,
    361-372): ("linear", M) xyz @ M | ("translate", t) xyz + t | ("dropout", r) a random subset of int(P * (1 - r)) rows."""
    for s in stages:
        if s[0] == "linear":
            xyz = xyz @ np.asarray(s[1], xyz.dtype).reshape(3, 3)
        elif s[0] == "translate":
            xyz = xyz + np.asarray(s[1], xyz.dtype).reshape(1, 3)
        elif s[0] == "dropout":
            n = len(xyz)
            xyz = xyz[np.random.choice(n, int(n * (1 - s[1])), replace=False)]
        else:
            raise NotImplementedError(f"ModelNet40H5Dataset: the augmentation stage {s[0]!r} has no per-sample host form "
                                      "(CoordinateUniformTranslation, RandomScale and CoordinateDropout have)")
    return xyz


@gin.configurable
class ModelNet40H5Dataset(Dataset):
    def __init__(self, phase, data_root="modelnet40h5", train_transformations=("CoordinateUniformTranslation",),
                 eval_transformations=(), num_points=2048, voxel_size=0.05, download=False):
        super().__init__()
        if download:
            raise NotImplementedError("ModelNet40H5Dataset never downloads: unpack modelnet40_ply_hdf5_2048 under data_root")
        phase = "test" if phase in ("val", "test") else "train"
        self.data, self.label = self.load_data(data_root, phase)
        names = train_transformations if phase == "train" else eval_transformations
        self.transformations = transforms.Compose([getattr(transforms, t)() for t in names]) if len(names) > 0 else None
        self.phase, self.voxel_size, self.num_points = phase, voxel_size, num_points

    @staticmethod
    def load_data(data_root, phase):
        if not os.path.isdir(data_root):
            raise FileNotFoundError(f"ModelNet40H5Dataset: data_root {data_root!r} does not exist (the dataset is never downloaded)")
        h5 = sorted(glob.glob(os.path.join(data_root, f"ply_data_{phase}*.h5")))
        npz = sorted(glob.glob(os.path.join(data_root, f"ply_data_{phase}*.npz")))
        data, labels = [], []
        if npz:
            for name in npz:
                with np.load(name) as f:
                    data.append(f["data"].astype("float32"))
                    labels.append(f["label"].astype("int64"))
        elif h5:
            try:
                import h5py
            except ImportError:
                raise ImportError(f"ModelNet40H5Dataset: {len(h5)} ply_data_{phase}*.h5 shards under {data_root!r} need h5py, which is "
                                  f"not installed; alternatively convert them to ply_data_{phase}*.npz shards holding the same two "
                                  "arrays, data [M, P, 3] and label [M, 1]") from None
            for name in h5:
                with h5py.File(name, "r") as f:
                    data.append(f["data"][:].astype("float32"))
                    labels.append(f["label"][:].astype("int64"))
        else:
            raise FileNotFoundError(f"ModelNet40H5Dataset: no ply_data_{phase}*.h5 or ply_data_{phase}*.npz shards under {data_root!r}")
        return np.concatenate(data, 0), np.concatenate(labels, 0).reshape(-1, 1)

    def __getitem__(self, i):
        xyz = self.data[i]
        if 0 < self.num_points < len(xyz):
            xyz = xyz[: self.num_points]
        if self.transformations is not None:
            xyz = apply_stages(xyz, self.transformations.draw())
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        return {"coordinates": xyz / self.voxel_size, "features": xyz, "labels": self.label[i]}

    def __len__(self):
        return self.data.shape[0]

    def __repr__(self):
        return f"{type(self).__name__}(phase={self.phase}, length={len(self)}, transform={self.transformations})"
