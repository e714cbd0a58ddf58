"""PeRFception-ScanNet plenoxel dataset for the segmentation family (counterpart of the reference's
`PlenoxelScannetDataset`, co3d_3d/src/data/scannet.py:450-660; Res16UNet is trained on it by
configs/scannet_plenoxel.gin).

Scene directory `<data_root>/plenoxel_torch_<scene>/data.npz`:
    links int [N] flat index into the `reso` grid, density f32 [N,1], sh uint8 [N,27] (* sh_scale + sh_min),
    reso int [3], labels int [N] (ScanNet-40 ids), dists f32 [N] (distance of the voxel to the labelled mesh)
`<dirname(data_root)>/split/scannet_256_{train,val}.txt` list the scenes, `split/scene_scales.data` (pickle) holds the
scale of every scene.  A sample, as in the reference (:585-653):

* voxels farther than `valid_thres` from the mesh get `void_label`; with `ignore_thres` the ones beyond it are dropped;
* `downsample_mode = 1` keeps the voxels whose grid coordinates are multiples of `downsample_stride`;
* coordinates = ((grid / reso) * 2 - 1) / scene_scale / voxel_size  -- metric voxels of `voxel_size`, NOT integers:
  `TensorField.sparse()` floors them and averages the features that share a voxel, `out.slice(field)` carries the
  prediction back to every input row (models/mink/res16unet.py);
* features selected by name from [dists | density (max-normalised when more than one feature) | sh | ones];
* labels mapped from the 40 raw ids to the 20 evaluated classes, everything else to `ignore_label`.

Augmentations (extension `device_augmentation=True`): the reference's recipe for this data set (RandomRotation,
RandomCrop, RandomAffine, CoordinateDropout, RandomFeatureJitter, RandomHorizontalFlip, RandomTranslation,
ElasticDistortion; data/seg_transforms.py) is drawn here, one program per scene with the scene's raw extent, and applied
to the whole batch on the GPU (`MinkowskiBaseModel.process_input`, `mink_augment_seg_scenes`); the training step gathers
the labels of the surviving rows.  Without it only an empty transformation list is accepted."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from nerf_downstream_amd import gin_lite as gin
from nerf_downstream_amd.safe_load import load_plain_pickle

from . import seg_transforms
from .ply import load_ply

CLASS_LABELS = ("wall", "floor", "cabinet", "bed", "chair", "sofa", "table", "door", "window", "bookshelf", "picture", "counter",
                "desk", "curtain", "refrigerator", "shower curtain", "toilet", "sink", "bathtub", "otherfurniture")
VALID_CLASS_IDS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 14, 16, 24, 28, 33, 34, 36, 39)


@gin.configurable
class PlenoxelScannetDataset(Dataset):
    NUM_LABELS = 41  # raw ids; mapped onto the 20 evaluated classes
    IGNORE_LABELS = tuple(set(range(NUM_LABELS)) - set(VALID_CLASS_IDS))
    DATA_PATH_FILE = {"train": "scannet_256_train.txt", "val": "scannet_256_val.txt", "test": "scannet_256_val.txt"}
    CLASS_LABELS = CLASS_LABELS
    VALID_CLASS_IDS = VALID_CLASS_IDS

    def __init__(self, phase, data_root="co3d_3d/datasets/co3d", train_transformations=(), eval_transformations=(),
                 downsample_mode=1, downsample_stride=2, voxel_size=0.02, num_points=-1, features=("sh",), ignore_label=-100,
                 void_label=None, valid_thres=0.05, ignore_thres=None, device_augmentation=False):
        phase = "test" if phase in ("val", "test") else "train"
        names = list(train_transformations if phase == "train" else eval_transformations)
        self.transformations = None
        if names and not device_augmentation:
            raise NotImplementedError(f"augmentations {names} of the ScanNet recipe run on the CPU in the reference and are "
                                      "outside the scope of this path: pass an empty transformation list (or "
                                      "device_augmentation=True to run them on the GPU)")
        if names:
            unknown = [t for t in names if t not in seg_transforms.SUPPORTED]
            if unknown:
                raise NotImplementedError(f"augmentations {unknown} have no GPU counterpart (supported: the classes of "
                                          "data/seg_transforms.py)")
            if "xyzs" in features:
                raise NotImplementedError("the 'xyzs' feature of an augmented scene is its transformed coordinates (reference "
                                          "scannet.py:633-640): not produced by the device program")
            self.transformations = seg_transforms.SegCompose([getattr(seg_transforms, t)() for t in names])
        if downsample_mode != 1:
            raise NotImplementedError("downsample_mode 0 (average pooling in the loader) is not implemented; mode 1 sub-samples")
        self.phase, self.data_root, self.features = phase, data_root, list(features)
        self.voxel_size, self.ignore_label = voxel_size, ignore_label
        self.void_label = void_label if void_label is not None else ignore_label
        self.valid_thres, self.ignore_thres, self.downsample_stride = valid_thres, ignore_thres, downsample_stride
        split = os.path.join(os.path.dirname(self.data_root), "split")
        with open(os.path.join(split, self.DATA_PATH_FILE[phase])) as f:
            self.files = [line.strip("\n") for line in f if line.strip() and not line.startswith("#")]
        label_map, n_used = {}, 0
        for raw in range(self.NUM_LABELS):
            if raw in self.IGNORE_LABELS:
                label_map[raw] = ignore_label
            else:
                label_map[raw] = n_used
                n_used += 1
        label_map[ignore_label] = ignore_label
        if void_label is not None and void_label != ignore_label:
            label_map[void_label] = n_used
        self.label_map = label_map
        self._lut = np.full(self.NUM_LABELS, ignore_label, dtype=np.int64)
        for raw, v in label_map.items():
            if 0 <= raw < self.NUM_LABELS:
                self._lut[raw] = v
        self.scene_scales = load_plain_pickle(os.path.join(split, "scene_scales.data"))  # {scene: scale}: plain data only
        self.NUM_CLASSES = len(self.CLASS_LABELS)

    def load_data(self, inst_id):
        z = np.load(os.path.join(self.data_root, f"plenoxel_torch_{inst_id}", "data.npz"))
        links = z["links"].astype(np.int64)
        density = z["density"].astype(np.float32).reshape(-1, 1)
        sh = z["sh"].astype(np.float32) * z["sh_scale"] + z["sh_min"]
        labels = z["labels"].astype(np.int64).reshape(-1, 1).copy()
        dists = z["dists"].astype(np.float32).reshape(-1, 1)
        labels[dists > self.valid_thres] = self.void_label
        if self.ignore_thres is not None and self.ignore_thres > 0:
            valid = (dists < self.ignore_thres).reshape(-1)
            links, sh, density, labels = links[valid], sh[valid], density[valid], labels[valid]
            # (the reference keeps `dists` unfiltered here, scannet.py:577-583, which only works when nothing is dropped)
            dists = dists[valid]
        return links, density, sh.reshape(len(links), -1).astype(np.float32), np.asarray(z["reso"]).astype(np.int64), labels, dists

    def __getitem__(self, index):
        inst_id = self.files[index]
        links, density, sh, reso, labels, dists = self.load_data(inst_id)
        grid = np.stack([links // (reso[1] * reso[2]), links % (reso[1] * reso[2]) // reso[2], links % reso[2]], 1).astype(np.float32)
        if len(self.features) > 1:
            density = density / (np.abs(density).max() + 1e-5)
        sel = (grid % self.downsample_stride == 0).all(axis=1)  # downsample_mode 1
        grid, dists, density, sh, labels = grid[sel], dists[sel], density[sel], sh[sel], labels[sel]
        xyzs = ((grid / reso.astype(np.float32) * 2 - 1.0) / np.float32(self.scene_scales[inst_id]) / np.float32(self.voxel_size)).astype(np.float32)
        cols = {"xyzs": xyzs, "dists": dists, "density": density.astype(np.float32), "sh": sh, "ones": np.ones_like(density, dtype=np.float32)}
        features = np.concatenate([cols[f] for f in self.features], axis=1).astype(np.float32)
        raw = labels.reshape(-1)
        mapped = np.where((raw >= 0) & (raw < self.NUM_LABELS), self._lut[np.clip(raw, 0, self.NUM_LABELS - 1)],
                          np.where(raw == self.void_label, self.label_map.get(self.void_label, self.ignore_label), self.ignore_label))
        sample = {"coordinates": torch.from_numpy(xyzs), "features": torch.from_numpy(features), "xyzs": torch.from_numpy(xyzs),
                  "labels": mapped.astype(np.int64), "dists": dists.reshape(-1, 1), "metadata": {"file": inst_id}}
        if self.transformations is not None:  # drawn here (DataLoader worker), applied on the GPU
            extent = (xyzs.max(0) - xyzs.min(0)).astype(np.float64) if len(xyzs) else np.zeros(3)
            params, stream = self.transformations.sample(extent)
            sample["aug_params"], sample["aug_stream"] = torch.from_numpy(params), stream
            sample["feature_names"] = tuple(self.features)
        return sample

    def __len__(self):
        return len(self.files)

    def __repr__(self):
        return f"{self.__class__.__name__}(phase={self.phase}, length={len(self)})"


@gin.configurable
class ScannetDataset(Dataset):
    """The original ScanNet point clouds (counterpart of the reference's `ScannetDataset`, co3d_3d/src/data/scannet.py:149-275;
    configs/scannet_semseg.gin).  `<data_root>/<DATA_PATH_FILE[phase]>` lists the scenes; each entry names a PLY file under
    `data_root`, with or without its `.ply` extension (data/ply.py reads it: x y z, red green blue, label).

    The loader only reads and draws.  Each sample carries the raw points (coordinates = xyz in metres, features = colours
    0..255, labels = raw ids), one down-sampling row (MINK_VOXDS_*: quantisation size, voxel size, ignore label), the
    raw-label -> class table, and the drawn programs: the geometric one (MINK_SEGAUG_*) and the colour one
    (MINK_COLORAUG_*).  `MinkowskiBaseModel.process_input` then runs on the GPU, per scene, what the reference runs in the
    loader: ME.utils.sparse_quantize(xyz, colours, labels, quantization_size=downsample_voxel_size) with label voting,
    coordinates = xyz[representative] / voxel_size, the recipe, and the map of the voted labels onto the 20 classes; the
    field carries the labels of its rows."""

    NUM_LABELS = PlenoxelScannetDataset.NUM_LABELS
    IGNORE_LABELS = PlenoxelScannetDataset.IGNORE_LABELS
    # (the reference's point-cloud split files, read from data_root itself: not the 256-scene plenoxel subset)
    DATA_PATH_FILE = {"train": "scannetv2_train.txt", "val": "scannetv2_val.txt", "test": "scannetv2_test.txt"}
    CLASS_LABELS = CLASS_LABELS
    VALID_CLASS_IDS = VALID_CLASS_IDS

    def __init__(self, phase, data_root="datasets/scannet", downsample_voxel_size=None, voxel_size=0.02,
                 train_transformations=("ChromaticTranslation", "ChromaticJitter", "CoordinateDropout", "RandomHorizontalFlip",
                                        "RandomAffine", "RandomTranslation", "NormalizeColor"),
                 eval_transformations=("NormalizeColor",), ignore_label=-100, features=("colors",)):
        self.phase, self.data_root, self.ignore_label = phase, data_root, ignore_label
        self.features = list(features)
        if self.features != ["colors"]:
            if "xyzs" in self.features:
                raise NotImplementedError("the 'xyzs' feature of an augmented scene is its transformed coordinates: not produced "
                                          "by the device program")
            raise NotImplementedError(f"features {self.features}: the point clouds provide ['colors']")
        names = list(train_transformations if phase == "train" else eval_transformations)
        if "RandomFeatureJitter" in names:
            raise NotImplementedError("RandomFeatureJitter on point-cloud colours is not part of the device program")
        self.transformations = seg_transforms.PointCompose([_transform(t) for t in names]) if names else None
        if downsample_voxel_size is None:
            downsample_voxel_size = voxel_size / 2
        self.downsample_voxel_size, self.voxel_size = downsample_voxel_size, voxel_size
        with open(os.path.join(self.data_root, self.DATA_PATH_FILE[phase])) as f:
            self.files = [line.strip() for line in f if line.strip() and not line.startswith("#")]
        label_map, lut = _label_map(self, ignore_label)
        self.label_map, self._lut = label_map, lut
        self.NUM_CLASSES = len(self.CLASS_LABELS)

    def path(self, entry):
        p = os.path.join(self.data_root, entry)
        if not os.path.exists(p) and not entry.endswith(".ply") and os.path.exists(p + ".ply"):
            p += ".ply"
        return p

    def __getitem__(self, index):
        xyz, colors, labels = load_ply(self.path(self.files[index]))
        ds = np.zeros(4, np.float64)  # MINK_VOXDS_*
        ds[0], ds[1], ds[2] = max(float(self.downsample_voxel_size), 0.0), self.voxel_size, self.ignore_label
        sample = {"coordinates": torch.from_numpy(xyz), "features": torch.from_numpy(colors), "labels": labels.astype(np.int64),
                  "ds_params": torch.from_numpy(ds), "class_lut": torch.from_numpy(self._lut), "metadata": {"file": self.files[index]},
                  "dataset": "scannet", "feature_names": tuple(self.features)}
        if self.transformations is not None:  # drawn here (DataLoader worker), applied on the GPU
            extent = ((xyz.max(0) - xyz.min(0)).astype(np.float64) / self.voxel_size) if len(xyz) else np.zeros(3)
            geo, col, stream = self.transformations.sample(extent)
            if geo is not None:
                sample["aug_params"] = torch.from_numpy(geo)
            if col is not None:
                sample["color_params"] = torch.from_numpy(col)
            sample["aug_stream"] = stream
        return sample

    def __len__(self):
        return len(self.files)

    def __repr__(self):
        return f"{self.__class__.__name__}(phase={self.phase}, length={len(self)})"


def _transform(name):
    cls = getattr(seg_transforms, name, None)
    if cls is None or not (isinstance(cls, type) and (cls in seg_transforms.COLOR_STAGES or name in seg_transforms.SUPPORTED)):
        if name in seg_transforms.UNSUPPORTED_COLOR:
            raise NotImplementedError(f"colour stage {name} has no device counterpart (supported: "
                                      f"{[c.__name__ for c in seg_transforms.COLOR_STAGES]})")
        raise NotImplementedError(f"augmentation {name} has no GPU counterpart (supported: the classes of data/seg_transforms.py)")
    return cls()


def _label_map(ds, ignore_label):
    """The reference's raw-id -> class map (scannet.py:205-214) and its table over 0..NUM_LABELS-1 (int64)."""
    label_map, n_used = {}, 0
    for raw in range(ds.NUM_LABELS):
        if raw in ds.IGNORE_LABELS:
            label_map[raw] = ignore_label
        else:
            label_map[raw] = n_used
            n_used += 1
    label_map[ignore_label] = ignore_label
    lut = np.array([label_map[r] for r in range(ds.NUM_LABELS)], np.int64)
    return label_map, lut
