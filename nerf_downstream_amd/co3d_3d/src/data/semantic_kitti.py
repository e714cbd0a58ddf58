"""SemanticKITTI LiDAR scans for the segmentation family (counterpart of the reference's `SemanticKITTIDataset`,
co3d_3d/src/data/semantic_kitti.py:73-238; configs/semantic_kitti.gin).

`<data_root>/dataset/sequences/<seq>/velodyne/<name>.bin` holds float32 (x, y, z, intensity) records in metres,
`.../labels/<name>.label` one 32-bit word per point: the semantic id in the low 16 bits, the instance id above them.

The loader only reads and draws.  A sample carries the raw scan, the raw label words (None without a .label file: the
reference labels such a scan 0 everywhere), the 260-entry raw-id -> class table, one (down-sampling voxel size, voxel size,
ignore label) row and the drawn geometric program (MINK_SEGAUG_*).  `MinkowskiBaseModel.process_input` then runs on the GPU
(`prepare_lidar_batch`), per scan and in the reference's order (:183-209):

* labels = table[word & 0xFFFF] -- BEFORE the voxel vote, so a voxel holding `car` (10) and `moving-car` (252) votes car;
* ME.utils.sparse_quantize(xyz, xyzi, labels, quantization_size=downsample_voxel_size) with label voting;
* the recipe, in METRES (the division by voxel_size comes after it, unlike ScannetDataset);
* features `xyzi` = the transformed metric coordinates and the intensity; coordinates = the same / voxel_size.

Differences from the reference, by design:
* its table is `np.zeros(260)`, so a semantic id below 260 that the label list does not name maps to class 0 (car); here
  such an id maps to `ignore_label`.  An id of 260 or more raises an IndexError there and `LidarLabelError` here.  Real
  SemanticKITTI files hold neither.
* `phase="small_val"` has no sequence list there (dead code); it is refused."""
import os

import numpy as np
import torch
from torch.utils.data import Dataset

from nerf_downstream_amd import gin_lite as gin

from . import seg_transforms
from .scannet import _transform

CLASS_LABELS = ("car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "bicyclist", "motorcyclist", "road", "parking",
                "sidewalk", "other-ground", "building", "fence", "vegetation", "trunk", "terrain", "pole", "traffic-sign")

# the raw semantic ids of the data set (semantic-kitti-api, config/semantic-kitti.yaml)
LABEL_NAMES = {
    0: "unlabeled", 1: "outlier", 10: "car", 11: "bicycle", 13: "bus", 15: "motorcycle", 16: "on-rails", 18: "truck",
    20: "other-vehicle", 30: "person", 31: "bicyclist", 32: "motorcyclist", 40: "road", 44: "parking", 48: "sidewalk",
    49: "other-ground", 50: "building", 51: "fence", 52: "other-structure", 60: "lane-marking", 70: "vegetation", 71: "trunk",
    72: "terrain", 80: "pole", 81: "traffic-sign", 99: "other-object", 252: "moving-car", 253: "moving-bicyclist",
    254: "moving-person", 255: "moving-motorcyclist", 256: "moving-on-rails", 257: "moving-bus", 258: "moving-truck",
    259: "moving-other-vehicle",
}
LUT_SIZE = 260

SEQUENCES = {
    "train": ("00", "01", "02", "03", "04", "05", "06", "07", "09", "10"),
    "trainval": ("00", "01", "02", "03", "04", "05", "06", "07", "08", "09", "10"),
    "val": ("08",),
    "test": ("11", "12", "13", "14", "15", "16", "17", "18", "19", "20", "21"),
}


def build_label_maps(ignore_label):
    """-> (label_map int64 [260], label_inv_map int64 [260], {class name: class}) as the reference builds them (:134-157):
    static ids in ascending order take the classes 0..18, a `moving-` id takes the class of its static name, everything
    else `ignore_label` -- and so does every id the list does not name (the reference leaves those at 0)."""
    label_map = np.full(LUT_SIZE, ignore_label, np.int64)
    label_inv_map = np.zeros(LUT_SIZE, np.int64)
    class_of, cnt = {}, 0
    for raw, name in LABEL_NAMES.items():
        if raw > 250:
            static = name.replace("moving-", "")
            if static in CLASS_LABELS:
                label_map[raw] = class_of[static]
        elif raw != 0 and name in CLASS_LABELS:
            label_map[raw] = class_of[name] = cnt
            label_inv_map[cnt] = raw
            cnt += 1
    return label_map, label_inv_map, class_of


@gin.configurable
class SemanticKITTIDataset(Dataset):
    NUM_LABELS = 19
    CLASS_LABELS = CLASS_LABELS

    def __init__(self, phase, data_root="datasets/semantic-kitti/", downsample_voxel_size=None, voxel_size=0.05,
                 train_transformations=("CoordinateDropout", "RandomHorizontalFlip", "RandomAffine", "RandomTranslation"),
                 eval_transformations=(), ignore_label=-100, features=("xyzi",)):
        if phase not in SEQUENCES:
            if phase == "small_val":
                raise NotImplementedError("phase 'small_val' has no sequence list in the reference (semantic_kitti.py:106-126 "
                                          "never reaches its [::10] branch): use 'val'")
            raise ValueError(f"phase {phase!r}: one of {sorted(SEQUENCES)}")
        self.phase, self.data_root, self.ignore_label = phase, data_root, ignore_label
        self.features = list(features)
        if self.features != ["xyzi"]:
            raise NotImplementedError(f"features {self.features}: the LiDAR preparation on the device produces ['xyzi']")
        self.transformations_list = list(train_transformations if phase == "train" else eval_transformations)
        stages = [_transform(t) for t in self.transformations_list]
        if any(isinstance(t, seg_transforms.COLOR_STAGES) for t in stages):
            raise NotImplementedError("colour stages on a LiDAR scan: its features are xyz and the intensity")
        self.transformations = seg_transforms.PointCompose(stages) if stages else None
        self.pc_files = []
        for seq in SEQUENCES[phase]:
            names = sorted(os.listdir(os.path.join(self.data_root, "dataset/sequences", seq, "velodyne")))
            self.pc_files.extend(os.path.join(seq, "velodyne", x) for x in names)
        if downsample_voxel_size is None:
            downsample_voxel_size = voxel_size / 2
        self.downsample_voxel_size, self.voxel_size = downsample_voxel_size, voxel_size
        self.label_map, self.label_inv_map, self.reverse_label_name_mapping = build_label_maps(ignore_label)
        self.NUM_CLASSES = len(self.CLASS_LABELS)

    def __len__(self):
        return len(self.pc_files)

    def __getitem__(self, data_index):
        sequence, filename = self.pc_files[data_index].split("/")[0], self.pc_files[data_index].split("/")[-1]
        full_path = os.path.join(self.data_root, "dataset/sequences", self.pc_files[data_index])
        scan = np.fromfile(full_path, dtype=np.float32).reshape(-1, 4)
        label_file = full_path.replace("velodyne", "labels").replace(".bin", ".label")
        raw = None
        if os.path.exists(label_file):
            raw = np.fromfile(label_file, dtype=np.int32).reshape(-1)
            if len(raw) != len(scan):
                raise ValueError(f"{label_file}: {len(raw)} label words for {len(scan)} points")
        lp = np.array([max(float(self.downsample_voxel_size), 0.0), self.voxel_size, self.ignore_label], np.float64)
        sample = {"scan": torch.from_numpy(scan), "raw_labels": None if raw is None else torch.from_numpy(raw),
                  "label_lut": torch.from_numpy(self.label_map), "lidar_params": lp,  # (numpy: host values, never moved to the device)
                  "metadata": {"file": self.pc_files[data_index], "sequence": sequence, "filename": filename, "data_index": data_index},
                  "dataset": "semantic_kitti", "feature_names": tuple(self.features)}
        if self.transformations is not None:  # drawn here (DataLoader worker), applied on the GPU, in metres
            extent = (scan[:, :3].max(0) - scan[:, :3].min(0)).astype(np.float64) if len(scan) else np.zeros(3)
            geo, _, stream = self.transformations.sample(extent)
            sample["aug_params"], sample["aug_stream"] = torch.from_numpy(geo), stream
        return sample

    def save_prediction(self, prediction, save_path, metadata):
        """Write class predictions as raw ids (uint32, through `label_inv_map`) to
        `<save_path>/sequences/<seq>/predictions/<name>.label`, as the reference does (:224-238); returns the path.  A host
        function.  It writes one word per PREDICTED row -- the rows the model saw, i.e. the down-sampled (and, in training,
        augmented) representatives -- which is NOT one word per raw point of the scan: the file lines up with the .bin file
        only for a prediction that was carried back to every raw point first."""
        pred_file = os.path.join(save_path, "sequences", metadata["sequence"], "predictions", metadata["filename"].replace("bin", "label"))
        os.makedirs(os.path.dirname(pred_file), exist_ok=True)
        if isinstance(prediction, torch.Tensor):
            prediction = prediction.cpu().numpy()
        self.label_inv_map[np.asarray(prediction)].astype(np.uint32).tofile(pred_file)
        return pred_file

    def __repr__(self):
        return (f"{self.__class__.__name__}(phase={self.phase}, length={len(self)}, features={self.features}, "
                f"downsample_voxel_size={self.downsample_voxel_size}, voxel_size={self.voxel_size}, "
                f"transformations={self.transformations_list})")
