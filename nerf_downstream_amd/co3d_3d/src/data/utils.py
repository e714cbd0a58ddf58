"""Batch collation (counterpart of the reference's co3d_3d/src/data/utils.py:25-50)."""
import numpy as np
import torch

from nerf_downstream_amd.minkowski import utils as me_utils


def _cat(tensors):
    """torch.cat; in a DataLoader worker the result is allocated in SHARED memory (as torch's default_collate does), so handing the
    batch to the trainer passes a file descriptor instead of copying its 29-105 MB a second time."""
    if torch.utils.data.get_worker_info() is None:
        return torch.cat(tensors)
    first = tensors[0]
    shape = (sum(int(t.shape[0]) for t in tensors),) + tuple(first.shape[1:])
    numel = int(np.prod(shape))
    storage = first._typed_storage()._new_shared(numel, device=first.device)
    out = first.new(storage).resize_(*shape)
    return torch.cat(tensors, out=out)


def collate_mink(list_data):
    """list of sample dicts -> {"coordinates": f32 [sumN,4] (batch,x,y,z), "features": f32 [sumN,C],
    "labels": int64 [B]}.  Runs in DataLoader workers: CPU only."""
    if "links" in list_data[0]:  # compact on-disk form (Co3DDatasetBase(compact=True)): decoded on the GPU later
        n = [int(d["links"].shape[0]) for d in list_data]
        package = {
            "links": _cat([d["links"] for d in list_data]),
            "density": _cat([d["density"] for d in list_data]),
            "sh_q": _cat([d["sh_q"] for d in list_data]),
            "scene_offsets": torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int32),
            "sh_scale": torch.stack([d["sh_scale"] for d in list_data]),
            "sh_min": torch.stack([d["sh_min"] for d in list_data]),
            "labels": torch.from_numpy(np.concatenate([np.asarray(d["labels"]) for d in list_data])),
            "feature_names": list_data[0]["feature_names"],
        }
        resos = {tuple(d.get("reso", (128, 128, 128))) for d in list_data}
        if len(resos) != 1:
            raise ValueError(f"one batch mixes grid resolutions {sorted(resos)} (data.npz scenes are 128^3, last.ckpt scenes 256^3)")
        package["reso"] = resos.pop()
        return _with_sampler(_with_programs(package, list_data, n), list_data, n)
    if "scan" in list_data[0]:  # raw LiDAR scans (SemanticKITTIDataset): decoded, down-sampled and augmented on the GPU later
        return _collate_scans(list_data)
    coords, feats = me_utils.sparse_collate(
        [d["coordinates"] for d in list_data], [d["features"] for d in list_data], dtype=torch.float32
    )
    package = {"coordinates": coords, "features": feats}
    for key in list_data[0].keys():
        if "label" in key or "instance" in key or "dists" in key:
            package[key] = torch.from_numpy(np.concatenate([np.asarray(d[key]) for d in list_data]))
    for key in ("metadata", "dataset", "colors"):
        if key in list_data[0]:
            package[key] = [d[key] for d in list_data]
    n = [int(d["coordinates"].shape[0]) for d in list_data]
    return _with_sampler(_with_points(_with_programs(package, list_data, n), list_data, n), list_data, n)


def _collate_scans(list_data):
    """Raw LiDAR scans (data/semantic_kitti.py): the .bin records and the .label words of every scan one after the other,
    one (down-sampling voxel size, voxel size, ignore label) row per scan and the raw-id -> class table.  `raw_labels` is
    left out when no scan of the batch had a .label file (every word is 0 then); a scan without one among others gets zeros."""
    n = [int(d["scan"].shape[0]) for d in list_data]
    package = {
        "scan": _cat([d["scan"] for d in list_data]),
        "scene_offsets": torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int32),
        # a numpy array, not a tensor: the trainer moves tensors to the device, and these host values size and steer the
        # launches (as `aug_params`, which it keeps on the host by name)
        "lidar_params": np.stack([np.asarray(d["lidar_params"], np.float64) for d in list_data]),
        "label_lut": list_data[0]["label_lut"],
        "feature_names": list_data[0].get("feature_names"),
    }
    if any(d.get("raw_labels") is not None for d in list_data):
        package["raw_labels"] = _cat([d["raw_labels"] if d.get("raw_labels") is not None else torch.zeros(k, dtype=torch.int32)
                                      for d, k in zip(list_data, n)])
    for key in ("metadata", "dataset"):
        if key in list_data[0]:
            package[key] = [d[key] for d in list_data]
    return _with_programs(package, list_data, n)


def _with_programs(package, list_data, n):
    """Augmentation programs drawn by the dataset (transforms.Compose.sample): one parameter row and one
    Philox stream id per scene, plus a seed for the batch; applied on the GPU in process_input."""
    if "aug_params" in list_data[0]:
        package["aug_params"] = torch.stack([d["aug_params"] for d in list_data])
        streams = np.array([d["aug_stream"] for d in list_data], dtype=np.uint32)
        package["aug_streams"] = torch.from_numpy(streams.view(np.int32).copy())
        package["aug_seed"] = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
        package.setdefault("scene_offsets", torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int32))
        package.setdefault("feature_names", list_data[0].get("feature_names"))
    return package


def _with_sampler(package, list_data, n):
    """The plan of the recipe's sampler (data/sampling.py), one per scene: `fps_start` int32 [B], the scene-local row of the
    first farthest-point pick, or `sample_rows` int64 [B, m], the drawn rows as GLOBAL rows of the batch; `sample_points` = m
    and `sample_n_max`, the largest scene (host ints).  The rows are taken on the GPU in process_input."""
    if "sample_points" in list_data[0]:
        offs = np.concatenate([[0], np.cumsum(n)])
        package["sample_points"], package["sample_n_max"] = int(list_data[0]["sample_points"]), int(max(n))
        if "fps_start" in list_data[0]:
            package["fps_start"] = torch.tensor([int(d["fps_start"]) for d in list_data], dtype=torch.int32)
        else:
            package["sample_rows"] = torch.from_numpy(np.stack([np.asarray(d["sample_rows"], np.int64) + offs[j]
                                                                 for j, d in enumerate(list_data)]))
        package.setdefault("scene_offsets", torch.tensor(offs, dtype=torch.int32))
        package.setdefault("feature_names", list_data[0].get("feature_names"))
    return package


def _with_points(package, list_data, n):
    """Raw point clouds (data/scannet.py ScannetDataset): one down-sampling row per scene, the raw-label -> class table,
    and the colour programs with their Philox stream ids when the recipe has colour stages; prepared on the GPU."""
    if "ds_params" in list_data[0]:
        package["ds_params"] = torch.stack([d["ds_params"] for d in list_data])
        package["class_lut"] = list_data[0]["class_lut"]
        package.setdefault("scene_offsets", torch.tensor(np.concatenate([[0], np.cumsum(n)]), dtype=torch.int32))
        if "color_params" in list_data[0]:
            package["color_params"] = torch.stack([d["color_params"] for d in list_data])
        if "aug_stream" in list_data[0] and "aug_streams" not in package:
            streams = np.array([d["aug_stream"] for d in list_data], dtype=np.uint32)
            package["aug_streams"] = torch.from_numpy(streams.view(np.int32).copy())
            package["aug_seed"] = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    return package
