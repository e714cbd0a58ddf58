"""SemanticKITTI and S3DIS without a GPU: the label tables, the registry, the sequence splits, the sample and batch schema
from synthetic trees, the gin configs, the prediction files, the numpy restatement's own rules, and the two LiDAR symbols of
include/mink_hip.h against the argument lists the binding passes."""
import os

import numpy as np
import pytest
import torch

from lidar_restate import (decode, finish, label_table, prepare_scene, synthetic_scan, write_kitti_tree, write_s3dis_tree)
from pc_restate import synthetic_scene

CFG = os.path.join(os.path.dirname(__file__), "..", "nerf_downstream_amd", "co3d_3d", "configs")
STATIC = {10: 0, 11: 1, 15: 2, 18: 3, 20: 4, 30: 5, 31: 6, 32: 7, 40: 8, 44: 9, 48: 10, 49: 11, 50: 12, 51: 13, 70: 14, 71: 15,
          72: 16, 80: 17, 81: 18}
MOVING = {252: 0, 253: 6, 254: 5, 255: 7, 258: 3, 259: 4}
IGNORED = (0, 1, 13, 16, 52, 60, 99, 256, 257)
INVERSE = [10, 11, 15, 18, 20, 30, 31, 32, 40, 44, 48, 49, 50, 51, 70, 71, 72, 80, 81]


@pytest.fixture
def kitti(tmp_path):
    rng = np.random.default_rng(3)
    scans = [synthetic_scan(rng, n) for n in (400, 300, 350, 1)]
    files = write_kitti_tree(str(tmp_path), scans, labels=[True, True, False, True])
    return str(tmp_path), scans, files


# ------------------------------------------------------------------ label tables
def test_label_table_pins():
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SemanticKITTIDataset, build_label_maps

    label_map, inv, by_name = build_label_maps(-100)
    assert label_map.shape == (260,) and inv.shape == (260,) and SemanticKITTIDataset.NUM_LABELS == 19
    for raw, cls in {**STATIC, **MOVING}.items():
        assert label_map[raw] == cls, raw
    for raw in IGNORED:
        assert label_map[raw] == -100, raw
    assert inv[:19].tolist() == INVERSE and not inv[19:].any()
    assert by_name["car"] == 0 and by_name["traffic-sign"] == 18 and len(by_name) == 19
    named = set(STATIC) | set(MOVING) | set(IGNORED)
    assert all(label_map[r] == -100 for r in range(260) if r not in named)  # (the reference leaves those at class 0)
    assert (build_label_maps(255)[0][list(IGNORED)] == 255).all()
    table, rinv = label_table(-100)  # the restatement builds the same tables on its own
    assert np.array_equal(table, label_map) and np.array_equal(rinv, inv)


def test_s3dis_label_map():
    from nerf_downstream_amd.co3d_3d.src.data.stanford import StanfordDataset

    assert StanfordDataset.NUM_LABELS == 14 and StanfordDataset.IGNORE_LABELS == (10,) and len(StanfordDataset.CLASS_LABELS) == 13
    assert StanfordDataset.VALID_CLASS_IDS == (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 11, 12, 13)
    assert StanfordDataset.DATA_PATH_FILE == {"train": "stanford_train.txt", "val": "stanford_val.txt", "test": "stanford_test.txt"}


def test_both_datasets_are_registered():
    from nerf_downstream_amd.co3d_3d.src.data.datasets import DATASETS, get_dataset
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SemanticKITTIDataset
    from nerf_downstream_amd.co3d_3d.src.data.stanford import StanfordDataset

    assert DATASETS["SemanticKITTIDataset"] is SemanticKITTIDataset and get_dataset("StanfordDataset") is StanfordDataset


# ------------------------------------------------------------------ SemanticKITTI samples
def test_sequence_splits(kitti):
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SEQUENCES, SemanticKITTIDataset

    assert SEQUENCES["train"] == ("00", "01", "02", "03", "04", "05", "06", "07", "09", "10")
    assert SEQUENCES["trainval"] == tuple(f"{i:02d}" for i in range(11)) and SEQUENCES["val"] == ("08",)
    assert SEQUENCES["test"] == tuple(str(i) for i in range(11, 22))
    root, _, files = kitti
    assert SemanticKITTIDataset("train", data_root=root).pc_files == files["00"]
    assert SemanticKITTIDataset("val", data_root=root).pc_files == files["08"]
    assert SemanticKITTIDataset("trainval", data_root=root).pc_files == files["00"] + files["08"]
    assert len(SemanticKITTIDataset("test", data_root=root)) == 0


def test_small_val_and_other_features_are_refused(kitti):
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SemanticKITTIDataset

    with pytest.raises(NotImplementedError, match="small_val"):
        SemanticKITTIDataset("small_val", data_root=kitti[0])
    with pytest.raises(NotImplementedError, match="xyzi"):
        SemanticKITTIDataset("train", data_root=kitti[0], features=["xyzs"])
    with pytest.raises(NotImplementedError, match="colour"):
        SemanticKITTIDataset("train", data_root=kitti[0], train_transformations=["NormalizeColor"])


def test_sample_and_batch_schema(kitti):
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as ST
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SemanticKITTIDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink

    root, scans, _ = kitti
    ds = SemanticKITTIDataset("train", data_root=root)  # scans 0 and 2: the second one without its .label file
    assert len(ds) == 2 and ds.downsample_voxel_size == 0.025 and ds.voxel_size == 0.05 and ds.ignore_label == -100
    assert ds.transformations_list == ["CoordinateDropout", "RandomHorizontalFlip", "RandomAffine", "RandomTranslation"]
    s, t = ds[0], ds[1]
    assert s["scan"].dtype == torch.float32 and s["scan"].shape == (400, 4) and np.array_equal(s["scan"].numpy(), scans[0][0])
    assert s["raw_labels"].dtype == torch.int32 and np.array_equal(s["raw_labels"].numpy().view(np.uint32), scans[0][1])
    assert (s["raw_labels"].numpy().view(np.uint32) >> 16).any()  # (instance ids travel; the device drops them)
    assert t["raw_labels"] is None and np.array_equal(t["scan"].numpy(), scans[2][0])
    assert s["label_lut"].dtype == torch.int64 and s["label_lut"].shape == (260,) and s["label_lut"][252] == 0
    # host values as numpy, not tensors: the trainer moves every tensor but `aug_params` to the device
    assert isinstance(s["lidar_params"], np.ndarray) and s["lidar_params"].dtype == np.float64
    assert s["lidar_params"].tolist() == [0.025, 0.05, -100.0]
    assert s["aug_params"].dtype == torch.float64 and s["aug_params"].shape == (ST.SEG["PARAMS"],) and isinstance(s["aug_stream"], int)
    assert s["metadata"] == {"file": "00/velodyne/000000.bin", "sequence": "00", "filename": "000000.bin", "data_index": 0}
    assert s["feature_names"] == ("xyzi",) and "coordinates" not in s and "labels" not in s  # nothing else is computed here
    b = collate_mink([s, t])
    assert b["scan"].shape == (750, 4) and b["scene_offsets"].tolist() == [0, 400, 750]
    assert isinstance(b["lidar_params"], np.ndarray) and b["lidar_params"].shape == (2, 3) and b["lidar_params"].dtype == np.float64
    from nerf_downstream_amd.co3d_3d.train import _to_device

    moved = _to_device(b, torch.device("cpu"))  # (what the trainer does to a batch: these two stay what they are)
    assert moved["lidar_params"] is b["lidar_params"] and moved["aug_params"] is b["aug_params"]
    assert b["raw_labels"].dtype == torch.int32 and not b["raw_labels"][400:].any() and torch.equal(b["raw_labels"][:400], s["raw_labels"])
    assert b["aug_params"].shape == (2, ST.SEG["PARAMS"]) and b["aug_streams"].shape == (2,) and isinstance(b["aug_seed"], int)
    assert b["label_lut"].shape == (260,) and [m["sequence"] for m in b["metadata"]] == ["00", "00"]
    assert "raw_labels" not in collate_mink([t, t])
    val = SemanticKITTIDataset("val", data_root=root)  # no recipe
    v = val[1]
    assert v["scan"].shape == (1, 4) and "aug_params" not in v and "aug_params" not in collate_mink([val[0], v])
    assert SemanticKITTIDataset("train", data_root=root, downsample_voxel_size=0)[0]["lidar_params"][0] == 0


def test_save_prediction_round_trip(kitti, tmp_path):
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SemanticKITTIDataset

    ds = SemanticKITTIDataset("val", data_root=kitti[0])
    pred = np.random.default_rng(0).integers(0, 19, 77)
    meta = ds[0]["metadata"]
    out = str(tmp_path / "pred")
    for p in (pred, torch.from_numpy(pred)):
        path = ds.save_prediction(p, out, meta)
        assert path == os.path.join(out, "sequences", "08", "predictions", "000001.label")
        words = np.fromfile(path, dtype=np.uint32)
        assert words.shape == (77,) and os.path.getsize(path) == 4 * 77  # one word per predicted row
        assert np.array_equal(words, np.array(INVERSE, np.uint32)[pred])
        assert np.array_equal(ds.label_map[words], pred)  # the inverse map inverts the map
    assert "not one word per raw point" in " ".join(ds.save_prediction.__doc__.lower().split())


# ------------------------------------------------------------------ S3DIS samples
def test_s3dis_sample_and_map(tmp_path):
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as ST
    from nerf_downstream_amd.co3d_3d.src.data.stanford import StanfordDataset

    rng = np.random.default_rng(5)
    scenes = [(xyz, rgb, (lab % 14).astype(np.int32)) for xyz, rgb, lab in (synthetic_scene(rng, 300) for _ in range(2))]
    write_s3dis_tree(str(tmp_path), scenes)
    ds = StanfordDataset("train", data_root=str(tmp_path))
    assert len(ds) == 2 and ds.downsample_voxel_size == 0.015 and ds.voxel_size == 0.03 and ds.NUM_CLASSES == 13
    assert [type(t).__name__ for t in ds.transformations.transforms] == ["ChromaticTranslation", "ChromaticJitter", "CoordinateDropout",
                                                                          "RandomHorizontalFlip", "RandomRotation", "NormalizeColor"]
    s = ds[1]
    assert s["class_lut"].tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, -100, 10, 11, 12]
    assert s["ds_params"].tolist() == [0.015, 0.03, -100.0, 0.0] and np.array_equal(s["labels"], scenes[1][2])
    assert s["aug_params"].shape == (ST.SEG["PARAMS"],) and s["color_params"].shape == (ST.COLOR["PARAMS"],)
    val = StanfordDataset("val", data_root=str(tmp_path))
    assert "aug_params" not in val[0] and val[0]["color_params"][0] == 1 and len(StanfordDataset("test", data_root=str(tmp_path))) == 2


# ------------------------------------------------------------------ configs
@pytest.mark.parametrize("cfg,name,cin,cout", [("semantic_kitti.gin", "SemanticKITTIDataset", 4, 19), ("stanford_semseg.gin", "StanfordDataset", 3, 13)])
def test_configs_parse_and_build_dataset_and_model(tmp_path, cfg, name, cin, cout):
    from nerf_downstream_amd import gin_lite as gin
    from nerf_downstream_amd.co3d_3d.src.data.datasets import get_dataset
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from oracle import me_cpu as OME

    rng = np.random.default_rng(7)
    if cin == 4:
        write_kitti_tree(str(tmp_path), [synthetic_scan(rng, 50) for _ in range(2)])
    else:
        write_s3dis_tree(str(tmp_path), [(x, c, (l % 14).astype(np.int32)) for x, c, l in [synthetic_scene(rng, 50)]])
    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings([os.path.join(CFG, cfg), os.path.join(CFG, "res16unet.gin")], [f"{name}.data_root='{tmp_path}'"])
        assert gin.query_parameter("get_dataset.dataset_name") == name and gin.query_parameter("train.optimizer_name") == "SGD"
        assert gin.query_parameter("get_model.in_channel") == cin and gin.query_parameter("get_model.out_channel") == cout
        ds = get_dataset()("train")
        assert type(ds).__name__ == name and len(ds) >= 1 and ds.NUM_CLASSES == cout
        assert ds.voxel_size == (0.05 if cin == 4 else 0.03)
        model = get_model(gin.query_parameter("get_model.name"), cin, cout, ME=OME)
        assert model.final.kernel.shape[-1] == cout
    finally:
        gin.clear_config()


# ------------------------------------------------------------------ the restatement's own rules
def test_table_comes_before_the_vote():
    """The data set's own table through the restated preparation: the order the device program is held to."""
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import LUT_SIZE, build_label_maps

    table = build_label_maps(-100)[0]
    assert len(table) == LUT_SIZE == 260
    scan = np.array([[1.001, 2.0, 0.0, 0.5], [1.002, 2.0, 0.0, 0.25], [-3.01, 0.0, 0.0, 0.1], [-3.02, 0.0, 0.0, 0.2], [5.0, 5.0, 5.0, 0.3]],
                    np.float32)
    words = np.array([10 | (7 << 16), 252 | (9 << 16), 10, 11, 4], np.uint32)
    c, f, cls, rows = prepare_scene(scan, words, table, 0.025, 0.05, -100)
    assert rows.tolist() == [0, 2, 4] and cls.tolist() == [0, -100, -100]  # car + moving-car: car; car + bicycle, unnamed id: ignore
    assert np.array_equal(c, scan[[0, 2, 4], :3] / np.float32(0.05)) and np.array_equal(f, scan[[0, 2, 4]])
    _, _, lab, bad = decode([scan, scan[:2]], [np.array([259, 260, 0xFFFF, 0x10000 | 81, 0], np.uint32), None], table, -100)
    assert lab.tolist() == [4, -100, -100, 18, -100, -100, -100] and bad == 2
    r = np.array([[0.1, -0.2, 1e-9]])
    assert np.array_equal(finish(r, 0.05)[0], r.astype(np.float32) / np.float32(0.05))


# ------------------------------------------------------------------ C ABI
def test_header_declares_the_two_symbols_as_the_binding_calls_them():
    import ctypes

    from nerf_downstream_amd._lib import CONSTANTS, SIGNATURES

    p, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64, ctypes.c_float
    # scan, raw_labels, n, scene_offsets, n_scenes, lut, lut_size, ignore_label, coords, feats, ldo, labels, status, stream
    assert SIGNATURES["mink_lidar_decode_scans"] == (ctypes.c_int, [p, p, i64, p, i32, p, i32, i32, p, p, i64, p, p, p])
    # coords, n, n_rows (device), voxel_size, feats, ldf, c0, stream
    assert SIGNATURES["mink_lidar_finish_rows"] == (ctypes.c_int, [p, i64, p, f32, p, i64, i32, p])
    assert CONSTANTS["MINK_ABI_VERSION"] == 4  # additive
    from nerf_downstream_amd.minkowski import utils

    for name in ("lidar_decode_batch", "lidar_status_check", "lidar_finish_rows", "prepare_lidar_batch", "LidarLabelError"):
        assert hasattr(utils, name), name
    utils.lidar_status_check(0)
    with pytest.raises(utils.LidarLabelError):
        utils.lidar_status_check(torch.tensor([2], dtype=torch.int32))
