"""ScanNet point clouds without a GPU: the PLY reader, the numpy restatement of the voxel down-sampling rules, the dataset
schema, the host draw sequence of the colour stages against a replay of the reference's calls, and the recipe split."""
import os
import random

import numpy as np
import pytest
import torch

from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as ST
from nerf_downstream_amd.co3d_3d.src.data.ply import PlyError, load_ply, read_vertices, write_ply
from pc_restate import downsample, synthetic_scene, write_scannet_tree


def _columns(rng, n):
    return [("x", rng.normal(size=n).astype(np.float32)), ("y", rng.normal(size=n).astype(np.float64)),
            ("z", rng.normal(size=n).astype(np.float32)), ("red", rng.integers(0, 256, n).astype(np.uint8)),
            ("green", rng.integers(0, 256, n).astype(np.uint8)), ("blue", rng.integers(0, 256, n).astype(np.uint8)),
            ("alpha", rng.integers(-100, 100, n).astype(np.int16)), ("label", rng.integers(0, 41, n).astype(np.uint16)),
            ("instance", rng.integers(-5, 5, n).astype(np.int32))]


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian", "binary_big_endian"])
def test_ply_round_trip_with_trailing_faces(tmp_path, fmt):
    rng = np.random.default_rng(0)
    cols = _columns(rng, 57)
    face = np.array([3, 0, 1, 2] * 4, np.int32)
    body = b"3 0 1 2\n" * 4 if fmt == "ascii" else (np.uint8(3).tobytes() + np.array([0, 1, 2], ">i4" if "big" in fmt else "<i4").tobytes()) * 4
    assert face.size  # (four triangles)
    p = str(tmp_path / "s.ply")
    write_ply(p, cols, fmt, extra_elements=[("face", 4, ["property list uchar int vertex_indices"], body)])
    v = read_vertices(p)
    for name, a in cols:
        assert v[name].dtype == a.dtype and np.array_equal(v[name], a), name
    xyz, rgb, lab = load_ply(p)
    assert xyz.dtype == np.float32 and rgb.dtype == np.float32 and lab.dtype == np.int32
    assert np.array_equal(xyz[:, 1], cols[1][1].astype(np.float32)) and np.array_equal(rgb[:, 2], cols[5][1])
    assert np.array_equal(lab, cols[7][1])


def test_ply_new_type_names_and_a_scalar_element_before_vertex(tmp_path):
    p = tmp_path / "n.ply"
    head = ("ply\nformat binary_little_endian 1.0\ncomment new names\nelement camera 2\nproperty float64 f\n"
            "element vertex 2\nproperty float32 x\nproperty float32 y\nproperty float32 z\nproperty uint8 red\n"
            "property uint8 green\nproperty uint8 blue\nproperty int32 label\nend_header\n")
    rec = np.zeros(2, [("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("r", "u1"), ("g", "u1"), ("b", "u1"), ("l", "<i4")])
    rec["x"], rec["l"], rec["g"] = [1.5, -2.0], [7, 40], [9, 255]
    p.write_bytes(head.encode() + np.array([3.0, 4.0], "<f8").tobytes() + rec.tobytes())
    xyz, rgb, lab = load_ply(str(p))
    assert xyz[:, 0].tolist() == [1.5, -2.0] and lab.tolist() == [7, 40] and rgb[:, 1].tolist() == [9, 255]


def test_ply_list_before_vertex_is_refused(tmp_path):
    p = tmp_path / "bad.ply"
    p.write_bytes(b"ply\nformat ascii 1.0\nelement face 1\nproperty list uchar int vertex_indices\nelement vertex 1\n"
                  b"property float x\nproperty float y\nproperty float z\nend_header\n3 0 0 0\n1 2 3\n")
    with pytest.raises(PlyError, match="list property"):
        read_vertices(str(p))


def test_ply_unknown_type_and_format_are_refused(tmp_path):
    p = tmp_path / "t.ply"
    p.write_bytes(b"ply\nformat ascii 1.0\nelement vertex 1\nproperty half x\nend_header\n1\n")
    with pytest.raises(PlyError, match="unknown PLY type"):
        read_vertices(str(p))
    p.write_bytes(b"ply\nformat binary_middle_endian 1.0\nend_header\n")
    with pytest.raises(PlyError, match="format"):
        read_vertices(str(p))


# ------------------------------------------------------------------ down-sampling rules (numpy restatement)
def test_conflicting_labels_vote_ignore_and_order_follows_first_rows():
    xyz = np.array([[0.05, 0, 0], [0.001, 0.002, 0.003], [0.052, 0.001, 0.0], [0.003, 0.001, 0.004], [0.2, 0.2, 0.2]], np.float32)
    reps, c, lab = downsample(xyz, [5, 3, 5, 4, 9], 0.01, 0.02, -100)
    assert reps.tolist() == [0, 1, 4]
    assert lab.tolist() == [5, -100, 9]
    assert np.array_equal(c, xyz[[0, 1, 4]] / np.float32(0.02))


def test_negative_coordinates_floor():
    xyz = np.array([[-0.001, 0, 0], [0.001, 0, 0], [-0.0099, 0, 0], [-0.0101, 0, 0]], np.float32)
    reps, _, lab = downsample(xyz, [1, 2, 1, 3], 0.01, 0.02, -1)
    assert reps.tolist() == [0, 1, 3] and lab.tolist() == [1, 2, 3]


def test_everything_in_one_voxel_and_q_zero():
    xyz = np.random.default_rng(1).random((50, 3)).astype(np.float32) * 0.009
    reps, c, lab = downsample(xyz, np.full(50, 7), 0.01, 0.02, -100)
    assert reps.tolist() == [0] and lab.tolist() == [7]
    reps, c, lab = downsample(xyz, np.arange(50), 0.0, 0.02, -100)
    assert reps.tolist() == list(range(50)) and np.array_equal(c, xyz / np.float32(0.02)) and lab.tolist() == list(range(50))


# ------------------------------------------------------------------ dataset
@pytest.fixture
def tree(tmp_path):
    rng = np.random.default_rng(2)
    scenes = [synthetic_scene(rng, 500) for _ in range(3)]
    write_scannet_tree(str(tmp_path), scenes)
    return str(tmp_path), scenes


def test_dataset_is_registered():
    from nerf_downstream_amd.co3d_3d.src.data.datasets import get_dataset
    from nerf_downstream_amd.co3d_3d.src.data.scannet import PlenoxelScannetDataset, ScannetDataset

    assert get_dataset("ScannetDataset") is ScannetDataset
    assert ScannetDataset.NUM_LABELS == 41 and ScannetDataset.VALID_CLASS_IDS is PlenoxelScannetDataset.VALID_CLASS_IDS


@pytest.mark.parametrize("phase", ["train", "val"])
def test_dataset_schema(tree, phase):
    from nerf_downstream_amd.co3d_3d.src.data.scannet import ScannetDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink

    root, scenes = tree
    ds = ScannetDataset(phase, data_root=root)
    assert len(ds) == 3 and ds.downsample_voxel_size == 0.01
    s = ds[1]
    xyz, rgb, lab = scenes[1]
    assert torch.equal(s["coordinates"], torch.from_numpy(xyz)) and torch.equal(s["features"], torch.from_numpy(rgb))
    assert np.array_equal(s["labels"], lab)
    assert s["ds_params"].tolist() == [0.01, 0.02, -100.0, 0.0]
    lut = s["class_lut"].numpy()
    assert lut[1] == 0 and lut[39] == 19 and lut[0] == -100 and (lut >= 0).sum() == 20
    assert s["color_params"].shape == (ST.COLOR["PARAMS"],)
    if phase == "val":  # NormalizeColor only
        assert "aug_params" not in s and s["color_params"][0] == 1 and s["color_params"][1] == ST.COLOR["NORMALIZE"]
    else:
        assert s["aug_params"].shape == (ST.SEG["PARAMS"],)
    b = collate_mink([ds[0], ds[1]])
    assert b["coordinates"].shape == (1000, 4) and b["ds_params"].shape == (2, 4) and b["scene_offsets"].tolist() == [0, 500, 1000]
    assert b["color_params"].shape == (2, ST.COLOR["PARAMS"]) and b["aug_streams"].shape == (2,) and b["labels"].shape == (1000,)


def test_dataset_refuses_xyzs_and_unsupported_colour_classes(tree):
    from nerf_downstream_amd.co3d_3d.src.data.scannet import ScannetDataset

    root, _ = tree
    with pytest.raises(NotImplementedError, match="xyzs"):
        ScannetDataset("train", data_root=root, features=["colors", "xyzs"])
    for name in ("ChromaticAutoContrast", "HueSaturationTranslation"):
        with pytest.raises(NotImplementedError, match=name):
            ScannetDataset("train", data_root=root, train_transformations=["ChromaticTranslation", name])


# ------------------------------------------------------------------ host draws
class _RefTranslation:  # the reference's draw calls (transforms.py:57-61), restated
    def __init__(self, ratio=0.1, p=0.9):
        self.ratio, self.p = ratio, p

    def __call__(self, out):
        if random.random() < self.p:
            out.append(("translate", ((np.random.rand(1, 3) - 0.5) * 255 * 2 * self.ratio).reshape(3)))


class _RefJitter:  # transforms.py:106-111: the gate, then np.random.randn(N, 3)
    def __init__(self, std=0.01, p=0.9, n=0):
        self.std, self.p, self.n = std, p, n

    def __call__(self, out):
        if random.random() < self.p:
            out.append(("jitter", self.std * 255))


def test_colour_draws_replay_the_reference_sequence():
    comp = ST.PointCompose([ST.ChromaticTranslation(), ST.ChromaticJitter(0.01, 0.7), ST.NormalizeColor(),
                            ST.ChromaticTranslation(0.2, 0.5)])
    refs = [_RefTranslation(), _RefJitter(0.01, 0.7), None, _RefTranslation(0.2, 0.5)]
    for seed in range(20):
        random.seed(seed), np.random.seed(seed)
        _, ops = comp.draw()
        after = (random.random(), np.random.rand())
        random.seed(seed), np.random.seed(seed)
        want = []
        for r in refs:
            if r is None:
                want.append(("normalize",))
            else:
                r(want)
        assert (random.random(), np.random.rand()) == after
        assert [o[0] for o in ops] == [w[0] for w in want]
        for o, w in zip(ops, want):
            if o[0] != "normalize":
                assert np.array_equal(np.asarray(o[1]), np.asarray(w[1]))


def test_colour_stages_after_elastic_are_accepted():
    comp = ST.PointCompose([ST.RandomCrop(250, 250, 250), ST.ChromaticJitter(), ST.ElasticDistortion(((4, 16),)),
                            ST.NormalizeColor()])
    geo, col, _ = comp.sample(np.array([300.0, 300.0, 100.0]))
    assert geo.shape == (ST.SEG["PARAMS"],) and col[ST.COLOR["COUNT"]] in (1, 2)
    with pytest.raises(NotImplementedError):  # (the geometric program alone still refuses a stage after the elastic one)
        ST.SegCompose([ST.ElasticDistortion(), ST.RandomCrop(1, 1, 1)])


def test_plenoxel_recipe_compiles_to_the_same_row():
    names = ["RandomRotation", "RandomCrop", "RandomAffine", "CoordinateDropout", "RandomFeatureJitter", "RandomHorizontalFlip",
             "RandomTranslation", "ElasticDistortion"]
    make = lambda: [getattr(ST, n)(200, 200, 200) if n == "RandomCrop" else getattr(ST, n)() for n in names]  # noqa: E731
    for seed in range(5):
        random.seed(seed), np.random.seed(seed)
        a = ST.SegCompose(make()).sample(np.array([300.0, 150.0, 300.0]))
        random.seed(seed), np.random.seed(seed)
        geo, col, stream = ST.PointCompose(make()).sample(np.array([300.0, 150.0, 300.0]))
        assert col is None and np.array_equal(a[0], geo) and a[1] == stream


def test_unsupported_colour_classes_are_refused():
    for name in ST.UNSUPPORTED_COLOR:
        with pytest.raises(NotImplementedError, match=name):
            ST.split_color_stages([ST.NormalizeColor(), name])


def test_colour_program_row():
    P = ST.compile_color_program([("translate", np.array([1.0, -2.0, 3.0])), ("jitter", 2.55), ("normalize", np.float32([128] * 3),
                                                                                                 np.float32([256] * 3))])
    o = ST.COLOR["OPS"]
    assert P[0] == 3 and P[o:o + 4].tolist() == [1, 1, -2, 3] and P[o + 8:o + 10].tolist() == [2, 2.55]
    assert P[o + 16:o + 23].tolist() == [3, 128, 128, 128, 256, 256, 256]
    with pytest.raises(NotImplementedError):
        ST.compile_color_program([("jitter", 1.0)] * 5)


def test_semseg_config_parses():
    from nerf_downstream_amd import gin_lite as gin

    cfg = os.path.join(os.path.dirname(__file__), "..", "nerf_downstream_amd", "co3d_3d", "configs", "scannet_semseg.gin")
    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings([cfg], [])
        assert gin.query_parameter("get_dataset.dataset_name") == "ScannetDataset"
        assert gin.query_parameter("ScannetDataset.train_transformations")[-1] == "NormalizeColor"
    finally:
        gin.clear_config()
