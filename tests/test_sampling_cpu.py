"""CPU: scene sub-sampling away from the kernel -- the numpy restatement of farthest-point sampling (tests/fps_restate.py)
against hand-worked cases, the two sampler classes (gin bindings of configs/co3d_points.gin, `plan()`), the dataset and collate
plumbing on a tiny written tree in the decoded and the compact form, every ordering refusal, the argument checks of
mink_fps_scenes (refused before any launch), and the sampler stage of `process_input` on the CPU backend of the trainer tests."""
import os
import re

import numpy as np
import pytest
import torch

import fps_restate as FR
from nerf_downstream_amd import gin_lite as gin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")


@pytest.fixture(autouse=True)
def _clean_gin():
    gin.clear_config()
    yield
    gin.clear_config()


def write_scenes(tmp_path, sizes=(300, 357), seed=1):
    """A tiny PeRFception-CO3D tree (data.npz scenes + filelist/train.txt and test.txt) -> the raw arrays per scene."""
    rng = np.random.default_rng(seed)
    (tmp_path / "filelist").mkdir()
    lines, raw = [], []
    for j, n in enumerate(sizes):
        links = np.sort(rng.choice(128 ** 3, n, replace=False)).astype(np.int32)
        sh = rng.integers(0, 256, (n, 27)).astype(np.uint8)
        dens = rng.random((n, 1)).astype(np.float32)
        scene = tmp_path / "data" / f"plenoxel_co3d_s{j}"
        scene.mkdir(parents=True)
        np.savez(scene / "data.npz", links=links, density=dens, sh=sh, sh_min=np.float32(-1.5), sh_scale=np.float32(0.0123),
                 reso=[[128] * 3, [256] * 3])
        lines.append(f"{'cup' if j % 2 else 'apple'} s{j}")
        raw.append({"links": links, "density": dens, "sh_q": sh})
    for f in ("train.txt", "test.txt"):
        (tmp_path / "filelist" / f).write_text("\n".join(lines) + "\n")
    return raw


def coords_of(links):
    links = np.asarray(links, np.int64)
    return np.stack([links // (128 * 128), links % (128 * 128) // 128, links % 128], 1).astype(np.float32)


# ------------------------------------------------------------------------------------------------------------ the restatement
def test_restatement_on_a_cube_is_all_ties():
    """2 x 2 x 2 integer grid, row = 4x + 2y + z.  From corner s the opposite corner 7 - s is alone at distance 3; after it every
    other point sits at distance 1 from what was picked and stays there until it is picked itself: ascending rows."""
    cube = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float32)
    for s in range(8):
        rest = [r for r in range(8) if r not in (s, 7 - s)]
        assert FR.fps_scene(cube, 9, s).tolist() == [s, 7 - s] + rest + [0]  # (all taken: every distance 0, row 0)


def test_restatement_on_a_line_of_five():
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [4, 0, 0]], np.float32)
    assert FR.fps_scene(line, 5, 0).tolist() == [0, 4, 2, 1, 3]  # 16 | [0,1,4,1,0] | tie 1,3 -> 1
    assert FR.fps_scene(line, 5, 2).tolist() == [2, 0, 4, 1, 3]  # tie 0,4 -> 0
    assert FR.fps_scene(line, 2, 4).tolist() == [4, 0]


def test_restatement_with_fewer_points_than_picks():
    pts = np.array([[0, 0, 0], [1, 0, 0], [3, 0, 0]], np.float32)
    assert FR.fps_scene(pts, 5, 1).tolist() == [1, 2, 0, 0, 0]
    assert FR.fps_batch(np.concatenate([pts, pts]), [0, 3, 6], 4, [1, 2]).tolist() == [[1, 2, 0, 0], [5, 3, 4, 3]]


def test_restatement_rounds_every_operation_to_fp32():
    """Coordinates at which a fused multiply-add or a float64 sum would pick differently: the restatement agrees with the
    reference's torch expression, operation by operation."""
    g = torch.Generator().manual_seed(3)
    xyz = torch.randn(400, 3, generator=g) * 1e3 + 1e4
    dist, cur, want = torch.ones(400) * 1e10, 17, []
    for _ in range(40):
        want.append(cur)
        d = torch.sum((xyz - xyz[cur]) ** 2, -1)
        mask = d < dist
        dist[mask] = d[mask]
        cur = int(torch.argmax(dist))
    assert FR.fps_scene(xyz.numpy(), 40, 17).tolist() == want


def test_host_implementation_of_the_cpu_backend_equals_the_restatement():
    from nerf_downstream_amd.co3d_3d.src.data.sampling import fps_numpy

    rng = np.random.default_rng(0)
    xyz = np.concatenate([rng.integers(0, 128, (70, 3)), rng.integers(0, 128, (5, 3))]).astype(np.float32)
    assert np.array_equal(fps_numpy(xyz, [0, 70, 75], 9, [69, 0]), FR.fps_batch(xyz, [0, 70, 75], 9, [69, 0]))
    with pytest.raises(ValueError):
        fps_numpy(xyz, [0, 70, 70], 4, [0, 0])
    with pytest.raises(ValueError):
        fps_numpy(xyz, [0, 70, 75], 4, [70, 0])


# ------------------------------------------------------------------------------------------------------------ classes, config
def test_gin_binds_both_classes_from_the_recipe():
    from nerf_downstream_amd.co3d_3d.src.data import sampling as S
    from nerf_downstream_amd.co3d_3d.src.data import transforms as T

    gin.parse_config_files_and_bindings([f"{CFG}/co3d_cls.gin", f"{CFG}/co3d_points.gin", f"{CFG}/dgcnn.gin"], [])
    assert S.FarthestPointSample().num_points == 1024 and S.RandomSample().num_points == 1024
    assert gin.query_parameter("Co3DDatasetBase.train_transformations")[0] == "FarthestPointSample"
    assert gin.query_parameter("Co3DDatasetBase.eval_transformations") == ["FarthestPointSample"]
    assert gin.query_parameter("get_model.name") == "DGCNN_cls"
    assert gin.query_parameter("get_model.in_channel") == len(T.raw_columns(gin.query_parameter("Co3DDatasetBase.features"))) == 30
    gin.bind_parameter("RandomSample.num_points", 7)
    assert S.RandomSample().num_points == 7 and S.RandomSample(num_points=9).num_points == 9
    assert not hasattr(S.FarthestPointSample, "draw") and not hasattr(S.RandomSample, "draw")
    with pytest.raises(ValueError):
        S.FarthestPointSample(0)


def test_plans():
    from nerf_downstream_amd.co3d_3d.src.data.sampling import FarthestPointSample, RandomSample

    np.random.seed(5)
    starts = {FarthestPointSample(16).plan(3)["fps_start"] for _ in range(200)}
    assert starts == {0, 1, 2} and FarthestPointSample(16).plan(3)["sample_points"] == 16
    assert FarthestPointSample(4).plan(1) == {"fps_start": 0, "sample_points": 4}
    for n, m in ((50, 10), (11, 10)):  # more rows than picks: no row twice
        p = RandomSample(m).plan(n)
        assert p["sample_points"] == m and p["sample_rows"].dtype == np.int64 and p["sample_rows"].shape == (m,)
        assert len(set(p["sample_rows"].tolist())) == m and 0 <= p["sample_rows"].min() and p["sample_rows"].max() < n
    p = RandomSample(10).plan(10)  # n <= m: with replacement, as the reference (a permutation has probability 10! / 10^10)
    assert p["sample_rows"].shape == (10,) and p["sample_rows"].max() < 10
    assert any(len(set(RandomSample(10).plan(10)["sample_rows"].tolist())) < 10 for _ in range(20))
    p = RandomSample(40).plan(3)
    assert p["sample_rows"].shape == (40,) and set(p["sample_rows"].tolist()) == {0, 1, 2}
    np.random.seed(9)  # the reference's draws, in its order
    a = RandomSample(6).plan(20)["sample_rows"]
    np.random.seed(9)
    assert np.array_equal(a, np.random.choice(20, 6, replace=False))
    np.random.seed(9)
    b = FarthestPointSample(6).plan(20)["fps_start"]
    np.random.seed(9)
    assert b == np.random.randint(0, 20)


# ------------------------------------------------------------------------------------------------------------ dataset, collate
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("density", [False, True])
def test_dataset_emits_the_plan_and_collate_batches_it(tmp_path, monkeypatch, compact, density):
    from nerf_downstream_amd.co3d_3d.src.data.co3d import Co3DDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink

    raw = write_scenes(tmp_path)
    monkeypatch.chdir(tmp_path)
    gin.parse_config("DensityBasedSample.percentile = 40.0\nFarthestPointSample.num_points = 32\nRandomSample.num_points = 400")
    pre = ["DensityBasedSample"] if density else []
    kept = [int((r["density"].reshape(-1) > np.percentile(r["density"], 40.0)).sum()) if density else len(r["links"]) for r in raw]
    kw = dict(phase="train", data_root=str(tmp_path / "data"), features=["density", "sh"], compact=compact)
    rows_key = "links" if compact else "coordinates"

    ds = Co3DDataset(train_transformations=pre + ["FarthestPointSample", "RandomScale"], **kw)
    samples = [ds[0], ds[1]]
    for s, n in zip(samples, kept):
        assert s[rows_key].shape[0] == n and s["sample_points"] == 32 and 0 <= s["fps_start"] < n and "sample_rows" not in s
        assert s["aug_params"].shape == (44,)  # the stages behind the sampler still make a program
    batch = collate_mink(samples)
    assert batch["fps_start"].dtype == torch.int32 and batch["fps_start"].tolist() == [s["fps_start"] for s in samples]
    assert batch["sample_points"] == 32 and batch["sample_n_max"] == max(kept) and "sample_rows" not in batch
    assert batch["scene_offsets"].tolist() == [0, kept[0], kept[0] + kept[1]] and batch["aug_params"].shape == (2, 44)

    ds = Co3DDataset(train_transformations=pre + ["RandomSample"], **kw)
    assert (ds.transformations is None) == (not density)  # the sampler is no stage of the program; the row filter stays in it
    samples = [ds[0], ds[1]]
    for s, n in zip(samples, kept):
        assert s["sample_rows"].shape == (400,) and s["sample_rows"].max() < n and "fps_start" not in s
        assert set(s["sample_rows"].tolist()) <= set(range(n))  # 400 picks of fewer rows: with replacement
    batch = collate_mink(samples)
    assert batch["sample_rows"].dtype == torch.int64 and batch["sample_rows"].shape == (2, 400)
    assert torch.equal(batch["sample_rows"][1], torch.from_numpy(samples[1]["sample_rows"]) + kept[0])  # global rows
    assert batch["scene_offsets"].tolist() == [0, kept[0], kept[0] + kept[1]] and batch["sample_points"] == 400
    # eval phase: its own list
    ev = Co3DDataset(**dict(kw, phase="val"), train_transformations=["RandomSample"], eval_transformations=[])
    assert ev.sampler is None and "sample_points" not in ev[0]


def test_ordering_rules_and_unknown_names(tmp_path, monkeypatch):
    from nerf_downstream_amd.co3d_3d.src.data.co3d import Co3DDataset
    from nerf_downstream_amd.co3d_3d.src.data.sampling import split_recipe
    from nerf_downstream_amd.co3d_3d.src.data.staging import DirectCompactLoader

    write_scenes(tmp_path)
    monkeypatch.chdir(tmp_path)
    gin.parse_config("FarthestPointSample.num_points = 8\nRandomSample.num_points = 8")
    kw = dict(phase="train", data_root=str(tmp_path / "data"), features=["sh"])
    for bad in (["RandomRotation", "FarthestPointSample"], ["RandomScale", "RandomSample", "RandomRotation"],
                ["FarthestPointSample", "RandomSample"], ["RandomSample", "RandomSample"], ["FarthestPointSample", "FarthestPointSample"],
                ["FarthestPointSample", "DensityBasedSample"], ["CoordinateDropout", "RandomSample"],
                ["DensityBasedSample", "RandomFeatureJitter", "FarthestPointSample"]):
        with pytest.raises(NotImplementedError, match="FarthestPointSample / RandomSample"):
            Co3DDataset(train_transformations=bad, **kw)
    for bad in (["ElasticDistortion"], ["FarthestPointSample", "ElasticDistortion"], ["LabelBasedSample"], ["NoSuchThing", "RandomSample"]):
        with pytest.raises(NotImplementedError, match="have no GPU counterpart"):
            Co3DDataset(train_transformations=bad, **kw)
    assert split_recipe(["DensityBasedSample", "RandomSample", "RandomScale"]) == (["DensityBasedSample", "RandomScale"], "RandomSample")
    assert split_recipe(["RandomScale"]) == (["RandomScale"], None) and split_recipe([]) == ([], None)
    ok = Co3DDataset(train_transformations=["DensityBasedSample", "FarthestPointSample", "RandomRotation", "RandomFeatureJitter"], **kw)
    assert type(ok.sampler).__name__ == "FarthestPointSample" and [type(t).__name__ for t in ok.transformations.transforms] == [
        "DensityBasedSample", "RandomRotation", "RandomFeatureJitter"]
    assert Co3DDataset(train_transformations=["RandomScale"], **kw).sampler is None
    # the direct pinned loader builds batches without collate_mink: it must step aside for a recipe with a sampler
    assert not DirectCompactLoader.usable(Co3DDataset(train_transformations=["RandomSample"], compact=True, **kw))


def test_data_module_keeps_refusing_collate_pointnet():
    from nerf_downstream_amd.co3d_3d.src.data.data_module import DataModule

    with pytest.raises(ValueError, match="collate_pointnet"):
        DataModule(collate_func_name="collate_pointnet")


# ------------------------------------------------------------------------------------------------------------ the C ABI
def test_header_thresholds_are_the_bound_ones():
    from nerf_downstream_amd import _lib

    text = open(os.path.join(ROOT, "include", "mink_hip.h")).read()
    val = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))  # noqa: E731
    assert (val("MINK_FPS_XYZ_REG_ROWS_SMALL"), val("MINK_FPS_XYZ_REG_ROWS"), val("MINK_FPS_DIST_REG_ROWS")) == (
        _lib.FPS_XYZ_REG_ROWS_SMALL, _lib.FPS_XYZ_REG_ROWS, _lib.FPS_DIST_REG_ROWS)
    assert (val("MINK_FPS_EMPTY_SCENE"), val("MINK_FPS_BAD_START"), val("MINK_FPS_SCENE_TOO_LARGE")) == (
        _lib.FPS_EMPTY_SCENE, _lib.FPS_BAD_START, _lib.FPS_SCENE_TOO_LARGE)
    assert _lib.FPS_XYZ_REG_ROWS_SMALL < _lib.FPS_XYZ_REG_ROWS < _lib.FPS_DIST_REG_ROWS
    assert all(v % val("MINK_FPS_THREADS") == 0 for v in (_lib.FPS_XYZ_REG_ROWS_SMALL, _lib.FPS_XYZ_REG_ROWS, _lib.FPS_DIST_REG_ROWS))


def test_fps_arguments_are_refused_before_any_launch():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced: every call below is refused before a launch
    big = _lib.FPS_DIST_REG_ROWS + 1
    ok = dict(xyz=P, n=100, ld=3, off=P, start=P, B=2, m=8, n_max=100, idx=P, status=P, ws=None, ws_bytes=0)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mink_fps_scenes(a["xyz"], a["n"], a["ld"], a["off"], a["start"], a["B"], a["m"], a["n_max"], a["idx"], a["status"],
                                 a["ws"], a["ws_bytes"], None)

    for kw, word in (({"xyz": None}, b"NULL"), ({"off": None}, b"NULL"), ({"start": None}, b"NULL"), ({"idx": None}, b"NULL"),
                     ({"status": None}, b"NULL"), ({"ld": 2}, b"ld = 2"), ({"ld": 4097}, b"ld = 4097"), ({"m": 0}, b"m = 0"),
                     ({"m": -3}, b"m = -3"), ({"B": 0}, b"B = 0"), ({"n": 0}, b"bad shape"), ({"n_max": 0}, b"bad shape"),
                     ({"n_max": 101}, b"bad shape"), ({"B": 1 << 20, "m": 1 << 11}, b"bad shape"),
                     ({"n": big, "n_max": big}, b"workspace of 0 bytes"),
                     ({"n": big, "n_max": big, "ws": P, "ws_bytes": 2 * big * 4 - 1}, b"workspace of"),
                     ({"n": big, "n_max": big, "ws": None, "ws_bytes": 2 * big * 4}, b"workspace of")):
        assert call(**kw) == -1, kw
        assert word in L.mink_last_error(), (kw, L.mink_last_error())
    assert L.mink_fps_workspace_bytes(_lib.FPS_DIST_REG_ROWS, 16) == 0 and L.mink_fps_workspace_bytes(1, 1) == 0
    assert L.mink_fps_workspace_bytes(big, 3) == 3 * big * 4 and L.mink_fps_workspace_bytes(big, 0) == 0
    assert L.mink_abi_version() == 4


def test_status_words_raise():
    from nerf_downstream_amd import _lib
    from nerf_downstream_amd.minkowski.utils import SampleSceneError, fps_status_check

    fps_status_check(0)
    for bits, word in ((_lib.FPS_EMPTY_SCENE, "empty scene"), (_lib.FPS_BAD_START, "first pick outside"),
                       (_lib.FPS_SCENE_TOO_LARGE, "n_max"), (_lib.FPS_EMPTY_SCENE | _lib.FPS_BAD_START, "empty scene")):
        with pytest.raises(SampleSceneError, match=word):
            fps_status_check(torch.tensor([bits], dtype=torch.int32))


def test_row_gather_keeps_pick_order():
    from nerf_downstream_amd.minkowski.utils import sample_scene_rows

    coords = torch.arange(7 * 4, dtype=torch.int32).view(7, 4)
    feats = torch.arange(7 * 2, dtype=torch.float32).view(7, 2)
    idx = torch.tensor([[2, 0, 2], [6, 4, 5]])
    c, f, off = sample_scene_rows(coords, feats, idx)
    assert torch.equal(c, coords[[2, 0, 2, 6, 4, 5]]) and torch.equal(f, feats[[2, 0, 2, 6, 4, 5]])
    assert off.dtype == torch.int32 and off.tolist() == [0, 3, 6]


# ------------------------------------------------------------------------------------------------------------ the CPU backend
@pytest.mark.parametrize("which", ["FarthestPointSample", "RandomSample"])
def test_process_input_samples_on_the_cpu_backend(tmp_path, monkeypatch, which):
    """The sampler stage of process_input through the oracle namespace: 48 rows per scene, the ones the plan names (the
    restatement's picks on the voxel coordinates for the farthest-point sampler), features gathered with them."""
    from nerf_downstream_amd.co3d_3d.src.data.co3d import Co3DDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from oracle import me_cpu as OME

    raw = write_scenes(tmp_path)
    monkeypatch.chdir(tmp_path)
    gin.parse_config("FarthestPointSample.num_points = 48\nRandomSample.num_points = 48")
    ds = Co3DDataset(phase="train", data_root=str(tmp_path / "data"), features=["density", "sh"], train_transformations=[which])
    batch = collate_mink([ds[0], ds[1]])
    full_c, full_f = batch["coordinates"].clone(), batch["features"].clone()
    if which == "RandomSample":
        rows = batch["sample_rows"].reshape(-1)
    else:
        xyz = np.concatenate([coords_of(r["links"]) for r in raw])
        rows = torch.from_numpy(FR.fps_batch(xyz, [0, 300, 657], 48, batch["fps_start"].tolist())).reshape(-1)
        assert len(set(rows.tolist())) == 96  # distinct voxels: no row twice
    model = get_model("ResNet14", 28, 51, ME=OME)
    field = model.process_input(batch)
    assert field.C.shape[0] == 96 and torch.equal(field.C[:, 0], torch.arange(2).repeat_interleave(48).to(field.C.dtype))
    assert torch.equal(field.C.float(), full_c[rows]) and torch.equal(field.F, full_f[rows])


def test_one_cpu_trainer_step_with_random_sample(tmp_path, monkeypatch):
    from nerf_downstream_amd.co3d_3d.train import train
    from oracle import me_cpu as OME

    write_scenes(tmp_path, sizes=(300, 357, 280, 330))
    monkeypatch.chdir(tmp_path)
    gin.parse_config_files_and_bindings(
        [f"{CFG}/co3d_cls.gin", f"{CFG}/resnet14.gin", f"{CFG}/feature_shdensity.gin"],
        ["train.gpus=0", "train.max_steps=1", "train.val_every_n_steps=1", "train.log_every_n_steps=1", "train.batch_size=2",
         "train.val_batch_size=2", "train.train_num_workers=0", "train.val_num_workers=0", "train.loggers=['csv']", "train.lr=0.01",
         f"Co3DDatasetBase.data_root='{tmp_path / 'data'}'", "Co3DDatasetBase.train_transformations=['RandomSample']",
         "Co3DDatasetBase.eval_transformations=['RandomSample']", "RandomSample.num_points=96"])
    seen = []
    model_cls = __import__("nerf_downstream_amd.co3d_3d.src.models.mink.base_model", fromlist=["x"]).MinkowskiBaseModel
    orig = model_cls.process_input

    def spy(self, batch, *a, **k):
        field = orig(self, batch, *a, **k)
        seen.append(int(field.C.shape[0]))
        return field

    monkeypatch.setattr(model_cls, "process_input", spy)
    res = train(save_path=str(tmp_path / "run"), resume_training=False, run_name="t", run_name_postfix=None, ME=OME)
    assert res["global_step"] == 1
    logged = [h for h in res["history"] if "train/loss" in h]
    assert len(logged) == 1 and np.isfinite(logged[0]["train/loss"])
    assert any("val/acc1" in h for h in res["history"])
    assert seen and all(n == 2 * 96 for n in seen)  # every batch, training and validation, reached the model with 96 rows per scene
