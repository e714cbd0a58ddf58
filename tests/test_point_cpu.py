"""CPU: the point-based classifiers' registry, state-dict layout, dataset and config, and the float64 restatement of the
field map (tests/point_restate.py) against a brute-force search on the shared two-clouds case."""
import os
import sys

import numpy as np
import pytest
import torch

import point_restate as PT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GIN = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs", "modelnet40_cls.gin")

BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _mlp(name):
    return [f"{name}.0.linear.weight"] + [f"{name}.1.bn.{k}" for k in BN]


def _conv(name):
    return [f"{name}.0.kernel"] + [f"{name}.1.bn.{k}" for k in BN]


# read off the reference's fcnn.py:64-129 / pointnet.py:63-98: module order is registration order
FCNN_KEYS = (_mlp("mlp1") + _conv("conv1") + _conv("conv2") + _conv("conv3") + _conv("conv4") + _conv("conv5.0") + _conv("conv5.1")
             + _conv("conv5.2") + _mlp("final.1") + _mlp("final.3") + ["final.4.linear.weight", "final.4.linear.bias"])
POINTNET_KEYS = (_mlp("conv1") + _mlp("conv2") + _mlp("conv3") + _mlp("conv4") + _mlp("conv5") + _mlp("linear1")
                 + ["linear2.linear.weight", "linear2.linear.bias"])
# in_channel 3, out_channel 40, the constructor defaults (channels (32, 48, 64, 96, 128), embedding 1024, kernel 3):
#   mlp1 3*32 + 64 | conv1..4 27*cin*cout + 2*cout | conv5 27*336*256, 27*256*512, 27*512*1024 (+ 2*cout) |
#   final 2048*512 + 1024, 512*512 + 1024, 512*40 + 40
FCNN_PARAMS = (160 + 41568 + 83072 + 166080 + 332032 + 2322944 + 3539968 + 14157824 + 1049600 + 263168 + 20520)
#   3*64 + 128, 64*64 + 128 (twice), 64*128 + 256, 128*1024 + 2048, 1024*512 + 1024, 512*40 + 40
POINTNET_PARAMS = 320 + 4224 + 4224 + 8448 + 133120 + 525312 + 20520


@pytest.mark.parametrize("name,keys,count", [("MinkowskiFCNN", FCNN_KEYS, FCNN_PARAMS), ("MinkowskiSplatFCNN", FCNN_KEYS, FCNN_PARAMS),
                                             ("MinkowskiPointNet", POINTNET_KEYS, POINTNET_PARAMS)])
def test_models_construct_with_the_reference_state_dict_layout(name, keys, count):
    from nerf_downstream_amd.co3d_3d.src.models import MODELS, get_model

    assert name in MODELS
    model = get_model(name, 3, 40)
    assert type(model).__name__ == name
    assert list(model.state_dict().keys()) == keys
    assert sum(p.numel() for p in model.parameters()) == count == (696168 if name == "MinkowskiPointNet" else 21976936)
    convs = [m for m in model.modules() if type(m).__name__ == "MinkowskiConvolution"]
    if name != "MinkowskiPointNet":
        assert [(c.kernel_size, c.stride) for c in convs] == [(3, 1), (3, 2), (3, 2), (3, 2), (3, 2), (3, 2), (3, 2)]
        k = convs[-1].kernel  # kaiming normal, fan_out: std = sqrt(2 / (27 * cout))
        assert abs(float(k.detach().std()) / (2.0 / (27 * 1024)) ** 0.5 - 1) < 0.02
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            assert bool((m.weight == 1).all()) and bool((m.bias == 0).all())


def test_constructor_arguments_follow_the_reference():
    from nerf_downstream_amd.co3d_3d.src.models.mink.fcnn import MinkowskiFCNN
    from nerf_downstream_amd.co3d_3d.src.models.mink.pointnet import MinkowskiPointNet

    net = MinkowskiFCNN(3, 5, kernel_size=3, embedding_channel=32, channels=(8, 12, 16, 24, 32))
    assert net.conv5[0][0].kernel.shape == (27, 12 + 16 + 24 + 32, 8) and net.conv5[2][0].kernel.shape == (27, 16, 32)
    assert net.final[1][0].linear.weight.shape == (512, 64) and net.final[4].linear.weight.shape == (5, 512)
    assert MinkowskiPointNet(3, 5, embedding_channel=32).conv5[0].linear.weight.shape == (32, 128)


def _write_shards(root, phase, sizes, seed):
    rng = np.random.default_rng(seed)
    out = []
    for i, m in enumerate(sizes):
        data = rng.uniform(-1, 1, size=(m, 64, 3)).astype(np.float32)
        label = rng.integers(0, 40, size=(m, 1)).astype(np.uint8)
        np.savez(os.path.join(root, f"ply_data_{phase}{i}.npz"), data=data, label=label)
        out.append((data, label))
    return out


def test_modelnet40_dataset_reads_npz_shards(tmp_path):
    from nerf_downstream_amd.co3d_3d.src.data.datasets import DATASETS
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink

    cls = DATASETS["ModelNet40H5Dataset"]
    root = str(tmp_path)
    train = _write_shards(root, "train", (5, 3), 1)
    test = _write_shards(root, "test", (2, 2), 2)
    ds = cls("train", data_root=root, train_transformations=[], eval_transformations=[], num_points=48, voxel_size=0.05)
    assert len(ds) == 8
    s = ds[6]
    assert set(s) == {"coordinates", "features", "labels"}
    assert s["features"].dtype == np.float32 and s["features"].shape == (48, 3)  # num_points truncates
    assert np.array_equal(s["features"], train[1][0][1][:48])
    assert np.array_equal(s["coordinates"], s["features"] / np.float32(0.05))
    assert s["labels"].dtype == np.int64 and s["labels"].tolist() == train[1][1][1].tolist()
    for phase in ("val", "test"):  # both read the test shards
        dv = cls(phase, data_root=root, train_transformations=["CoordinateDropout"], eval_transformations=[], voxel_size=0.1)
        assert len(dv) == 4 and dv.transformations is None
        assert np.array_equal(dv[2]["features"], test[1][0][0])
    batch = collate_mink([ds[0], ds[1]])
    assert batch["coordinates"].shape == (96, 4) and batch["coordinates"].dtype == torch.float32
    assert batch["coordinates"][:, 0].tolist() == [0.0] * 48 + [1.0] * 48 and batch["labels"].shape == (2,)


def test_modelnet40_train_transforms_run_on_the_host(tmp_path):
    from nerf_downstream_amd.co3d_3d.src.data import modelnet40, transforms

    xyz = np.random.default_rng(0).uniform(-1, 1, size=(50, 3)).astype(np.float32)
    out = modelnet40.apply_stages(xyz, [("translate", np.array([0.5, 0.0, -1.0])), ("linear", np.eye(3) * 2.0)])
    assert np.allclose(out, (xyz + np.float32([0.5, 0, -1])) * 2, atol=1e-6)
    np.random.seed(0)
    kept = modelnet40.apply_stages(xyz, [("dropout", 0.2)])
    assert kept.shape == (40, 3) and len({tuple(r) for r in kept.tolist()} - {tuple(r) for r in xyz.tolist()}) == 0
    with pytest.raises(NotImplementedError, match="flip"):
        modelnet40.apply_stages(xyz, [("flip", (0, 1))])
    _write_shards(str(tmp_path), "train", (3,), 3)
    ds = modelnet40.ModelNet40H5Dataset("train", data_root=str(tmp_path), voxel_size=0.05,
                                        train_transformations=["CoordinateUniformTranslation", "RandomScale", "CoordinateDropout"])
    assert isinstance(ds.transformations, transforms.Compose)
    s = ds[0]
    assert s["features"].shape[0] in (64, 51) and np.allclose(s["coordinates"], s["features"] / np.float32(0.05))
    shift = s["features"][:3] - ds.data[0][:3]
    assert s["features"].shape[0] != 64 or float(np.abs(shift).max()) <= 0.2 * 1.1 + 0.1 * 1.0  # translated by <= 0.2, scaled by <= 10 %


def test_modelnet40_named_errors(tmp_path, monkeypatch):
    from nerf_downstream_amd.co3d_3d.src.data.modelnet40 import ModelNet40H5Dataset

    missing = str(tmp_path / "nowhere")
    with pytest.raises(FileNotFoundError, match="nowhere"):
        ModelNet40H5Dataset("train", data_root=missing)
    with pytest.raises(FileNotFoundError, match="ply_data_train"):
        ModelNet40H5Dataset("train", data_root=str(tmp_path))
    (tmp_path / "ply_data_train0.h5").write_bytes(b"")
    monkeypatch.setitem(sys.modules, "h5py", None)  # `import h5py` raises ImportError
    with pytest.raises(ImportError, match=r"h5py.*\.npz"):
        ModelNet40H5Dataset("train", data_root=str(tmp_path))


def test_modelnet40_config_parses():
    from nerf_downstream_amd import gin_lite as gin
    from nerf_downstream_amd.co3d_3d.src.data.datasets import get_dataset
    from nerf_downstream_amd.co3d_3d.src.models import MODELS

    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings([GIN], [])
        assert get_dataset().__name__ == "ModelNet40H5Dataset"
        assert MODELS[gin.query_parameter("get_model.name")].__name__ == "MinkowskiFCNN"
        q = gin.query_parameter
        assert (q("get_model.in_channel"), q("get_model.out_channel")) == (3, 40)
        assert q("ModelNet40H5Dataset.voxel_size") == 0.05 and q("ModelNet40H5Dataset.eval_transformations") == []
        assert q("ModelNet40H5Dataset.train_transformations") == ["CoordinateUniformTranslation", "RandomScale", "CoordinateDropout"]
        assert q("ModelNet40H5Dataset.data_root") == "./datasets/modelnet40_ply_hdf5_2048/"
        assert q("RandomScale.scale_ratio") == 0.05 and q("CoordinateUniformTranslation.max_translation") == 0.2
        assert q("train.training_module") == "ClassificationTraining" and q("train.monitor_metric") == "val/acc1"
        assert (q("train.optimizer_name"), q("SGD.momentum"), q("train.lr"), q("train.weight_decay")) == ("SGD", 0.9, 0.1, 1e-4)
        assert q("train.scheduler_name") == "CosineAnnealingLR"
        assert (q("train.batch_size"), q("train.val_batch_size"), q("train.max_steps"), q("train.val_every_n_steps")) == (32, 16, 100000, 500)
    finally:
        gin.clear_config()


def test_two_clouds_case_and_field_map_restatement():
    coords, feats = PT.two_clouds()
    assert coords.shape == (260, 4) and feats.shape == (260, 3) and coords.dtype == torch.float32
    assert coords[:, 0].tolist() == [0.0] * 193 + [1.0] * 67
    assert float(coords[0, 1]) == -16.0 and float(coords[1, 1]) == -0.25
    assert float(coords[:, 1:].min()) >= -24 and float(coords[:, 1:].max()) < 24
    vox, inv = PT.quantise(coords)
    assert vox.shape[0] < coords.shape[0]  # the stride-1 level has fewer voxels than points
    assert vox.shape[0] <= 260 - 30 + 2 and torch.equal(vox[inv][:, 1:], coords[:, 1:].double().floor().long())
    for ts in (1, 2, 4, 8, 16, 32, 64, 128):
        lev = PT.level(coords, ts)
        per_sample = torch.bincount(lev[:, 0], minlength=2)
        assert int(per_sample.min()) >= 2, (ts, per_sample.tolist())  # every level has at least 2 voxels per sample
        idx = PT.field_map(coords, lev, ts)
        assert torch.equal(idx, PT.field_map_brute(coords, lev, ts)), ts
        assert int(idx.min()) >= 0  # every point lies in a voxel of every level derived from the field
        assert torch.equal(lev[idx][:, 0], coords[:, 0].long())
    lev8 = PT.level(coords, 8)
    assert PT.field_key((0.0, -16.0, 3.5, -0.25), 8) == (0, -16, 0, -8) and PT.field_key((0.0, -0.25, 0, 0), 128) == (0, -128, 0, 0)
    # a batch index without voxels, and a level that lost a voxel, find nothing
    far = torch.tensor([[7.0, 1.0, 1.0, 1.0]])
    assert PT.field_map(far, lev8, 8).tolist() == [-1] == PT.field_map_brute(far, lev8, 8).tolist()
    cut = PT.field_map(coords, lev8[1:], 8)
    assert torch.equal(cut, PT.field_map_brute(coords, lev8[1:], 8)) and int((cut < 0).sum()) >= 1
    # explicit backward formulas against autograd
    x = torch.randn(lev8.shape[0] - 1, 5, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(260, 5, dtype=torch.float64)
    PT.gather_fwd(x, cut).backward(dy)
    assert torch.allclose(x.grad, PT.gather_bwd(dy, cut, x.shape[0]), atol=1e-12)
    f = torch.randn(260, 5, dtype=torch.float64, requires_grad=True)
    dv = torch.randn(vox.shape[0], 5, dtype=torch.float64)
    PT.voxel_mean(f, inv, vox.shape[0]).backward(dv)
    assert torch.allclose(f.grad, PT.mean_bwd(dv, inv, vox.shape[0]), atol=1e-12)
