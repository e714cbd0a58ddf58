"""Segmentation augmentation without a GPU: the float64 restatement against scipy and the reference's crop rules, the
folded MINK_SEGAUG_* program against the stage-by-stage evaluation, the host-side noise-grid bound, and the dataset /
config plumbing of `PlenoxelScannetDataset(device_augmentation=True)`."""
import os
import random

import numpy as np
import pytest

from seg_restate import (blur, canonical, crop_rows, elastic_dims, grid_noise, row_coins, stagewise, trilinear)

CFG = os.path.join(os.path.dirname(__file__), "..", "nerf_downstream_amd", "co3d_3d", "configs")


def _recipe(**over):
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    kw = dict(crop=dict(x=200, y=200, z=200), affine=dict(upright_axis="y", application_ratio=0.7),
              elastic=dict(distortion_params=[(4, 16)], application_ratio=0.7))
    kw.update(over)
    return [S.RandomRotation(upright_axis="y"), S.RandomCrop(**kw["crop"]), S.RandomAffine(**kw["affine"]),
            S.CoordinateDropout(), S.RandomFeatureJitter(), S.RandomHorizontalFlip(upright_axis="y"), S.RandomTranslation(),
            S.ElasticDistortion(**kw["elastic"])]


def _scene(rng, n, extent):
    return (rng.random((n, 3)) * extent - extent / 2).astype(np.float32)


def test_blur_and_interpolation_match_scipy():
    """The restatement's smoothing and interpolation = the reference's scipy calls (transforms.py:550-585) on one grid."""
    import scipy.interpolate
    import scipy.ndimage

    rng = np.random.default_rng(0)
    noise = rng.normal(size=(7, 5, 9, 3))
    want = noise.copy()
    kx, ky, kz = np.ones((3, 1, 1, 1)) / 3, np.ones((1, 3, 1, 1)) / 3, np.ones((1, 1, 3, 1)) / 3
    for _ in range(2):
        for k in (kx, ky, kz):
            want = scipy.ndimage.convolve(want, k, mode="constant", cval=0)
    got = blur(noise)
    assert np.abs(got - want).max() < 1e-12
    lo, g, dims = np.array([-3.25, 10.0, 0.5]), 4.0, np.array(noise.shape[:3])
    ax = [np.linspace(a, a + g * (d - 1), d) for a, d in zip(lo - g, dims)]
    interp = scipy.interpolate.RegularGridInterpolator(ax, got, bounds_error=False, fill_value=0)
    pts = lo - g + rng.random((4000, 3)) * (dims - 1) * g * 1.2 - 0.1 * g * (dims - 1)  # some beyond the grid
    pts = np.concatenate([pts, lo - g + np.stack(np.meshgrid(*[np.arange(d) for d in dims], indexing="ij"), -1).reshape(-1, 3) * g])
    assert np.abs(trilinear(got, lo, g, pts) - interp(pts)).max() < 1e-12


def _reference_crop(c, size, max_retries):
    """The reference's RandomCrop loop (:204-244), drawing lazily from np.random."""
    norm = c - c.min(0, keepdims=True)
    rng = np.clip(norm.max(0, keepdims=True) - size, 0, np.inf)
    if np.prod(rng == 0):
        return np.ones(len(c), bool)
    for _ in range(max_retries):
        lo = np.random.rand(1, 3) * rng
        sel = np.logical_and(np.prod(norm > lo, 1), np.prod(norm < lo + size, 1))
        if np.sum(sel) > 0:
            return sel.astype(bool)
    return np.ones(len(c), bool)


def test_crop_rules_match_reference():
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    rng = np.random.default_rng(1)
    crop = S.RandomCrop(50, 50, 50, max_retries=10)
    size = np.array([[50.0, 50.0, 50.0]])
    cases = [_scene(rng, 3000, np.array([200.0, 120.0, 80.0])),     # crops
             _scene(rng, 500, np.array([40.0, 30.0, 45.0])),        # smaller than the crop: every range 0, no crop
             _scene(rng, 500, np.array([40.0, 300.0, 45.0])),       # one axis larger: crops along it only
             np.array([[0, 0, 0], [1000, 1000, 1000]], np.float32)]  # every box empty: no crop
    for c in cases:
        c = c.astype(np.float64)
        np.random.seed(7)
        want = _reference_crop(c, size, 10)
        np.random.seed(7), random.seed(0)
        stages = []
        crop.draw(stages)
        got = crop_rows(c, stages[0][1][None], stages[0][2])
        assert np.array_equal(got, want)
    assert crop_rows(cases[1].astype(np.float64), size, np.random.rand(10, 3)).all()
    assert crop_rows(cases[3].astype(np.float64), size, np.random.rand(10, 3)).all()
    # strict inequalities: a row on a face of the box is outside
    c = np.array([[0, 0, 0], [10, 10, 10], [59, 10, 10], [60, 10, 10], [100, 100, 100]], np.float64)
    u = np.array([[0.2, 0.0, 0.0]])  # range 50 per axis: box x in (10, 60), y and z in (0, 50)
    assert crop_rows(c, size, u).tolist() == [False, False, True, False, False]


def _random_recipe(rng):
    """A recipe of the supported form: the reference's stages, some dropped, linear / translate stages inserted anywhere
    before the elastic stage."""
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    base = _recipe(crop=dict(x=60, y=50, z=70, max_retries=4))
    for t in base:
        t.application_ratio = 1.0
    keep = [t for t in base if rng.random() < 0.75]
    for _ in range(int(rng.integers(0, 3))):
        extra = S.RandomScale(scale_ratio=0.3) if rng.random() < 0.5 else S.CoordinateUniformTranslation(max_translation=5)
        extra.application_ratio = 1.0
        last = len(keep) - (1 if keep and isinstance(keep[-1], S.ElasticDistortion) else 0)
        keep.insert(int(rng.integers(0, last + 1)), extra)
    return keep


def test_folded_program_equals_stagewise():
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    rng = np.random.default_rng(2)
    random.seed(2), np.random.seed(2)
    seed = 0x1234567890ABCDEF
    for trial in range(60):
        comp = S.SegCompose(_random_recipe(rng))
        c = _scene(rng, 800, np.array([150.0, 90.0, 120.0]))
        stages = comp.draw()
        P = S.compile_seg_program(stages, c.max(0) - c.min(0))
        stream = int(rng.integers(0, 2 ** 32))
        coin = row_coins(len(c), stream, seed)
        keep, r = canonical(c, P, coin)
        no_elastic = [s for s in stages if s[0] != "elastic"]
        want_c, _, rows = stagewise(c, np.zeros((len(c), 1)), no_elastic, stream, seed, [-1])
        assert np.array_equal(np.flatnonzero(keep), rows), (trial, stages)
        assert np.abs(r - want_c).max() < 1e-9, trial


@pytest.mark.parametrize("order", [
    ["RandomCrop", "CoordinateDropout", "RandomCrop"],
    ["CoordinateDropout", "RandomCrop"],
    ["RandomHorizontalFlip", "RandomCrop"],
    ["ElasticDistortion", "RandomTranslation"],
    ["ElasticDistortion", "RandomFeatureJitter"],
    ["RandomHorizontalFlip", "RandomHorizontalFlip"],
    ["CoordinateDropout", "CoordinateDropout"],
    ["CoordinateJitter"],
])
def test_unsupported_orders_raise(order):
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S
    from nerf_downstream_amd.co3d_3d.src.data import transforms as T

    def make(name):
        return S.RandomCrop(10, 10, 10) if name == "RandomCrop" else (getattr(S, name, None) or getattr(T, name))()

    with pytest.raises(NotImplementedError):
        S.SegCompose([make(n) for n in order])
    stages = []
    for n in order:  # the same orders as drawn stage lists
        t = make(n)
        t.application_ratio = 1.0
        t.draw(stages)
    with pytest.raises(NotImplementedError):
        S.compile_seg_program(stages)


def test_supported_orders_compile():
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    S.SegCompose(_recipe())
    S.SegCompose([S.RandomCrop(5, 5, 5), S.RandomHorizontalFlip(), S.CoordinateDropout(), S.RandomScale(), S.ElasticDistortion()])
    S.SegCompose([S.RandomTranslation(), S.ElasticDistortion()])


def test_grid_bound_covers_actual_dims():
    """The host bound of every elastic grid >= the dims the stagewise evaluation builds, on random programs and scenes."""
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    rng = np.random.default_rng(3)
    random.seed(3), np.random.seed(3)
    seed = 99
    checked = 0
    for trial in range(80):
        comp = S.SegCompose(_recipe(crop=dict(x=40, y=40, z=40), elastic=dict(distortion_params=[(4, 16), (2, 24)], application_ratio=1.0)))
        ext = rng.random(3) * 120 + 5
        c = _scene(rng, 400, ext)
        stages = comp.draw()
        P = S.compile_seg_program(stages, c.max(0) - c.min(0))
        bound = S.grid_bounds(P[None])[0]
        stream = int(rng.integers(0, 2 ** 32))
        el = [s for s in stages if s[0] == "elastic"]
        pre, _, _ = stagewise(c, np.zeros((len(c), 1)), [s for s in stages if s[0] != "elastic"], stream, seed, [-1])
        if not el or not len(pre):
            continue
        x = pre
        for e, (g, m) in enumerate(el[0][1]):
            d = elastic_dims(x, g)
            assert (d <= bound).all(), (trial, d, bound)
            x = x + trilinear(blur(grid_noise(d, e, stream, seed)), x.min(0), g, x) * m
            checked += 1
    assert checked > 40
    assert S.elastic_passes(np.zeros((2, S.SEG["PARAMS"]))) == 0


def test_scannet_dataset_emits_programs_only_when_asked(tmp_path):
    import torch

    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S
    from nerf_downstream_amd.co3d_3d.src.data.scannet import PlenoxelScannetDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink
    from test_train_cpu import _write_scannet_tree

    data_root, names, _, _ = _write_scannet_tree(tmp_path)
    recipe = ["RandomRotation", "RandomCrop", "RandomAffine", "CoordinateDropout", "RandomFeatureJitter", "RandomHorizontalFlip",
              "RandomTranslation", "ElasticDistortion"]
    plain = PlenoxelScannetDataset("train", data_root=str(data_root), features=["density", "sh"])
    assert not any(k.startswith("aug_") for k in plain[0])
    with pytest.raises(NotImplementedError):
        PlenoxelScannetDataset("train", data_root=str(data_root), train_transformations=recipe)
    from nerf_downstream_amd import gin_lite as gin

    gin.parse_config_files_and_bindings([], ["RandomCrop.x = 200", "RandomCrop.y = 200", "RandomCrop.z = 200"])
    try:
        ds = PlenoxelScannetDataset("train", data_root=str(data_root), features=["density", "sh"], train_transformations=recipe,
                                    device_augmentation=True)
        val = PlenoxelScannetDataset("val", data_root=str(data_root), features=["density", "sh"], train_transformations=recipe,
                                     device_augmentation=True)
        s = ds[1]
    finally:
        gin.clear_config()
    assert s["aug_params"].dtype == torch.float64 and s["aug_params"].shape == (S.SEG["PARAMS"],)
    xyz = s["coordinates"].numpy()
    assert np.allclose(s["aug_params"][S.SEG["EXTENT"]:S.SEG["EXTENT"] + 3].numpy(), xyz.max(0) - xyz.min(0))
    assert not any(k.startswith("aug_") for k in val[0])
    b = collate_mink([ds[0], ds[1]])
    assert b["aug_params"].shape == (2, S.SEG["PARAMS"]) and b["aug_streams"].dtype == torch.int32
    assert b["scene_offsets"].tolist() == [0, len(ds[0]["labels"]), len(ds[0]["labels"]) + len(ds[1]["labels"])]
    assert b["feature_names"] == ("density", "sh") and len(b["labels"]) == len(b["coordinates"])
    assert S.raw_columns(["density", "sh"]) == [4] + list(range(5, 32))
    with pytest.raises(NotImplementedError):
        PlenoxelScannetDataset("train", data_root=str(data_root), features=["xyzs"], train_transformations=["RandomRotation"],
                               device_augmentation=True)


def test_scannet_aug_config_parses():
    from nerf_downstream_amd import gin_lite as gin
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S
    import nerf_downstream_amd.co3d_3d.train  # noqa: F401  (registers the configurables)

    gin.parse_config_files_and_bindings([f"{CFG}/scannet_plenoxel_aug.gin", f"{CFG}/res16unet.gin"], [])
    try:
        crop, el, aff = S.RandomCrop(), S.ElasticDistortion(), S.RandomAffine()
    finally:
        gin.clear_config()
    assert crop.max_size.tolist() == [200, 200, 200] and el.distortion_params == ((4.0, 16.0),) and el.application_ratio == 0.7
    assert aff.application_ratio == 0.7 and aff.upright_axis == 1


def test_co3d_accepted_set_unchanged():
    from nerf_downstream_amd.co3d_3d.src.data import transforms as T

    drawable = sorted(n for n in dir(T) if hasattr(getattr(T, n), "draw"))
    assert drawable == ["Compose", "CoordinateDropout", "CoordinateJitter", "CoordinateUniformTranslation", "DensityBasedSample",
                        "RandomAffine", "RandomFeatureJitter", "RandomHorizontalFlip", "RandomRotation", "RandomScale",
                        "RandomTranslation"]


def test_feature_jitter_start_must_not_be_negative():
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    with pytest.raises(ValueError):
        S.compile_seg_program([("feature_jitter", 0.01, -1, 27)])


def test_scannet_refuses_names_outside_the_program(tmp_path):
    from nerf_downstream_amd.co3d_3d.src.data.scannet import PlenoxelScannetDataset
    from test_train_cpu import _write_scannet_tree

    data_root, _, _, _ = _write_scannet_tree(tmp_path)
    for name in ("SegCompose", "Compose", "DensityBasedSample", "CoordinateJitter"):
        with pytest.raises(NotImplementedError):
            PlenoxelScannetDataset("train", data_root=str(data_root), train_transformations=[name], device_augmentation=True)
