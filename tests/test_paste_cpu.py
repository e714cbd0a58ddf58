"""The background paste without a GPU: tests/paste_restate.py against the recorded Pillow results (tests/golden/bkgd_pillow_v1.npz,
scripts/make_bkgd_golden.py) and against live Pillow where it imports; the rectangle's identities; `BackgroundAug.draw`; the
PeRFception train set's draws, samples and batches on written frames; the header section of `mink_img_paste` and the host check."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import paste_restate as R  # noqa: E402

from nerf_downstream_amd import gin_lite as gin  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", "bkgd_pillow_v1.npz")) as z:
        return {k: z[k] for k in z.files}


def _case(g, name):
    return g[f"{name}_fg"], g[f"{name}_mask"], g[f"{name}_bg"], tuple(int(v) for v in g[f"{name}_size"])


def test_restatement_equals_the_recorded_pillow_results(golden):
    names = [str(n) for n in golden["names"]]
    assert len(names) >= 20 and len(set(names)) == len(names)
    for name in names:
        fg, mask, bg, size = _case(golden, name)
        assert size == R.resized_size((fg.shape[1], fg.shape[0]), float(golden[f"{name}_scale"])), name
        got = R.paste(fg, mask, bg, size)
        assert got.dtype == np.uint8 and np.array_equal(got, golden[f"{name}_out"]), name
    # what the cases are there for
    sz = {n: tuple(int(v) for v in golden[f"{n}_size"]) for n in names}
    assert sz["one_pixel"] == (1, 1) and sz["both_passes_skipped"] == (64, 64) and sz["horizontal_skipped"] == (3, 52)
    assert golden["mask_of_another_size_mask"].shape != golden["mask_of_another_size_fg"].shape[:2]
    assert np.array_equal(golden["mask_all_0_out"], golden["mask_all_0_bg"])
    fg, _, bg, size = _case(golden, "mask_all_255")
    (hs, he, ws, we), (y0, x0) = R.geometry(bg.shape[:2], size[1], size[0])
    assert np.array_equal(golden["mask_all_255_out"][hs:he, ws:we], R.resize(fg, size)[y0:y0 + he - hs, x0:x0 + we - ws])
    parities = {((golden[f"{n}_bg"].shape[0] - sz[n][1]) % 2, (golden[f"{n}_bg"].shape[1] - sz[n][0]) % 2) for n in names}
    assert parities == {(0, 0), (0, 1), (1, 0), (1, 1)}


def test_all_255_frames_do_not_stay_255(golden):
    """255 * m + (1 - m) * 255 in float64 falls below 255 for many m and is truncated: the composite cannot be simplified."""
    assert (golden["all_255_fg"] == 255).all() and (golden["all_255_bg"] == 255).all()
    out = golden["all_255_out"]
    assert (out < 255).any() and (out >= 254).all()
    assert np.array_equal(R.paste(*_case(golden, "all_255")), out)


def test_restatement_equals_pillow_live(golden):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    for name in (str(n) for n in golden["names"]):
        fg, mask, bg, size = _case(golden, name)
        assert np.array_equal(R.resize(fg, size), np.asarray(Image.fromarray(fg).resize(size))), name
        assert np.array_equal(R.resize(mask, size), np.asarray(Image.fromarray(mask).resize(size))), name
    for (w, h), (rw, rh) in (((17, 9), (4, 3)), ((9, 17), (36, 68)), ((5, 70), (5, 17)), ((64, 3), (16, 3))):  # the range's ends
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        assert np.array_equal(R.resize(img, (rw, rh)), np.asarray(Image.fromarray(img).resize((rw, rh)))), (w, h, rw, rh)


def test_rectangle_identities():
    for b in range(1, 12):
        for r in range(1, 25):
            (hs, he, ws, we), (y0, x0) = R.geometry((b, b + 1), r, r + 2)
            assert he - hs == min(b, r) and we - ws == min(b + 1, r + 2)
            assert 0 <= hs and he <= b and 0 <= y0 and y0 + (he - hs) <= r
            assert 0 <= ws and we <= b + 1 and 0 <= x0 and x0 + (we - ws) <= r + 2
            assert hs == (max(b - r, 0)) // 2 and (r <= b or hs == 0)


def test_background_aug_draws_once():
    from nerf_downstream_amd.co3d_2d.src.data import transforms as T

    gin.clear_config()
    aug = T.BackgroundAug()
    np.random.seed(11)
    got = aug.draw((40, 30))
    after = np.random.random()
    np.random.seed(11)
    s = np.random.random() * (1.5 - 0.5) + 0.5
    assert got == (int(40 * s), int(30 * s)) and after == np.random.random()
    assert T.BackgroundAug((1.0, 1.0)).draw((7, 5)) == (7, 5)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        aug(None, None, None)
    for bad in ((0.2, 1.5), (0.5, 4.5), (1.5, 0.5)):
        with pytest.raises(ValueError, match="rescale_range"):
            T.BackgroundAug(bad)


SCENES = (("apple", "s1", (40, 30)), ("tv", "s2", (33, 47)), ("vase", "s3", (64, 64)))


def _write_scenes(tmp_path):
    """Three scenes of three renders each, with bg/ and mask/ beside fgbg/.  Every file is a PNG whatever its name says, so the
    decoded bytes are the written ones; the tv scene's masks have one band and half the render's size."""
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(6)
    root, lists = tmp_path / "data", tmp_path / "filelist"
    lists.mkdir()
    written = {}
    for cls, scene, (W, H) in SCENES:
        for sub in ("fgbg", "bg", "mask"):
            (root / cls / scene / sub).mkdir(parents=True)
        for f in range(3):
            fg = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            bg = rng.integers(0, 256, (H + 2, W + 1, 3), dtype=np.uint8)
            mask = rng.integers(0, 256, (H // 2, W // 2), dtype=np.uint8) if cls == "tv" else rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            Image.fromarray(fg).save(root / cls / scene / "fgbg" / f"image{f:03d}.png")
            Image.fromarray(bg).save(root / cls / scene / "bg" / f"image{f:03d}.jpg", format="PNG")
            Image.fromarray(mask).save(root / cls / scene / "mask" / f"mask{f:03d}.png")
            written[cls, f] = (fg, bg, mask if mask.ndim == 2 else mask[..., 0])
    for phase in ("train", "val", "test"):
        (lists / f"{phase}.txt").write_text("".join(f"{cls} {scene} 3\n" for cls, scene, _ in SCENES))
    return str(root), str(lists), written


def _dataset(root, lists, bkgd_aug):
    from nerf_downstream_amd.co3d_2d.src.data import loader as Ld

    gin.clear_config()
    ds = Ld.PeRFCeptionCo3DTrainDataset(bkgd_aug=bkgd_aug, data_root=root, filelist_root=lists, bkgd_on_device=True)
    ds.num_frames, ds.bkgd_frames = [3] * len(ds), 3  # (the reference draws among 50 frames; three were written)
    return ds


def _seed_with_p(below, bkgd_aug):
    """A numpy seed whose second draw (p) lies on the wanted side of bkgd_aug."""
    for seed in range(100):
        np.random.seed(seed)
        np.random.randint(3)
        if (np.random.random() < bkgd_aug) == below:
            return seed
    raise AssertionError


@pytest.mark.parametrize("pastes", [True, False])
def test_dataset_draws_in_the_reference_order(tmp_path, pastes):
    from nerf_downstream_amd.co3d_2d.src.data import loader as Ld
    from nerf_downstream_amd.co3d_2d.src.data import transforms as T

    root, lists, written = _write_scenes(tmp_path)
    ds = _dataset(root, lists, 0.5)
    seed = _seed_with_p(pastes, 0.5)
    np.random.seed(seed)
    s = ds[1]  # the tv scene: 33x47 renders
    follows = np.random.random()
    # the same stream by hand
    np.random.seed(seed)
    frame = np.random.randint(3)
    p = np.random.random()
    assert (p < 0.5) == pastes
    fg, _, mask = written["tv", frame]
    if pastes:
        scene, bg_frame = np.random.randint(3), np.random.randint(3)
        bg = written[SCENES[scene][0], bg_frame][1]
        rw, rh = T.BackgroundAug().draw((33, 47))
        assert torch.equal(s["image"], torch.from_numpy(bg)) and s["paste"]["size"] == (rw, rh)
        assert torch.equal(s["paste"]["fg"], torch.from_numpy(fg)) and torch.equal(s["paste"]["mask"], torch.from_numpy(mask))
        assert tuple(s["paste"]["mask"].shape) == (23, 16)
        size = (bg.shape[1], bg.shape[0])
    else:
        assert "paste" not in s and torch.equal(s["image"], torch.from_numpy(fg))
        size = (33, 47)
    draws = ds.augmix.draw(size, ds.transforms.draw)  # AugMix sees a frame of the background's size
    assert torch.equal(s["program"], torch.from_numpy(T.compile_program(draws)))
    assert follows == np.random.random() and int(s["labels"]) == Ld.CLASSES_IDX["tv"]


def test_batches_with_and_without_a_paste(tmp_path):
    from nerf_downstream_amd.co3d_2d.src.data import loader as Ld
    from nerf_downstream_amd.minkowski.utils import image_batch_check, image_paste_check

    root, lists, _ = _write_scenes(tmp_path)
    P = R.layout()
    # no sample pastes: a sample and a batch hold what those of the plain data set hold, key for key and byte for byte
    plain = Ld.PeRFCeptionCo3DTrainDataset(data_root=root, filelist_root=lists)
    plain.num_frames = [3] * 3
    never = _dataset(root, lists, 0.0)
    np.random.seed(40)
    a = [never[i] for i in range(3)]
    assert all(sorted(s) == sorted(plain[0]) == ["image", "labels", "program", "size"] for s in a)
    ba = Ld.collate_images(a)
    assert sorted(ba) == sorted(Ld.collate_images([plain[0]])) == ["labels", "offsets", "packed", "programs", "size", "sizes"]
    assert torch.equal(ba["packed"], torch.cat([s["image"].reshape(-1) for s in a])) and ba["packed"].dtype == torch.uint8
    assert ba["offsets"].tolist() == [0, 3600, 3600 + 4653, 3600 + 4653 + 12288] and ba["offsets"].dtype == torch.int64
    assert ba["sizes"].tolist() == [[40, 30], [33, 47], [64, 64]] and ba["sizes"].dtype == torch.int32
    assert torch.equal(ba["programs"], torch.stack([s["program"] for s in a])) and int(ba["size"]) == 224
    assert ba["labels"].tolist() == [Ld.CLASSES_IDX[c] for c, _, _ in SCENES]
    # a mixed batch
    always = _dataset(root, lists, 1.0)
    np.random.seed(5)
    samples = [always[0], never[1], always[2], always[1]]
    batch = Ld.collate_images(samples)
    assert sorted(batch) == ["labels", "offsets", "packed", "paste_fg", "paste_mask", "paste_table", "programs", "size", "sizes"]
    assert batch["sizes"].tolist() == [[s["image"].shape[1], s["image"].shape[0]] for s in samples]
    t = batch["paste_table"]
    assert t.dtype == torch.int64 and tuple(t.shape) == (4, P["PARAMS"]) and not t[1].any()
    fo = mo = 0
    for i in (0, 2, 3):
        ps = samples[i]["paste"]
        fh, fw = ps["fg"].shape[:2]
        mh, mw = ps["mask"].shape
        assert [int(t[i, P[k]]) for k in ("FG_OFFSET", "MASK_OFFSET", "FG_W", "FG_H", "MASK_W", "MASK_H", "RW", "RH")] == [
            fo, mo, fw, fh, mw, mh, ps["size"][0], ps["size"][1]]
        assert torch.equal(batch["paste_fg"][fo:fo + 3 * fw * fh].view(fh, fw, 3), ps["fg"])
        assert torch.equal(batch["paste_mask"][mo:mo + mw * mh].view(mh, mw), ps["mask"])
        fo, mo = fo + 3 * fw * fh, mo + mw * mh
    assert batch["paste_fg"].numel() == fo and batch["paste_mask"].numel() == mo
    assert image_batch_check(batch["offsets"].numpy(), batch["sizes"].numpy(), batch["programs"].numpy(), batch["packed"].numel()) == (4, 3)
    mw_, mh_ = image_paste_check(t.numpy(), batch["sizes"].numpy(), fo, mo)
    want = [(min(int(batch["sizes"][i, 0]), samples[i]["paste"]["size"][0]), min(int(batch["sizes"][i, 1]), samples[i]["paste"]["size"][1]))
            for i in (0, 2, 3)]
    assert (mw_, mh_) == (max(w for w, _ in want), max(h for _, h in want))


def test_bare_bkgd_aug_stays_refused(tmp_path):
    from nerf_downstream_amd.co3d_2d.src.data import loader as Ld

    root, lists, _ = _write_scenes(tmp_path)
    gin.clear_config()
    with pytest.raises(NotImplementedError, match="BackgroundAug.*bkgd_on_device"):
        Ld.PeRFCeptionCo3DTrainDataset(bkgd_aug=0.5, data_root=root, filelist_root=lists)


def test_bkgd_config_parses_after_the_frames_config():
    from nerf_downstream_amd.co3d_2d.src.data.loader import DataModule

    cfg = os.path.join(ROOT, "nerf_downstream_amd", "co3d_2d", "configs")
    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings([os.path.join(cfg, n) for n in ("resnet18.gin", "co3d_frames.gin", "perfception_bkgd.gin")], [])
        dm = DataModule()
        assert dm.source == "files" and dm.train_co3d is False
        assert gin.query_parameter("PeRFCeptionCo3DTrainDataset.bkgd_aug") == 0.5
        assert gin.query_parameter("PeRFCeptionCo3DTrainDataset.bkgd_on_device") is True
    finally:
        gin.clear_config()


def test_header_section_and_entry_point_checks():
    from nerf_downstream_amd import _lib

    P = _lib.constants("MINK_PASTE_")
    assert P["PARAMS"] == 8 and sorted(P[k] for k in ("FG_OFFSET", "MASK_OFFSET", "FG_W", "FG_H", "MASK_W", "MASK_H", "RW", "RH")) == list(range(8))
    assert _lib.CONSTANTS["MINK_ABI_VERSION"] == 4 and _lib.constants("MINK_IMG_")["PARAMS"] == 165
    assert len(_lib.SIGNATURES["mink_img_paste"][1]) == 13
    with open(_lib.HEADER) as f:
        assert "(csrc/paste.hip)" in f.read()
    L = _lib.lib()
    A, Bp, C = 0x10000, 0x20000, 0x30000  # never dereferenced: every check comes before the launch
    assert L.mink_img_paste(None, None, None, 1000, 4, None, 0, None, 0, None, 0, 0, None) == 0  # no paste, no launch
    assert L.mink_img_paste(None, None, None, 1000, 4, None, 10, None, 10, None, 5, 5, None) == -1
    assert b"NULL" in L.mink_last_error()
    assert L.mink_img_paste(A, A, A, 1000, 4, Bp, 10, C, 10, A, P["MAX_SIDE"] + 1, 5, None) == -1
    assert b"rectangle" in L.mink_last_error()
    assert L.mink_img_paste(A, A, A, 1000, 4, A + 2999, 10, C, 10, A, 5, 5, None) == -1
    assert b"overlap" in L.mink_last_error()
    assert L.mink_img_paste(A, A, A, 2, 4, Bp, 10, C, 10, A, 5, 5, None) == -1
    assert b"pixels" in L.mink_last_error()


def test_host_check_refuses_bad_rows():
    from nerf_downstream_amd.minkowski.utils import image_paste_check

    P = R.layout()
    sizes = np.array([[40, 30], [33, 47]], np.int32)
    good = np.zeros((2, P["PARAMS"]), np.int64)
    good[1, [P["FG_OFFSET"], P["MASK_OFFSET"], P["FG_W"], P["FG_H"], P["MASK_W"], P["MASK_H"], P["RW"], P["RH"]]] = [6, 2, 10, 8, 5, 4, 50, 12]
    assert image_paste_check(good, sizes, 6 + 240, 2 + 20) == (33, 12)
    assert image_paste_check(np.zeros_like(good), sizes, 0, 0) == (0, 0)
    for col, v in (("FG_OFFSET", 7), ("FG_OFFSET", -1), ("MASK_OFFSET", 3), ("MASK_OFFSET", -2), ("FG_W", 0), ("FG_H", 9), ("MASK_W", 6),
                   ("MASK_H", -4), ("RH", 0), ("RW", -3), ("RW", P["MAX_SIDE"] + 1)):
        bad = good.copy()
        bad[1, P[col]] = v
        with pytest.raises(ValueError, match="paste table, sample 1"):
            image_paste_check(bad, sizes, 6 + 240, 2 + 20)
    with pytest.raises(ValueError, match="paste table"):
        image_paste_check(good[:1], sizes, 246, 22)
    with pytest.raises(ValueError, match="paste table"):
        image_paste_check(good.astype(np.int32), sizes, 246, 22)
