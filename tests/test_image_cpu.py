"""CPU: the 2-D recipe's arithmetic and host layer.  tests/image_restate.py (numpy) equals what Pillow computed
(tests/golden/augmix_pillow_v1.npz, recorded by scripts/make_augmix_golden.py) bit for bit -- the hue plane included: the exact form
was found (`2.0 + rc - bc` is a double expression in Pillow's C, `bc - gc` a float one), so the fixture test is exact there too.
With Pillow installed the same holds live on random programs.  Then the draws, `collate_images`, the four datasets on PNG frames,
the gin config, and the argument checks of the new entry points, which need no GPU."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_restate as R  # noqa: E402

from nerf_downstream_amd import gin_lite as gin  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "augmix_pillow_v1.npz")


@pytest.fixture(scope="module")
def golden():
    assert os.path.getsize(GOLDEN) < 250_000
    return np.load(GOLDEN)


def _images(golden):
    for n in range(len(golden["sizes"])):
        yield n, golden[f"i{n}_image"], (lambda k, n=n: golden[f"i{n}_{k}"])


def test_fixture_images(golden):
    assert [tuple(s) for s in golden["sizes"]] == [(1, 1), (1, 7), (37, 53), (61, 83)]
    for n, img, _ in _images(golden):
        W, H = golden["sizes"][n]
        assert img.shape == (H, W, 3) and img.dtype == np.uint8
    # the narrow band: autocontrast stretches; 61x83: equalize's raw table runs past 255 and is clamped
    img = golden["i3_image"]
    band = img[8:, :, 1]  # (rows 0..7 hold the black / white / grey / saturated patches)
    assert int(band.max()) - int(band.min()) < 64
    clamped = False
    for h in R.histogram(img):
        nz = np.nonzero(h)[0]
        step = (int(h.sum()) - int(h[nz[-1]])) // 255
        n, top = step // 2, 0
        for i in range(256):
            top = max(top, n // step)
            n += int(h[i])
        clamped |= top > 255
    assert clamped


def test_point_ops_equal_pillow(golden):
    for n, img, g in _images(golden):
        assert np.array_equal(R.autocontrast(img), g("autocontrast")), n
        assert np.array_equal(R.equalize(img), g("equalize")), n
        for bits in (3, 4):
            assert np.array_equal(R.posterize(img, bits), g(f"posterize_{bits}")), (n, bits)
        for t in (180, 253):
            assert np.array_equal(R.solarize(img, t), g(f"solarize_{t}")), (n, t)


def test_geometric_ops_equal_pillow(golden):
    names, params = [str(v) for v in golden["geometric_names"]], list(golden["geometric_params"])
    assert sorted(names) == ["rotate", "shear_x", "shear_y", "translate_x", "translate_y"]
    for n, img, g in _images(golden):
        for name, p in zip(names, params):
            for sign, tag in ((1, "p"), (-1, "m")):
                assert np.array_equal(R.apply_op(img, name, sign * p), g(f"{name}_{tag}")), (n, name, tag)
        # rotate by 0 degrees and translate by 0 pixels are the identity, bit for bit
        assert np.array_equal(R.apply_op(img, "rotate", 0), img) and np.array_equal(R.apply_op(img, "translate_x", 0), img)


def test_crop_resize_equals_pillow(golden):
    S = int(golden["S"])
    for n, img, g in _images(golden):
        cases = g("crop_cases")
        assert len(cases) == 4
        for c, row in enumerate(cases):
            got = R.crop_resize(img, tuple(row[:4]), tuple(row[4:6]), tuple(row[6:8]), S)
            assert np.array_equal(got, g(f"crop_{c}")), (n, c)
        W, H = golden["sizes"][n]
        assert R.center_crop_geometry(int(W), int(H), S) == (tuple(cases[3][:4]), tuple(cases[3][4:6]), tuple(cases[3][6:8]))


def test_enhancers_and_hsv_equal_pillow(golden):
    for n, img, g in _images(golden):
        for f in (0.63, 1.37):
            assert np.array_equal(R.brightness(img, f), g(f"brightness_{f}")), (n, f)
            assert np.array_equal(R.saturation(img, f), g(f"saturation_{f}")), (n, f)
        hsv = R.rgb_to_hsv(img)
        assert np.array_equal(hsv[..., 1:], g("hsv")[..., 1:]), n
        diff = np.abs(hsv[..., 0].astype(int) - g("hsv")[..., 0].astype(int))
        assert diff.max(initial=0) <= 1 and (diff != 0).mean() <= 0.005  # the issue's bound ...
        assert np.array_equal(hsv[..., 0], g("hsv")[..., 0]), n  # ... and the exact form that was found
        for shift in (0, 37, -101):
            moved = g("hsv").copy()
            moved[..., 0] = (moved[..., 0].astype(int) + shift) % 256
            assert np.array_equal(R.hsv_to_rgb(moved), g(f"hsv_to_rgb_{shift}")), (n, shift)
    assert R.hue_shift(-0.4) == (256 - 102) and R.hue_shift(0.4) == 102 and R.hue_shift(0.0) == 0


# ------------------------------------------------------------------------------------------------------------- live, with Pillow
def _pil_branch(Image, ImageEnhance, ImageOps, img, br, S, chain):
    I = R.layout()
    im = Image.fromarray(img)
    BIL = getattr(Image, "Resampling", Image).BILINEAR
    AFF = getattr(Image, "Transform", Image).AFFINE
    if chain:
        for r in range(int(br[I["B_DEPTH"]])):
            op = br[I["B_OPS"] + r * I["OP_STRIDE"]: I["B_OPS"] + (r + 1) * I["OP_STRIDE"]]
            name = R.OPS[int(op[0]) - 1]
            if name == "autocontrast":
                im = ImageOps.autocontrast(im)
            elif name == "equalize":
                im = ImageOps.equalize(im)
            elif name == "posterize":
                im = ImageOps.posterize(im, int(op[1]))
            elif name == "solarize":
                im = ImageOps.solarize(im, int(op[1]))
            else:
                im = im.transform(im.size, AFF, tuple(op[1:7]), resample=BIL)
    x0, y0, w, h = (int(v) for v in br[I["B_BOX"]:I["B_BOX"] + 4])
    ow, oh = (int(v) for v in br[I["B_TARGET"]:I["B_TARGET"] + 2])
    wx, wy = (int(v) for v in br[I["B_WINDOW"]:I["B_WINDOW"] + 2])
    im = im.crop((x0, y0, x0 + w, y0 + h)).resize((ow, oh), BIL).crop((wx, wy, wx + S, wy + S))
    for slot in range(3):
        kind = int(br[I["B_ORDER"] + slot])
        f = br[I["B_FACTORS"] + kind - 1] if kind else None
        if kind == I["JIT_BRIGHTNESS"]:
            im = ImageEnhance.Brightness(im).enhance(f)
        elif kind == I["JIT_SATURATION"]:
            im = ImageEnhance.Color(im).enhance(f)
        elif kind == I["JIT_HUE"]:
            h_, s_, v_ = im.convert("HSV").split()
            nh = (np.array(h_, dtype=np.int32) + int(f * 255)) % 256
            im = Image.merge("HSV", (Image.fromarray(nh.astype(np.uint8), "L"), s_, v_)).convert("RGB")
    out = np.asarray(im)
    return out[:, ::-1] if br[I["B_FLIP"]] else out


def random_program(rng, sizes_wh, S, eval_form=False):
    """A program row with chain lengths 1..3, ops among the nine at levels, signs and integer parameters of the reference's ranges
    (rotate by 0 degrees and translate by 0 pixels among them), boxes inside the image, all jitter orders, sum(ws) = 1 in float32."""
    from nerf_downstream_amd.co3d_2d.src.data import augmix as A
    from nerf_downstream_amd.co3d_2d.src.data.transforms import compile_program

    W, H = sizes_wh
    I = R.layout()

    def branch():
        if eval_form:
            box, target, window = R.center_crop_geometry(W, H, S)
            return {"size": (W, H), "S": S, "box": box, "target": target, "window": window}
        w, h = int(rng.integers(1, W + 1)), int(rng.integers(1, H + 1))
        order = [int(v) for v in rng.permutation([I["JIT_BRIGHTNESS"], I["JIT_SATURATION"], I["JIT_HUE"]])][:int(rng.integers(0, 4))]
        return {"size": (W, H), "S": S, "box": (int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h),
                "target": (S, S), "window": (0, 0), "order": order,
                "factors": [rng.choice([0.6, 1.4, rng.uniform(0.6, 1.4)]), rng.choice([0.6, 1.4, rng.uniform(0.6, 1.4)]),
                            rng.choice([-0.4, 0.4, rng.uniform(-0.4, 0.4)])],
                "flip": bool(rng.integers(0, 2)), "rgb": rng.normal(0, 0.02, 3).astype(np.float32)}

    if eval_form:
        return compile_program(branch())
    width = 3
    ws = np.float32(rng.dirichlet([1.0] * width))
    chains = []
    for i in range(width):
        ops = []
        for _ in range(i + 1 if rng.integers(0, 2) else int(rng.integers(1, 4))):
            kind = int(rng.integers(1, 10))
            level, sign = rng.uniform(0.1, 3), (1 if rng.random() > 0.5 else -1)
            name = R.OPS[kind - 1]
            if name in ("autocontrast", "equalize"):
                ops.append((kind,))
            elif name == "posterize":
                ops.append((kind, 4 - int(level * 4 / 10)))
            elif name == "solarize":
                ops.append((kind, 256 - int(level * 256 / 10)))
            elif name == "rotate":
                ops.append((kind, *A.rotate_matrix(sign * int(rng.choice([0, level * 30 / 10])), (W, H))))
            elif name.startswith("shear"):
                ops.append((kind, *R.op_matrix(name, sign * level * 0.3 / 10, W, H)))
            else:
                ops.append((kind, *R.op_matrix(name, sign * int(rng.choice([0, level * (W if name[-1] == "x" else H) / 3 / 10])), W, H)))
        b = branch()
        b["ops"] = ops
        chains.append(b)
    return compile_program({"width": width, "ws": ws, "m": np.float32(rng.beta(1.0, 1.0)), "branches": [branch()] + chains})


def test_random_programs_equal_pillow_live():
    Image = pytest.importorskip("PIL.Image")
    from PIL import ImageEnhance, ImageOps

    rng = np.random.default_rng(7)
    I = R.layout()
    for t in range(20):
        W, H = (int(v) for v in rng.integers(1, 90, 2))
        S = int(rng.choice([7, 16, 33]))
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        img[..., 1] = 100 + img[..., 1] // 8
        row = random_program(rng, (W, H), S)
        assert abs(float(np.float32(row[I["WS"]:I["WS"] + 3]).sum()) - 1.0) < 3e-7
        _, stages, _ = R.run_program(img, row, S)
        for k in range(int(row[I["WIDTH"]]) + 1):
            br = row[I["BRANCH"] + k * I["BRANCH_STRIDE"]: I["BRANCH"] + (k + 1) * I["BRANCH_STRIDE"]]
            want = _pil_branch(Image, ImageEnhance, ImageOps, img, br, S, k > 0)
            assert np.array_equal(stages[k], want), (t, k)


def test_rotate_matrix_is_what_pillow_rotates_by():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(3)
    img = rng.integers(0, 256, (31, 45, 3), dtype=np.uint8)
    for d in (-9, -1, 0, 4, 9):
        want = np.asarray(Image.fromarray(img).rotate(d, resample=getattr(Image, "Resampling", Image).BILINEAR))
        assert np.array_equal(R.affine(img, R.rotate_matrix(d, 45, 31)), want), d


# ------------------------------------------------------------------------------------------------------------------ the host layer
def test_draws_are_in_range():
    from nerf_downstream_amd.co3d_2d.src.data import transforms as T

    np.random.seed(11)
    I = R.layout()
    recipe = T.Compose(T.TRAIN_ORDER)
    kinds = set()
    for W, H in ((800, 600), (37, 53), (1, 400)):
        for _ in range(40):
            s = T.AugMix().draw((W, H), recipe.draw)
            row = T.compile_program(s)
            assert s["ws"].dtype == np.float32 and abs(float(s["ws"].sum()) - 1) < 3e-7 and 0 <= float(s["m"]) <= 1
            assert row[I["WIDTH"]] == 3 and len(s["branches"]) == 4
            boxes = set()
            for k, b in enumerate(s["branches"]):
                x0, y0, w, h = b["box"]
                assert 0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H
                assert sorted(b["order"]) == [1, 2, 3] and 0.6 <= b["factors"][0] <= 1.4 and -0.4 <= b["factors"][2] <= 0.4
                boxes.add(b["box"])
                for op in b.get("ops", []):
                    kinds.add(op[0])
                    name = R.OPS[op[0] - 1]
                    if name == "posterize":
                        assert op[1] in (3, 4)
                    elif name == "solarize":
                        assert 256 - 76 <= op[1] <= 256
                    elif name.startswith("translate"):
                        assert op[3 if name[-1] == "x" else 6] == int(op[3 if name[-1] == "x" else 6])
                if k:
                    assert 1 <= len(b["ops"]) <= 3
            if (W, H) == (800, 600):
                assert len(boxes) > 1  # every branch has its own crop
            if (W, H) == (1, 400):
                assert all(b["box"] == (0, 199, 1, 1) or b["box"][2] == 1 for b in s["branches"])
    assert kinds == set(range(1, 10))
    # ten failed tries, then the central crop of the nearest legal aspect
    rrc = T.RandomResizedCrop()
    rrc.scale = (4.0, 4.0)
    assert rrc.get_params(1, 400) == (0, 199, 1, 1) and rrc.get_params(400, 1) == (199, 0, 1, 1) and rrc.get_params(40, 40) == (0, 0, 40, 40)
    with pytest.raises(RuntimeError, match="runs on the GPU"):
        T.ColorJitter()(None)
    with pytest.raises(NotImplementedError):
        T.Compose(["ColorJitter", "RandomResizedCrop", "ToTensor", "Normalize"])


def _write_frames(tmp_path, sub):
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(5)
    root, lists = tmp_path / "data", tmp_path / "filelist"
    lists.mkdir()
    rows = []
    for cls, scene, (W, H) in (("apple", "s1", (40, 30)), ("tv", "s2", (33, 47)), ("vase", "s3", (64, 64))):
        d = root / cls / scene / sub
        d.mkdir(parents=True)
        for f in range(3):
            Image.fromarray(rng.integers(0, 256, (H, W, 3), dtype=np.uint8)).save(d / f"frame{f:03d}.png")
        rows.append(f"{cls} {scene} 3")
    for phase in ("train", "val", "test"):
        (lists / f"{phase}.txt").write_text("\n".join(rows) + "\n")
    return str(root), str(lists)


@pytest.mark.parametrize("perfception", [False, True])
def test_datasets_on_png_frames(tmp_path, perfception):
    from nerf_downstream_amd.co3d_2d.src.data import loader as Ld

    root, lists = _write_frames(tmp_path, "fgbg" if perfception else "images")
    I = R.layout()
    np.random.seed(2)
    if perfception:
        train = Ld.PeRFCeptionCo3DTrainDataset(data_root=root, filelist_root=lists)
        train.num_frames = [3] * len(train)  # (the reference draws among 50 renders per scene; three were written)
        ev = Ld.PeRFCeptionCo3DEvalDataset("val", data_root=root, filelist_root=lists)
        with pytest.raises(NotImplementedError, match="BackgroundAug"):
            Ld.PeRFCeptionCo3DTrainDataset(bkgd_aug=0.5, data_root=root, filelist_root=lists)
    else:
        train = Ld.Co3DTrainDataset(data_root=root, filelist_root=lists)
        ev = Ld.Co3DEvalDataset("val", data_root=root, filelist_root=lists)
    assert len(train) == 3 and len(ev) == 9 and Ld.CLASSES[50] == "wineglass" and len(Ld.CLASSES) == 51
    s = train[1]
    assert s["image"].dtype == torch.uint8 and tuple(s["image"].shape) == (47, 33, 3) and int(s["labels"]) == Ld.CLASSES_IDX["tv"]
    assert s["program"].shape == (I["PARAMS"],) and s["program"][I["WIDTH"]] == 3 and s["size"] == 224
    e = ev[8]
    assert tuple(e["image"].shape) == (64, 64, 3) and e["program"][I["WIDTH"]] == 0 and int(e["labels"]) == Ld.CLASSES_IDX["vase"]
    batch = Ld.collate_images([train[0], train[1], train[2], ev[0]])
    assert batch["offsets"].tolist() == [0, 3600, 3600 + 4653, 3600 + 4653 + 12288, 3600 + 4653 + 12288 + 3600]
    assert batch["sizes"].tolist() == [[40, 30], [33, 47], [64, 64], [40, 30]] and batch["packed"].numel() == batch["offsets"][-1]
    assert batch["programs"].shape == (4, I["PARAMS"]) and batch["labels"].tolist() == [0, Ld.CLASSES_IDX["tv"], Ld.CLASSES_IDX["vase"], 0]
    assert torch.equal(batch["packed"][-3600:].view(30, 40, 3), ev[0]["image"])
    from nerf_downstream_amd.minkowski.utils import image_batch_check

    assert image_batch_check(batch["offsets"].numpy(), batch["sizes"].numpy(), batch["programs"].numpy(), batch["packed"].numel()) == (4, 3)
    with pytest.raises(ValueError, match="running sum"):
        image_batch_check(batch["offsets"].numpy() + 1, batch["sizes"].numpy(), batch["programs"].numpy(), batch["packed"].numel())


def test_synthetic_source_is_unchanged():
    from nerf_downstream_amd.co3d_2d.src.data.loader import DataModule, SyntheticRenders

    gin.clear_config()
    dm = DataModule(num_workers=0, batch_size=2)
    assert dm.source == "synthetic"
    assert isinstance(dm.train_dataloader().dataset, SyntheticRenders)
    s = dm.val_dataloader().dataset[5]
    # values of the parent commit for (phase "val", index 5): a fixed generator, so they are constants of the data set
    assert tuple(s["images"].shape) == (3, 224, 224) and int(s["labels"]) == 5
    again = SyntheticRenders("val")[5]["images"]
    assert torch.equal(s["images"], again)
    assert abs(float(s["images"].double().mean()) - _SYNTHETIC_MEAN) < 1e-6 and abs(float(s["images"][1, 100, 50]) - _SYNTHETIC_PIXEL) < 1e-6
    with pytest.raises(ValueError):
        DataModule(source="disk")


_SYNTHETIC_MEAN, _SYNTHETIC_PIXEL = -1.0235175155501528, 0.6509144902229309  # recorded on the parent commit


def test_frames_config_parses_after_a_model_config():
    from nerf_downstream_amd.co3d_2d.src.data import transforms as T
    from nerf_downstream_amd.co3d_2d.src.data.loader import DataModule

    cfg = os.path.join(ROOT, "nerf_downstream_amd", "co3d_2d", "configs")
    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings([os.path.join(cfg, "resnet18.gin"), os.path.join(cfg, "co3d_frames.gin")],
                                            ["RandomResizedCrop.image_size = (16, 16)", "AugMix.width = 2"])
        dm = DataModule()
        assert dm.source == "files" and dm.train_co3d is True and dm.batch_size == 32
        assert T.RandomResizedCrop().image_size == 16 and T.CenterCrop().image_size == 224 and T.AugMix().width == 2
        assert T.ColorJitter().hue == 0.4 and T.PCALoss().alphastd == 0.1
    finally:
        gin.clear_config()


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced: every check comes before the first launch
    need = L.mink_img_workspace_bytes(1000, 4, 3, 224)
    assert need >= 2 * 3 * 3000 + 4 * 3 * 768 * 5
    assert L.mink_img_workspace_bytes(1000, 4, 4, 224) == -1
    assert L.mink_img_chain_buffer_offset(1000, 4, 3, 1, 1) == L.mink_img_chain_buffer_offset(1000, 4, 3, 1, 3)
    assert L.mink_img_chain_buffer_offset(1000, 4, 3, 1, 1) < L.mink_img_chain_buffer_offset(1000, 4, 3, 1, 2) < need
    assert L.mink_img_chain_buffer_offset(1000, 4, 3, 0, 1) == -1 and L.mink_img_chain_buffer_offset(1000, 4, 3, 4, 1) == -1
    assert L.mink_img_chain_round(None, None, None, None, 1000, 4, 3, 0, P, need, None) == -1
    assert b"NULL" in L.mink_last_error()
    assert L.mink_img_chain_round(P, P, P, P, 1000, 4, 3, 0, None, need, None) == -1
    assert b"NULL workspace" in L.mink_last_error()
    assert L.mink_img_chain_round(P, P, P, P, 1000, 4, 3, 0, P, need - 1, None) == -1
    assert b"workspace" in L.mink_last_error() and str(need).encode() in L.mink_last_error()
    assert L.mink_img_chain_round(P, P, P, P, 1000, 4, 3, 3, P, need, None) == -1
    assert b"round" in L.mink_last_error()
    assert L.mink_img_finish(None, None, None, None, 1000, 4, 3, 16, P, need, P, None, None) == -1
    assert b"NULL" in L.mink_last_error()
    assert L.mink_img_finish(P, P, P, P, 1000, 4, 3, 16, P, need, None, None, None) == -1
    assert b"NULL output" in L.mink_last_error()
    assert L.mink_img_finish(P, P, P, P, 1000, 4, 3, 16, P, need - 1, P, None, None) == -1
    assert b"workspace" in L.mink_last_error() and str(need).encode() in L.mink_last_error()
    assert L.mink_img_finish(P, P, P, P, 1000, 4, 3, 0, P, need, P, None, None) == -1
    assert L.mink_img_finish(P, P, P, P, 1000, 4, 4, 16, P, need, P, None, None) == -1
    assert b"width" in L.mink_last_error()
    assert _lib.CONSTANTS["MINK_ABI_VERSION"] == 4 and _lib.constants("MINK_IMG_")["PARAMS"] == 5 + 4 * 40
