"""-m gpu: the LiDAR input on the device (`mink_lidar_decode_scans`, `mink_lidar_finish_rows`, minkowski/utils.py
prepare_lidar_batch, data/semantic_kitti.py, data/stanford.py) against the numpy restatement (tests/lidar_restate.py): the
decode bit for bit across empty scans, single rows and a wave boundary; down-sampling plus finish without a recipe (table
before the vote); the full default recipe with every stage forced on; coordinates without a voxel; S3DIS through the
point-cloud path; and two training steps plus a validation pass of both configs through
`python -m nerf_downstream_amd.co3d_3d.train`."""
import csv
import glob
import os
import random
import subprocess
import sys

import numpy as np
import pytest
import torch

from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as ST
from lidar_restate import decode, label_table, prepare_scene, synthetic_scan, write_kitti_tree, write_s3dis_tree
from pc_restate import color_program, downsample, synthetic_scene

pytestmark = pytest.mark.gpu

ROOT = os.path.join(os.path.dirname(__file__), "..")
CFG = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")
SEED = 0x0DDC0FFEE1234567
IGNORE = -100
Q, VOXEL = 0.025, 0.05


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dev():
    return torch.device("cuda")


def _batch(scans, words, q=Q, voxel=VOXEL):
    """The collated batch of data/utils.py, on the device; words: list of uint32 arrays, or None for a batch without labels."""
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    table, _ = label_table(IGNORE)
    b = {"scan": torch.from_numpy(np.concatenate(scans).astype(np.float32).reshape(-1, 4)).to(_dev()),
         "scene_offsets": torch.from_numpy(offs).to(_dev()), "label_lut": torch.from_numpy(table).to(_dev()),
         "lidar_params": np.array([[q, voxel, IGNORE]] * len(scans), np.float64), "feature_names": ("xyzi",)}
    if words is not None:
        b["raw_labels"] = torch.from_numpy(np.concatenate(words).astype(np.uint32).view(np.int32)).to(_dev())
    return b, offs, table


# ------------------------------------------------------------------ decode
def _decode_scans():
    rng = np.random.default_rng(0)
    return [synthetic_scan(rng, n) for n in (0, 1, 63, 64, 65, 257, 5003)]


@pytest.mark.parametrize("labels", ["named", "outside", "none"])
def test_decode_matches_restatement_bit_for_bit(labels):
    """7 scans of 0, 1, 63, 64, 65, 257 and 5003 points in one batch.  `named`: the ids of the data set with instance ids
    above them, ids 0 and 259 among them; `outside`: ids 260 and 0xFFFF too -- those rows get the ignore label, the status
    word counts them and the host check raises; `none`: a NULL label pointer."""
    from nerf_downstream_amd.minkowski.utils import LidarLabelError, lidar_decode_batch, lidar_status_check

    pairs = _decode_scans()
    scans, words = [p[0] for p in pairs], [p[1].copy() for p in pairs]
    words[6][:4] = [0, 259, 0xFFFF0000, 0xABCD0000 | 259]
    words[1][0] = 0x00010000 | 252
    if labels == "outside":
        words[6][10:14] = [260, 0xFFFF, 0x12340000 | 260, 0x7FFF]
        words[3][63] = 0xFFFFFFFF
    b, offs, table = _batch(scans, None if labels == "none" else words)
    c, f, lab, status = lidar_decode_batch(b["scan"], b.get("raw_labels"), b["scene_offsets"], b["label_lut"], IGNORE)
    torch.cuda.synchronize()
    rc, rf, rl, bad = decode(scans, [None] * 7 if labels == "none" else words, table, IGNORE)
    assert c.shape == (offs[-1], 4) and f.shape == (offs[-1], 4) and lab.dtype == torch.int32
    assert np.array_equal(_bits(c.cpu().numpy()), _bits(rc)) and np.array_equal(_bits(f.cpu().numpy()), _bits(rf))
    assert np.array_equal(lab.cpu().numpy(), rl)
    assert int(status.item()) == bad == (5 if labels == "outside" else 0)
    if labels == "outside":
        got = lab.cpu().numpy()
        assert (got[offs[6] + 10:offs[6] + 14] == IGNORE).all() and got[offs[3] + 63] == IGNORE
        with pytest.raises(LidarLabelError):
            lidar_status_check(status)
    else:
        lidar_status_check(status)
        if labels == "none":
            assert (lab == IGNORE).all()  # (id 0 = unlabeled)
        else:
            got = lab.cpu().numpy()
            assert got[offs[6]:offs[6] + 4].tolist() == [IGNORE, 4, IGNORE, 4] and got[offs[1]] == 0


# ------------------------------------------------------------------ down-sampling + finish, no recipe
def _vote_scans():
    """Three scans over +-80 m.  Scan 0 ends in six planted points: two in one voxel with ids 10 and 252 (car and
    moving-car), two in another with ids 10 and 11, and two exactly on multiples of the voxel size; every scan also gets
    points snapped to multiples of the voxel size and of the down-sampling size."""
    rng = np.random.default_rng(21)
    out = []
    for n in (4000, 1, 2500):
        scan, words = synthetic_scan(rng, n)
        k, a = n // 8, n // 5  # (past the first tenth: those keep their second returns beside them)
        scan[a:a + k, :3] = (np.round(scan[a:a + k, :3] / VOXEL) * VOXEL).astype(np.float32)
        scan[a + k:a + 2 * k, :3] = (np.round(scan[a + k:a + 2 * k, :3] / Q).astype(np.float32) * np.float32(Q))
        out.append((scan, words))
    scan, words = out[0]
    planted = np.array([[-90.006, -90.004, 1.005, 0.5], [-90.004, -90.003, 1.01, 0.6], [-95.006, 95.004, 1.005, 0.7],
                        [-95.004, 95.003, 1.01, 0.8], [-91.0, -91.5, 0.05, 0.9], [np.float32(-0.05) * 1801, 91.0, -0.1, 1.0]], np.float32)
    pw = np.array([10 | (3 << 16), 252 | (4 << 16), 10, 11, 40, 48], np.uint32)
    out[0] = (np.concatenate([scan, planted]), np.concatenate([words, pw]))
    return out


def test_downsample_and_finish_without_a_recipe_bit_for_bit():
    from nerf_downstream_amd.minkowski.utils import prepare_lidar_batch

    pairs = _vote_scans()
    scans, words = [p[0] for p in pairs], [p[1] for p in pairs]
    assert (np.concatenate(scans)[:, :3] < 0).any()
    b, offs, table = _batch(scans, words)
    c, f, lab, src = [t.cpu().numpy() for t in prepare_lidar_batch(b)]
    assert lab.dtype == np.int64 and src.dtype == np.int32 and f.shape[1] == 4
    scene = c[:, 0].astype(np.int64)
    assert (np.diff(scene) >= 0).all()
    for s in range(len(scans)):
        rc, rf, rl, rows = prepare_scene(scans[s], words[s], table, Q, VOXEL, IGNORE)
        mine = scene == s
        assert int(mine.sum()) == len(rows), s
        assert np.array_equal(src[mine] - offs[s], rows), s  # representatives and their order
        assert np.array_equal(_bits(c[mine, 1:]), _bits(rc)) and np.array_equal(_bits(f[mine]), _bits(rf)), s
        assert np.array_equal(lab[mine], rl), s
    n0 = len(scans[0])
    by_row = {int(r): int(l) for r, l in zip(src[scene == 0], lab[scene == 0])}
    assert by_row[n0 - 6] == 0 and (n0 - 5) not in by_row  # car + moving-car share a voxel: class 0 (car), not ignore
    assert by_row[n0 - 4] == IGNORE and (n0 - 3) not in by_row  # car + bicycle: voted away
    assert by_row[n0 - 2] == 8 and by_row[n0 - 1] == 10
    # (the vote is exercised beyond the planted voxel: some voxel whose rows map to different classes)
    _, _, mapped, _ = decode([scans[0]], [words[0]], table, IGNORE)
    reps, _, voted = downsample(scans[0][:, :3], mapped, Q, 1.0, IGNORE)
    assert ((voted == IGNORE) & (mapped[reps] != IGNORE)).sum() > 1


# ------------------------------------------------------------------ the default recipe, every stage forced on
def _recipe_batch(n_scans=3, seed=5):
    from nerf_downstream_amd.co3d_3d.src.data.transforms import CoordinateDropout, RandomAffine, RandomHorizontalFlip, RandomTranslation

    rng = np.random.default_rng(seed)
    pairs = [synthetic_scan(rng, n) for n in (6000, 2000, 3001)[:n_scans]]
    scans, words = [p[0] for p in pairs], [p[1] for p in pairs]
    b, offs, table = _batch(scans, words)
    comp = ST.PointCompose([CoordinateDropout(0.2, application_ratio=1), RandomHorizontalFlip("z", application_ratio=1),
                            RandomAffine(application_ratio=1), RandomTranslation(application_ratio=1)])
    random.seed(seed), np.random.seed(seed)
    drawn = [comp.sample((s[:, :3].max(0) - s[:, :3].min(0)).astype(np.float64)) for s in scans]
    P = np.stack([d[0] for d in drawn])
    streams = np.array([d[2] for d in drawn], np.uint32)
    assert (P[:, ST.SEG["DROPOUT"]] == 0.2).all() and (P[:, ST.SEG["FLIP"]:ST.SEG["FLIP"] + 2] == 1).all()
    assert not np.allclose(P[:, ST.SEG["B"]:ST.SEG["B"] + 9], np.eye(3).reshape(-1)) and P[:, ST.SEG["b"]:ST.SEG["b"] + 3].all()
    b["aug_params"], b["aug_seed"] = torch.from_numpy(P), SEED
    b["aug_streams"] = torch.from_numpy(streams.view(np.int32).copy()).to(_dev())
    return b, scans, words, offs, table, P, streams


def test_full_default_recipe_matches_restatement():
    from nerf_downstream_amd.minkowski.utils import lidar_batch_status_check, lidar_finish_rows, prepare_lidar_batch

    b, scans, words, offs, table, P, streams = _recipe_batch()
    out1 = [t.cpu() for t in prepare_lidar_batch(b)]
    out2 = [t.cpu() for t in prepare_lidar_batch(b)]
    for x, y in zip(out1, out2):  # two runs, bitwise
        assert x.dtype == y.dtype and torch.equal(x.view(torch.int32) if x.is_floating_point() else x, y.view(torch.int32) if y.is_floating_point() else y)
    c, f, lab, src = [t.numpy() for t in out1]
    scene = c[:, 0].astype(np.int64)
    want_c, want_f, total_reps = [], [], 0
    for s in range(len(scans)):
        rc, rf, rl, rows = prepare_scene(scans[s], words[s], table, Q, VOXEL, IGNORE, P[s], streams[s], SEED)
        total_reps += len(downsample(scans[s][:, :3], np.zeros(len(scans[s])), Q, 1.0, IGNORE)[0])
        mine = scene == s
        assert int(mine.sum()) == len(rows), s  # survivors
        assert np.array_equal(src[mine] - offs[s], rows) and np.array_equal(lab[mine], rl), s  # their source rows and classes
        assert np.array_equal(_bits(c[mine, 1:]), _bits(rc)), s  # f32(r) / f32(0.05)
        assert np.array_equal(_bits(f[mine]), _bits(rf)), s  # f32(r) and the intensity of the source row
        want_c.append(np.concatenate([np.full((len(rc), 1), s, np.float32), rf[:, :3]], 1)), want_f.append(rf)
    k = len(c)
    assert 0.6 * total_reps < k < 0.95 * total_reps  # (the dropout removed about a fifth)
    # the deferred form: full-length buffers, the count through pinned memory
    fc, ff, fl, fs, (host, ev) = prepare_lidar_batch(b, count_async=True)
    ev.synchronize()
    lidar_batch_status_check(host)
    assert host.numel() == 5 and int(host[0]) == k and fc.shape[0] == offs[-1] and torch.equal(fc[:k].cpu(), out1[0])
    assert torch.equal(ff[:k].cpu(), out1[1]) and torch.equal(fl[:k].cpu(), out1[2]) and torch.equal(fs[:k].cpu(), out1[3])
    # rows past the survivor count are untouched: the finish step on sentinel-filled buffers holding the restated rows
    n = int(offs[-1])
    hc, hf = np.full((n, 4), 0x7FC0BEEF, np.uint32).view(np.float32), np.full((n, 4), 0x7FC0BEEF, np.uint32).view(np.float32)
    hc[:k], hf[:k, 3] = np.concatenate(want_c), np.concatenate(want_f)[:, 3]
    dc, df = torch.from_numpy(hc.copy()).to(_dev()), torch.from_numpy(hf.copy()).to(_dev())
    lidar_finish_rows(dc, df, torch.tensor([k], dtype=torch.int32, device=_dev()), VOXEL)
    gc, gf = dc.cpu().numpy(), df.cpu().numpy()
    assert np.array_equal(_bits(gc[k:]), _bits(hc[k:])) and np.array_equal(_bits(gf[k:]), _bits(hf[k:]))
    assert np.array_equal(_bits(gc[:k]), _bits(c)) and np.array_equal(_bits(gf[:k]), _bits(f))


# ------------------------------------------------------------------ the deferred form, as the trainer drives it
def _loader_batch(tmp_path, bad_word=None):
    """A collated training batch of SemanticKITTIDataset, moved to the device the way train.py moves it."""
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SemanticKITTIDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink
    from nerf_downstream_amd.co3d_3d.train import _to_device

    rng = np.random.default_rng(17)
    scans = [synthetic_scan(rng, n) for n in (1500, 900)]
    if bad_word is not None:
        scans[1][1][33] = bad_word
    write_kitti_tree(str(tmp_path), scans, sequences=("00",))
    ds = SemanticKITTIDataset("train", data_root=str(tmp_path))
    random.seed(2), np.random.seed(2)
    batch = _to_device(collate_mink([ds[0], ds[1]]), _dev())
    torch.cuda.synchronize()
    return batch


def test_deferred_preparation_makes_no_synchronising_call(tmp_path):
    """`prepare_lidar_batch(count_async=True)` on a batch moved as the trainer moves it: torch's sync debug mode turns every
    synchronising call (a `.cpu()`, an `.item()`, a blocking copy) into an error, and none may happen.  The host values
    stay on the host through the move; handed over as a device tensor they are refused, not read back."""
    from nerf_downstream_amd.minkowski.utils import lidar_batch_status_check, prepare_lidar_batch

    batch = _loader_batch(tmp_path)
    assert isinstance(batch["lidar_params"], np.ndarray) and not batch["aug_params"].is_cuda and batch["scan"].is_cuda
    want = [t.cpu() for t in prepare_lidar_batch(batch)]
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        with pytest.raises(RuntimeError):  # (the mode has teeth here: a read-back is an error)
            batch["scene_offsets"].cpu()
        c, f, lab, src, (host, ev) = prepare_lidar_batch(batch, count_async=True)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    ev.synchronize()
    lidar_batch_status_check(host)
    k = int(host[0])
    assert k == len(want[0]) and torch.equal(c[:k].cpu(), want[0]) and torch.equal(f[:k].cpu(), want[1])
    assert torch.equal(lab[:k].cpu(), want[2]) and torch.equal(src[:k].cpu(), want[3])
    with pytest.raises(TypeError, match="host values"):
        prepare_lidar_batch(dict(batch, lidar_params=torch.from_numpy(batch["lidar_params"]).cuda()), count_async=True)


def test_label_word_outside_the_table_raises_through_every_form(tmp_path):
    """One word with semantic id 260 in the batch: the fifth status word carries it through the synchronous form, the
    deferred form and `process_input(defer=True)` + `finish_input`; the same batch without it goes through all three."""
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.minkowski.utils import LidarLabelError, lidar_batch_status_check, prepare_lidar_batch

    model = get_model("Res16UNet14A", 4, 19).cuda()
    for bad in (None, 0x00050000 | 260):
        batch = _loader_batch(tmp_path / ("bad" if bad else "good"), bad)
        out = prepare_lidar_batch(batch, count_async=True)
        out[4][1].synchronize()
        assert out[4][0].tolist()[1:] == [0, 0, 0, 1 if bad else 0]
        if bad is None:
            k = len(prepare_lidar_batch(batch)[0])
            lidar_batch_status_check(out[4][0])
            field = model.finish_input(model.process_input(batch, defer=True))
            assert int(out[4][0][0]) == k == len(field.row_labels) == len(field.point_rows) and field.row_labels.dtype == torch.int64
        else:
            with pytest.raises(LidarLabelError):
                prepare_lidar_batch(batch)
            with pytest.raises(LidarLabelError):
                lidar_batch_status_check(out[4][0])
            pending = model.process_input(batch, defer=True)
            with pytest.raises(LidarLabelError):
                model.finish_input(pending)


# ------------------------------------------------------------------ coordinates without a voxel
@pytest.mark.parametrize("bad", [float("nan"), float("inf"), 1e20])
def test_coordinates_without_a_voxel_raise(bad):
    from nerf_downstream_amd.minkowski.utils import VoxelRangeError, prepare_lidar_batch

    b, scans, words, offs, table, P, streams = _recipe_batch(n_scans=2)
    prepare_lidar_batch(b)  # the same batch without it passes
    b["scan"][offs[1] + 17, 1] = bad
    with pytest.raises(VoxelRangeError):
        prepare_lidar_batch(b)


# ------------------------------------------------------------------ S3DIS through the point-cloud path
def _s3dis_scenes(rng, n_scenes, n):
    return [(xyz, rgb, (lab % 14).astype(np.int32)) for xyz, rgb, lab in (synthetic_scene(rng, n) for _ in range(n_scenes))]


def test_stanford_dataset_through_prepare_point_batch(tmp_path):
    from nerf_downstream_amd.co3d_3d.src.data.stanford import StanfordDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink
    from nerf_downstream_amd.minkowski.utils import prepare_point_batch

    scenes = _s3dis_scenes(np.random.default_rng(8), 2, 6000)
    write_s3dis_tree(str(tmp_path), scenes)
    ds = StanfordDataset("val", data_root=str(tmp_path))  # NormalizeColor only: every value is determined
    batch = collate_mink([ds[0], ds[1]])
    offs = batch["scene_offsets"].numpy()
    c, f, lab, src = [t.cpu().numpy() for t in prepare_point_batch({k: (v.cuda() if torch.is_tensor(v) else v) for k, v in batch.items()})]
    lut = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, IGNORE, 10, 11, 12])
    scene = c[:, 0].astype(np.int64)
    seen = set()
    for s, (xyz, rgb, raw) in enumerate(scenes):
        reps, rc, voted = downsample(xyz, raw, 0.015, 0.03, IGNORE)
        mine = scene == s
        assert np.array_equal(src[mine] - offs[s], reps) and np.array_equal(_bits(c[mine, 1:]), _bits(rc)), s
        want = np.where(voted == IGNORE, IGNORE, lut[np.clip(voted, 0, 13)])
        assert np.array_equal(lab[mine], want), s
        colours = color_program(rgb[reps], batch["color_params"][s].numpy(), reps, 0, 0)
        assert np.array_equal(_bits(f[mine]), _bits(colours)), s
        seen |= set(want.tolist())
    assert IGNORE in seen and 12 in seen and max(seen) == 12  # raw id 10 and the votes -> ignore; raw id 13 -> class 12
    train = StanfordDataset("train", data_root=str(tmp_path))  # the drawn recipe: the classes follow the surviving rows
    random.seed(1), np.random.seed(1)
    tb = collate_mink([train[0], train[1]])
    c, f, lab, src = [t.cpu().numpy() for t in prepare_point_batch({k: (v.cuda() if torch.is_tensor(v) and k != "aug_params" else v)
                                                                    for k, v in tb.items()})]
    for s, (xyz, rgb, raw) in enumerate(scenes):
        reps, _, voted = downsample(xyz, raw, 0.015, 0.03, IGNORE)
        vote_of = dict(zip(reps.tolist(), np.where(voted == IGNORE, IGNORE, lut[np.clip(voted, 0, 13)]).tolist()))
        mine = c[:, 0] == s
        assert mine.any() and lab[mine].tolist() == [vote_of[r] for r in (src[mine] - offs[s]).tolist()], s
    assert np.isfinite(f).all() and np.abs(f).max() <= 0.6


# ------------------------------------------------------------------ end to end
def _train(tmp_path, cfg, bindings):
    save = tmp_path / "run"
    cmd = [sys.executable, "-m", "nerf_downstream_amd.co3d_3d.train", "--ginc", f"{CFG}/{cfg}", "--ginc", f"{CFG}/res16unet.gin",
           "--save_path", str(save), "--run_name", "lidar", "--seed", "3"]
    for b in ["train.max_steps=2", "train.val_every_n_steps=2", "train.log_every_n_steps=1", "train.batch_size=2",
              "train.val_batch_size=1", "train.train_num_workers=0", "train.val_num_workers=0", "train.lr=0.01",
              "get_model.name='Res16UNet14A'"] + bindings:
        cmd += ["--ginb", b]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    logs = glob.glob(str(save / "**" / "*.csv"), recursive=True)
    assert logs, r.stderr[-2000:]
    rows = [row for f in logs for row in csv.DictReader(open(f))]
    losses = [float(row["train/loss"]) for row in rows if row.get("train/loss")]
    assert len(losses) == 2 and all(np.isfinite(losses)), rows
    vals = [row for row in rows if row.get("val/mIoU")]
    assert vals and all(np.isfinite(float(v["val/loss"])) for v in vals), rows


def test_train_two_steps_and_validate_with_semantic_kitti_config(tmp_path):
    rng = np.random.default_rng(13)
    scans = [synthetic_scan(rng, 3000 + 7 * i) for i in range(4)]
    write_kitti_tree(str(tmp_path), scans, sequences=("00",))
    write_kitti_tree(str(tmp_path), scans[:2], sequences=("08",))
    _train(tmp_path, "semantic_kitti.gin", [f"SemanticKITTIDataset.data_root='{tmp_path}'"])


def test_train_two_steps_and_validate_with_stanford_config(tmp_path):
    write_s3dis_tree(str(tmp_path), _s3dis_scenes(np.random.default_rng(14), 3, 8000))
    _train(tmp_path, "stanford_semseg.gin", [f"StanfordDataset.data_root='{tmp_path}'"])
