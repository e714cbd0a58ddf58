"""GPU: the 2-D trainer on frames from disk -- resnet18.gin + co3d_frames.gin, eight PNG frames of three sizes, batch 4, a handful of
steps and one evaluation: finite loss, logits of the right shape, and an evaluation input equal to the restatement's CenterCrop
tensor."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import image_restate as R  # noqa: E402

from nerf_downstream_amd import gin_lite as gin  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_training_on_png_frames(tmp_path):
    Image = pytest.importorskip("PIL.Image")
    from nerf_downstream_amd.co3d_2d import train as T
    from nerf_downstream_amd.co3d_2d.src.data import loader as Ld

    rng = np.random.default_rng(13)
    root, lists = tmp_path / "data", tmp_path / "filelist"
    lists.mkdir()
    lines, frames = [], {}
    sizes = [(96, 64), (50, 70), (64, 64)]
    for j, cls in enumerate(("apple", "bench", "cup", "donut", "kite", "mouse", "tv", "vase")):  # eight scenes of one frame each
        scene, (W, H), n = f"scene{j}", sizes[j % 3], 1
        d = root / cls / scene / "images"
        d.mkdir(parents=True)
        for f in range(n):
            arr = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
            Image.fromarray(arr).save(d / f"frame{f:03d}.png")
            frames[str(d / f"frame{f:03d}.png")] = arr
        lines.append(f"{cls} {scene} {n}")
    for phase in ("train", "val", "test"):
        (lists / f"{phase}.txt").write_text("\n".join(lines) + "\n")
    cfg = os.path.join(ROOT, "nerf_downstream_amd", "co3d_2d", "configs")
    S = 64
    seen = {}
    old = Ld.images_to_device

    def spy(batch, device):
        out = old(batch, device)
        if "programs" in batch and float(batch["programs"][0, R.layout()["WIDTH"]]) == 0 and "eval" not in seen:
            seen["eval"] = (batch, out["images"].detach().cpu().numpy())
        return out

    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings(
            [os.path.join(cfg, "resnet18.gin"), os.path.join(cfg, "co3d_frames.gin")],
            [f'Co3DTrainDataset.data_root = "{root}"', f'Co3DTrainDataset.filelist_root = "{lists}"',
             f'Co3DEvalDataset.data_root = "{root}"', f'Co3DEvalDataset.filelist_root = "{lists}"',
             f"RandomResizedCrop.image_size = ({S}, {S})", f"CenterCrop.image_size = {S}", "DataModule.batch_size = 4",
             "DataModule.chunks = 4", "DataModule.num_workers = 0", "run.max_steps = 3", "run.max_epochs = 50", "run.run_eval = False",
             "run.log_every_n_steps = 1", f'run.log_dir = "{tmp_path / "logs"}"', "run.precision = 32"])
        Ld.images_to_device = T.images_to_device = spy
        np.random.seed(0)
        res = T.run(ckpt_path=None, resume_training=False, seed=1)
        # the model on one prepared training batch: logits [4, 51]
        dm = Ld.DataModule()
        batch = old(next(iter(dm.train_dataloader())), torch.device("cuda", 0))
        assert tuple(batch["images"].shape) == (4, 3, S, S) and bool(torch.isfinite(batch["images"]).all())
        from nerf_downstream_amd.co3d_2d.src.modules.classification import LitModel

        with torch.no_grad():
            logits = LitModel().cuda().eval().model(batch["images"])
        assert tuple(logits.shape) == (4, 51) and bool(torch.isfinite(logits).all())
    finally:
        Ld.images_to_device = T.images_to_device = old
        gin.clear_config()
    assert res["global_step"] == 3
    train_rows = [h for h in res["history"] if "train/celoss" in h]
    assert len(train_rows) == 3 and all(np.isfinite(h["train/celoss"]) for h in train_rows)
    val = [h for h in res["history"] if "val/acc" in h]
    assert len(val) == 1 and np.isfinite(val[0]["val/loss"])
    # the first evaluation batch is the first four frames in sorted order, through CenterCrop
    batch, images = seen["eval"]
    paths = sorted(frames)[:4]
    for b, p in enumerate(paths):
        H, W = frames[p].shape[:2]
        o = int(batch["offsets"][b])
        assert np.array_equal(batch["packed"][o:o + 3 * W * H].numpy().reshape(H, W, 3), frames[p])
        want = R.run_program(frames[p], batch["programs"][b].numpy(), S)[0]
        assert np.array_equal(images[b].view(np.uint32), want.view(np.uint32)), p
