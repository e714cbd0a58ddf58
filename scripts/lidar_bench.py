"""Times the LiDAR input of a batch of SemanticKITTI-shaped scans on the GPU (minkowski/utils.py prepare_lidar_batch:
`mink_lidar_decode_scans`, `mink_voxel_downsample_scenes`, `mink_augment_seg_scenes`, `mink_lidar_finish_rows`), the two new
kernels alone, and the numpy restatement of the same preparation (tests/lidar_restate.py) on the host.

    python scripts/lidar_bench.py [--out profiles/lidar_kernels.txt] [--repeats 5] [--scans 4] [--points 120000]

  shape   : 4 synthetic scans of 120 k returns over +-80 m (tests/lidar_restate.py synthetic_scan), down-sampled at 0.025 m,
            voxel size 0.05 m, the default recipe (CoordinateDropout, RandomHorizontalFlip, RandomAffine, RandomTranslation)
            with every stage drawn
  device  : device-event time per call over windows of back-to-back calls after a warm-up of the same shape
            (scripts/dgcnn_bench.py time_windows, as scripts/fps_bench.py): the whole `prepare_lidar_batch(count_async=True)`
            (nothing is read back inside a window), `lidar_decode_batch` alone and `lidar_finish_rows` alone (voxel size 1, so
            that the in-place division leaves the values where they are from call to call); the three alternate window by
            window.  A single-kernel call is a few microseconds of work: its window shows the host's launch pace, not the kernel
  host    : host clock around `lidar_restate.prepare_scene` over the same scans, one after the other

Every figure is the median [min .. max] over `--repeats` windows.  The device figures need the GPU: there is no CPU path."""
import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--scans", type=int, default=4)
    ap.add_argument("--points", type=int, default=120_000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lidar_bench needs the GPU"
    from dgcnn_bench import time_windows
    from lidar_restate import label_table, prepare_scene, synthetic_scan

    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as ST
    from nerf_downstream_amd.co3d_3d.src.data.transforms import CoordinateDropout, RandomAffine, RandomHorizontalFlip, RandomTranslation
    from nerf_downstream_amd.minkowski.utils import lidar_decode_batch, lidar_finish_rows, prepare_lidar_batch

    dev = torch.device("cuda")
    q, voxel, ignore, seed = 0.025, 0.05, -100, 0x5EED5EED5EED
    rng = np.random.default_rng(0)
    pairs = [synthetic_scan(rng, args.points) for _ in range(args.scans)]
    scans, words = [p[0] for p in pairs], [p[1] for p in pairs]
    offs = np.concatenate([[0], np.cumsum([len(s) for s in scans])]).astype(np.int32)
    table, _ = label_table(ignore)
    comp = ST.PointCompose([CoordinateDropout(0.2, application_ratio=1), RandomHorizontalFlip("z", application_ratio=1),
                            RandomAffine(application_ratio=1), RandomTranslation(application_ratio=1)])
    random.seed(0), np.random.seed(0)
    drawn = [comp.sample((s[:, :3].max(0) - s[:, :3].min(0)).astype(np.float64)) for s in scans]
    P, streams = np.stack([d[0] for d in drawn]), np.array([d[2] for d in drawn], np.uint32)
    batch = {"scan": torch.from_numpy(np.concatenate(scans)).to(dev), "scene_offsets": torch.from_numpy(offs).to(dev),
             "raw_labels": torch.from_numpy(np.concatenate(words).view(np.int32)).to(dev), "label_lut": torch.from_numpy(table).to(dev),
             "lidar_params": np.array([[q, voxel, ignore]] * len(scans), np.float64), "feature_names": ("xyzi",),
             "aug_params": torch.from_numpy(P), "aug_streams": torch.from_numpy(streams.view(np.int32).copy()).to(dev), "aug_seed": seed}
    lut32 = batch["label_lut"].to(torch.int32)
    c, f, _, _ = prepare_lidar_batch(batch)
    k = int(c.shape[0])
    reach = float(c[:, 1:].abs().max())  # the largest voxel coordinate the coordinate maps would key (their field: +-32767)
    fc, ff = torch.zeros(int(offs[-1]), 4, device=dev), torch.zeros(int(offs[-1]), 4, device=dev)
    fc[:k], ff[:k] = c, f
    count = torch.tensor([k], dtype=torch.int32, device=dev)
    fns = [lambda: prepare_lidar_batch(batch, count_async=True),
           lambda: lidar_decode_batch(batch["scan"], batch["raw_labels"], batch["scene_offsets"], lut32, ignore),
           lambda: lidar_finish_rows(fc, ff, count, 1.0)]
    whole, dec, fin = time_windows(fns, args.repeats)

    host = []
    for _ in range(args.repeats):
        t = time.perf_counter()
        rows = 0
        for s in range(len(scans)):
            rows += len(prepare_scene(scans[s], words[s], table, q, voxel, ignore, P[s], streams[s], seed)[3])
        host.append((time.perf_counter() - t) * 1e3)
    assert rows == k, (rows, k)  # the two prepared the same batch
    host = (statistics.median(host), min(host), max(host))

    fmt = lambda t: f"{t[0]:9.3f} [{t[1]:.3f} .. {t[2]:.3f}] ms"  # noqa: E731
    n = int(offs[-1])
    lines = [f"lidar_bench: the LiDAR input on the device and its numpy restatement on the host, fp32, {torch.cuda.get_device_name(0)}",
             f"{len(scans)} scans of {args.points} points ({n} per batch) over +-80 m, down-sampling {q} m, voxel size {voxel} m, every "
             f"stage of the default recipe drawn; {k} rows survive, largest |voxel coordinate| {reach:.0f}; median [min .. max] per call "
             f"over {args.repeats} windows", "",
             f"prepare_lidar_batch (decode, down-sampling, recipe, finish; device events) {fmt(whole)}",
             f"  lidar_decode_batch alone, {n} rows (launch-paced, see below)             {fmt(dec)}",
             f"  lidar_finish_rows alone, {k} rows (launch-paced, see below)              {fmt(fin)}",
             f"numpy restatement of the same preparation on the host (host clock)       {fmt(host)}", "",
             "The two single-kernel lines are NOT kernel times and give no bandwidth: each call is one launch of a few microseconds of",
             f"work ({n * 56 / 1e6:.0f} MB and {k * 64 / 1e6:.0f} MB that stay in the last-level cache) issued through ctypes, the decode call with four",
             "torch.empty allocations, so the window measures the pace at which one host thread issues such calls: an upper bound on",
             "the kernels.  The whole preparation is back-to-back calls from one host thread too: where the host issues its launches",
             "more slowly than the device runs them, the window holds that."]
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
