"""Time the segmentation augmentation (`mink_augment_seg_scenes`, the reference's ScanNet recipe with every gate forced)
of a ScanNet-shaped batch -- 8 scenes of 50-100 k rows -- on the prepare stream with events, and the float64 CPU
restatement of the same batch on one thread.  Prints one JSON line.

    timeout -k 10 300 python scripts/seg_augment_bench.py [--iters 50]"""
import argparse
import json
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the CPU restatement runs on one thread
    os.environ[_v] = "1"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--cpu-scenes", type=int, default=8, help="scenes of the CPU restatement timing")
    args = ap.parse_args()
    from seg_restate import stagewise, synthetic_scannet_batch
    from test_gpu_seg_augment import SEED, _programs

    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.data import seg_transforms as S

    coords, feats, labels, dists, offs = synthetic_scannet_batch(0)
    stages, params, streams = _programs("full", offs, coords)
    dc, df, do = torch.from_numpy(coords).cuda(), torch.from_numpy(feats).cuda(), torch.from_numpy(offs).cuda()
    ds, hp = torch.from_numpy(streams.view(np.int32)).cuda(), torch.from_numpy(params)
    raw = S.raw_columns(["density", "sh"])
    side = torch.cuda.Stream()
    ms, host_ms = [], []
    with torch.cuda.stream(side):
        for it in range(args.iters + 5):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            h = time.perf_counter()
            t0.record()
            out = ME.utils.augment_seg_batch(dc, df, do, hp, ds, SEED, raw, count_async=True)
            t1.record()
            h = time.perf_counter() - h
            t1.synchronize()
            if it >= 5:
                ms.append(t0.elapsed_time(t1))
                host_ms.append(h * 1e3)
    kept = int(out[3][0][0])
    # every grid over its bound: the displacement evaluated point by point, without stored grids (the crop fall-back path)
    direct_ms = []
    with torch.cuda.stream(side):
        for it in range(10):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            ME.utils.augment_seg_batch(dc, df, do, hp, ds, SEED, raw, count_async=True, grid_bound=np.full((len(offs) - 1, 3), 4))
            t1.record()
            t1.synchronize()
            if it >= 2:
                direct_ms.append(t0.elapsed_time(t1))
    t = time.perf_counter()
    for b in range(args.cpu_scenes):
        lo, hi = int(offs[b]), int(offs[b + 1])
        stagewise(coords[lo:hi, 1:], feats[lo:hi], stages[b], int(streams[b]), SEED, raw)
    cpu_ms = (time.perf_counter() - t) * 1e3 * (len(offs) - 1) / args.cpu_scenes
    grid = int(np.prod(S.grid_bounds(params), axis=1).sum())
    print(json.dumps({"bench": "seg_augment", "scenes": len(offs) - 1, "rows": int(len(coords)), "survivors": kept,
                      "grid_bound_nodes": grid, "gpu_ms_median": float(np.median(ms)), "gpu_ms_min": float(np.min(ms)),
                      "host_call_ms_median": float(np.median(host_ms)), "gpu_ms_median_no_stored_grid": float(np.median(direct_ms)),
                      "cpu_restatement_ms_1thread": cpu_ms}))


if __name__ == "__main__":
    main()
