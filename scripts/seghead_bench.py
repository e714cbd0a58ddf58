#!/usr/bin/env python3
"""Times the tail of a segmentation step two ways, in one process, with device events:

  (a) the torch expressions the trainer used before csrc/seghead.hip: F.cross_entropy(weight, ignore_index) forward +
      backward, argmax, confusion(), the ignore-ratio mean;
  (b) one seg_cross_entropy(want_pred=True, want_hist=True) forward + backward.

Per shape (N, C) and with / without class weights it prints microseconds per call (mean over the timed iterations,
alternating (a) and (b) blocks), the peak extra device memory of one call and, for (b), the achieved GB/s against the
algorithmic bytes N * (4C + 8 + 4 + 4) forward and N * (8C + 8 + 4) backward.  Kernel launch counts come from a separate
`rocprofv3 --kernel-trace --stats -- python scripts/seghead_bench.py --iters 5 --warmup 2` run.

    python scripts/seghead_bench.py [--iters 50] [--warmup 10]
"""
import argparse
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_downstream_amd import minkowski as ME  # noqa: E402
from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import confusion  # noqa: E402

SHAPES = [(1_200_000, 20), (1_200_000, 21), (200_000, 8)]
IGNORE = 255


def make(n, C, weighted, seed=0):
    rng = np.random.default_rng(seed)
    z = np.clip(rng.normal(0.0, 3.0, (n, C)), -16.0, 16.0).astype(np.float32)
    y = rng.integers(0, C, n).astype(np.int64)
    y[rng.random(n) < 0.05] = IGNORE
    w = None
    if weighted:
        w = torch.ones(C, device="cuda")
        w[-1] = 0.3
    return torch.from_numpy(z).cuda().requires_grad_(True), torch.from_numpy(y).cuda(), w


def torch_tail(z, y, w):
    loss = F.cross_entropy(z, y, weight=w, ignore_index=IGNORE)
    loss.backward()
    with torch.no_grad():
        hist = confusion(z.argmax(1), y, z.shape[1])
        ratio = (y == IGNORE).float().mean()
    return loss, hist, ratio


def hip_tail(z, y, w):
    loss, pred, hist, stats = ME.seg_cross_entropy(z, y, weight=w, ignore_index=IGNORE, want_pred=True, want_hist=True)
    loss.backward()
    return loss, hist, stats


def hip_forward(z, y, w):
    with torch.no_grad():
        return ME.seg_cross_entropy(z, y, weight=w, ignore_index=IGNORE, want_pred=True, want_hist=True)


def timed(fn, z, y, w, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        z.grad = None
        fn(z, y, w)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # microseconds


def peak_extra(fn, z, y, w):
    z.grad = None
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn(z, y, w)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--iters", type=int, default=50)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=3, help="alternating (a) / (b) blocks of --iters calls each")
    args = p.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("seghead_bench needs the GPU: a CPU timing says nothing about it")
    print(f"# device: {torch.cuda.get_device_name(0)}; {args.iters} iterations x {args.rounds} alternating rounds after {args.warmup} warm-up calls")
    print("# N C weights | (a) torch us | (b) hip us | (a)/(b) | (b) fwd us, GB/s | (b) bwd us, GB/s | peak extra MiB (a), (b) | N*C*4 MiB")
    for n, C in SHAPES:
        for weighted in (False, True):
            z, y, w = make(n, C, weighted)
            for _ in range(args.warmup):
                for fn in (torch_tail, hip_tail, hip_forward):
                    z.grad = None
                    fn(z, y, w)
            torch.cuda.synchronize()
            ta, tb, tf = [], [], []
            for _ in range(args.rounds):
                ta.append(timed(torch_tail, z, y, w, args.iters))
                tb.append(timed(hip_tail, z, y, w, args.iters))
                tf.append(timed(hip_forward, z, y, w, args.iters))
            a, b, f = float(np.mean(ta)), float(np.mean(tb)), float(np.mean(tf))
            bwd = max(b - f, 1e-3)
            fwd_bytes, bwd_bytes = n * (4 * C + 8 + 4 + 4), n * (8 * C + 8 + 4)
            pa, pb = peak_extra(torch_tail, z, y, w), peak_extra(hip_tail, z, y, w)
            mib = 1 << 20
            print(f"{n} {C} {'w' if weighted else '-'} | {a:9.1f} (spread {min(ta):.1f}-{max(ta):.1f}) | {b:9.1f} (spread {min(tb):.1f}-{max(tb):.1f}) | "
                  f"{a / b:5.2f} | {f:8.1f} {fwd_bytes / f / 1e3:7.1f} | {bwd:8.1f} {bwd_bytes / bwd / 1e3:7.1f} | "
                  f"{pa / mib:7.1f} {pb / mib:7.1f} | {n * C * 4 / mib:6.1f}", flush=True)
            del z, y, w
    return 0


if __name__ == "__main__":
    sys.exit(main())
