#!/usr/bin/env python
"""Times instance norm and layer norm, forward + backward, in one process with device events:

  instance norm : the segmented kernels (InstanceNormFunction: 3 + 4 launches whatever B is, offsets read on the device)
                  against the slice-and-concatenate path MinkowskiInstanceNorm used before them (batch offsets read back
                  with .tolist(), one BatchNormFunction per sample, torch.cat), restated here so both run on one build
  layer norm    : LayerNormFunction (1 + 2 launches) against torch.nn.functional.layer_norm

at the rows x channels a Res16UNet14 training step normalises on ScanNet batches of B in {1, 4, 16} scenes: ~150 k voxels
per scene at tensor stride 1 (scripts/seghead_bench.py's 1.2 M rows are 8 such scenes), a quarter of the rows per level
below, PLANES (32, 48, 64, 96, 96, 96, 64, 64).  The two paths alternate, ROUNDS times each, after a warm-up; the median is
reported.  Bytes: the two-pass minimum of instance norm moves 12 B / element forward (read x twice, write y) and 20 backward
(read dy and x twice, write dx); layer norm 8 + 12.  Achieved bytes/s = that minimum over the measured time.

    python scripts/norm_bench.py [--out profiles/norm_bench.txt]"""
import argparse
import itertools
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

LEVELS = [(150_000, 32), (150_000, 64), (37_500, 32), (37_500, 48), (9_400, 64), (2_350, 96), (600, 96)]  # (rows per scene, C)
BATCHES = (1, 4, 16)
WARMUP, ITERS, ROUNDS = 5, 20, 3


def scene_sizes(rows, B, seed):
    g = torch.Generator().manual_seed(seed)
    return [max(1, int(rows * (0.8 + 0.4 * float(torch.rand(1, generator=g))))) for _ in range(B)]


def segmented_in(x, off, gamma, beta, dy, Fn):
    y = Fn.InstanceNormFunction.apply(x, gamma, beta, off, 1e-8, None, False)
    y.backward(dy)


def sliced_in(x, off, gamma, beta, dy, Fn):
    boff = off.tolist()
    parts = [Fn.BatchNormFunction.apply(x[s:e], gamma, beta, None, None, True, 0.0, 1e-8, None, False, None)
             for s, e in zip(boff[:-1], boff[1:]) if e > s]
    torch.cat(parts, 0).backward(dy)


def hip_ln(x, gamma, beta, dy, Fn):
    Fn.LayerNormFunction.apply(x, gamma, beta, 1e-5, None, False).backward(dy)


def torch_ln(x, gamma, beta, dy, Fn):
    torch.nn.functional.layer_norm(x, (x.shape[1],), gamma, beta, 1e-5).backward(dy)


def timed(fn, args, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        for t in args:
            if torch.is_tensor(t) and t.requires_grad:
                t.grad = None
        fn(*args)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # microseconds


def compare(new, old, args_new, args_old):
    for _ in range(WARMUP):
        new(*args_new), old(*args_old)
    t_new, t_old = [], []
    for _ in range(ROUNDS):
        t_new.append(timed(new, args_new, ITERS))
        t_old.append(timed(old, args_old, ITERS))
    return statistics.median(t_new), statistics.median(t_old), max(t_new) - min(t_new), max(t_old) - min(t_old)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("norm_bench measures on the GPU only")
    from nerf_downstream_amd.minkowski import functional as Fn

    lines = [f"device: {torch.cuda.get_device_name(0)}; forward + backward, microseconds per call, median of {ROUNDS} x {ITERS} after {WARMUP} warm-up calls; "
             "GB/s = two-pass minimum bytes / measured time",
             "instance norm: segmented kernels (7 launches for every B) vs one batch norm per sample + cat (offsets read back)",
             f"{'B':>3} {'rows':>9} {'C':>4} {'segmented us':>13} {'spread':>7} {'sliced us':>10} {'spread':>7} {'speed-up':>9} {'GB/s':>7}"]
    # process warm-up: code objects, the allocator's pools and the device's clocks settle on a throw-away shape first -- the
    # per-shape warm-up does not cover the start of the process
    xw = (torch.randn(600_000, 64, device="cuda")).requires_grad_(True)
    offw = torch.tensor([0, 200_000, 600_000], dtype=torch.int32, device="cuda")
    gw, bw = torch.ones(64, device="cuda", requires_grad=True), torch.zeros(64, device="cuda", requires_grad=True)
    dyw = torch.randn(600_000, 64, device="cuda")
    for _ in range(3):
        compare(segmented_in, sliced_in, (xw, offw, gw, bw, dyw, Fn), (xw, offw, gw, bw, dyw, Fn))
        compare(hip_ln, torch_ln, (xw, gw, bw, dyw, Fn), (xw, gw, bw, dyw, Fn))
    del xw, dyw
    worst = None
    # (B, rows per scene, C, sizes or None): the even batches; the B = 1 block once more at the end, as a check that the first
    # block was measured on a settled device; and one UNEVEN batch -- every sample gets the same number of row chunks, so one
    # large scene among 15 small ones is reduced by 2048 / 16 = 128 workgroups only
    cases = [(B, rows, C, None) for B in BATCHES for rows, C in LEVELS] + [(1, rows, C, None) for rows, C in LEVELS]
    cases += [(16, 150_000, C, [1_500_000] + [60_000] * 15) for C in (32, 64)]
    for B, rows, C, sizes in cases:
        if True:
            uneven = sizes is not None
            sizes = sizes or scene_sizes(rows, B, seed=rows + B)
            n = sum(sizes)
            off = torch.tensor([0] + list(itertools.accumulate(sizes)), dtype=torch.int32, device="cuda")
            x = (torch.randn(n, C, device="cuda") * 1.5 + 0.2).requires_grad_(True)
            gamma, beta = torch.ones(C, device="cuda", requires_grad=True), torch.zeros(C, device="cuda", requires_grad=True)
            dy = torch.randn(n, C, device="cuda")
            a = (x, off, gamma, beta, dy, Fn)
            t_new, t_old, s_new, s_old = compare(segmented_in, sliced_in, a, a)
            gbs = 32.0 * n * C / (t_new * 1e-6) / 1e9
            lines.append(f"{B:>3} {n:>9} {C:>4} {t_new:>13.1f} {s_new:>7.1f} {t_old:>10.1f} {s_old:>7.1f} {t_old / t_new:>9.2f} {gbs:>7.0f}"
                         + ("  uneven: one scene of 1.5 M rows, 15 of 60 k" if uneven else ""))
            if worst is None or t_old / t_new < worst[0]:
                worst = (t_old / t_new, B, n, C)
    lines.append(f"smallest speed-up over the sliced path: {worst[0]:.2f}x at B={worst[1]}, rows={worst[2]}, C={worst[3]}")
    lines += ["layer norm: LayerNormFunction (3 launches) vs torch.nn.functional.layer_norm",
              f"{'rows':>9} {'C':>4} {'hip us':>8} {'spread':>7} {'torch us':>9} {'spread':>7} {'speed-up':>9} {'GB/s':>7}"]
    for B in BATCHES:
        for rows, C in LEVELS:
            n = rows * B
            x = (torch.randn(n, C, device="cuda") * 1.5 + 0.2).requires_grad_(True)
            gamma, beta = torch.ones(C, device="cuda", requires_grad=True), torch.zeros(C, device="cuda", requires_grad=True)
            dy = torch.randn(n, C, device="cuda")
            a = (x, gamma, beta, dy, Fn)
            t_new, t_old, s_new, s_old = compare(hip_ln, torch_ln, a, a)
            gbs = 20.0 * n * C / (t_new * 1e-6) / 1e9
            lines.append(f"{n:>9} {C:>4} {t_new:>8.1f} {s_new:>7.1f} {t_old:>9.1f} {s_old:>7.1f} {t_old / t_new:>9.2f} {gbs:>7.0f}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
