#!/usr/bin/env python
"""Times the sparse pooling family (csrc/pool.hip) in one process with device events, scripts/kbench.py style, at the
rows x channels of level 0 of a Res16UNet / FCNN step on ScanNet batches: B = 4 scenes of ~150 k voxels at tensor stride 1
(scripts/norm_bench.py's shape), C = 32.  The scenes are uniformly random occupied cells of a 128 x 128 x 32 box (29 % full):
denser windows than a scanned surface has, so the local pools gather more rows per output here than on real scans.

Per operator: forward alone (no autograd graph) and forward + backward, microseconds per call, median of ROUNDS x ITERS
after a warm-up; GB/s = the bytes the pass must move at least (features read once per present table entry for the local
pools -- the table itself included --, once per row for the global pools, outputs written once) over the measured time.

    python scripts/pool_bench.py [--out profiles/pool_bench.txt]"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, ROWS, C = 4, 150_000, 32
BOX = (128, 128, 32)
WARMUP, ITERS, ROUNDS = 5, 20, 3


def scenes(seed=0):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for b in range(B):
        cell = torch.randperm(BOX[0] * BOX[1] * BOX[2], generator=g)[:ROWS]
        xyz = torch.stack([cell % BOX[0], cell // BOX[0] % BOX[1], cell // (BOX[0] * BOX[1])], 1)
        rows.append(torch.cat([torch.full((ROWS, 1), b), xyz], 1))
    return torch.cat(rows).int()


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3 / iters  # microseconds


def measure(fn):
    for _ in range(WARMUP):
        fn()
    t = [timed(fn, ITERS) for _ in range(ROUNDS)]
    return statistics.median(t), max(t) - min(t)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("pool_bench measures on the GPU only")
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.minkowski import functional as Fn

    coords = scenes().cuda()
    n = coords.shape[0]
    st = ME.SparseTensor(torch.zeros(n, 1, device="cuda"), coordinates=coords)
    m, key1 = st.coordinate_manager, ME.CoordinateMapKey(1)
    boff = m.batch_offsets(key1)
    x = torch.randn(n, C, device="cuda").requires_grad_(True)
    lines = [f"device: {torch.cuda.get_device_name(0)}; {B} scenes x {ROWS} voxels = {n} rows at tensor stride 1, C = {C}; microseconds per call, "
             f"median of {ROUNDS} x {ITERS} after {WARMUP} warm-up calls (spread = max - min of the rounds)",
             f"{'operator':<40} {'rows out':>9} {'pairs':>9} {'fwd us':>8} {'spread':>7} {'fwd GB/s':>9} {'fwd+bwd us':>11} {'spread':>7}"]

    def row(name, fn, n_out, pairs, fwd_bytes):
        dy = torch.randn(n_out, C, device="cuda")

        def fwd():
            with torch.no_grad():
                fn()

        def both():
            x.grad = None
            out = fn()
            (out[0] if isinstance(out, tuple) else out).backward(dy)

        t_f, s_f = measure(fwd)
        t_b, s_b = measure(both)
        lines.append(f"{name:<40} {n_out:>9} {pairs:>9} {t_f:>8.1f} {s_f:>7.1f} {fwd_bytes / (t_f * 1e-6) / 1e9:>9.0f} {t_b:>11.1f} {s_b:>7.1f}")

    for k, s in ((2, 2), (3, 2), (3, 1)):
        out_key = m.stride(key1, s)
        nbr, nbr_t = m.kernel_table(key1, out_key, k, 1, transposed=True)
        n_out, pairs = nbr.shape[0], int((nbr >= 0).sum())
        fwd_bytes = 4 * C * (pairs + n_out) + 4 * nbr.numel()
        for name, f in (("avg", Fn.AvgPoolFunction), ("sum (overlapping kernels)", Fn.OverlapSumPoolFunction), ("max", Fn.SparseMaxPoolFunction)):
            extra = 4 * C * n_out if name == "max" else 0  # (arg)
            row(f"local {name} k={k} s={s}", lambda f=f: f.apply(x, nbr, nbr_t), n_out, pairs, fwd_bytes + extra)
        if (k, s) == (2, 2):
            i2o = m.stride_map(key1, out_key)
            row("local sum k=2 s=2 (mink_pool_sum_*)", lambda: Fn.SumPoolFunction.apply(x, nbr, i2o), n_out, pairs, fwd_bytes)
    row("global max", lambda: Fn.GlobalMaxPoolFunction.apply(x, boff), B, n, 4 * C * n)
    row("global sum", lambda: Fn.GlobalSumPoolFunction.apply(x, boff), B, n, 4 * C * n)
    row("global avg (mink_global_avg_*)", lambda: Fn.GlobalAvgPoolFunction.apply(x, boff), B, n, 4 * C * n)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
