#!/usr/bin/env python
"""Times the generative layers (csrc/generate.hip, minkowski/generative.py) against what the backend offered for the same result
before they existed.  For the record, not a threshold.

  pruning     half of 800 k rows x 32 channels (4 scenes of 200 k voxels at tensor stride 1; a random half kept):
              ME.MinkowskiPruning  vs  boolean indexing with torch + SparseTensor(coordinates=...) on the kept rows.
              Both sides end with a usable tensor on a manager of its own, so both include one hash build of the kept rows and
              its host read-back; the row marked `kernels` is mink_prune_compact + mink_prune_gather alone.
  generation  one generative block at 100 k parents (tensor stride 2 -> 800 k children), 32 -> 16 channels:
              ME.MinkowskiGenerativeConvolutionTranspose (which builds the children's map every call)  vs  the existing
              MinkowskiConvolutionTranspose(2, 2) onto a PREBUILT map of all children with its tables cached -- the comparison
              favours the old layer by the whole map build, which it could not do inside a network at all.

Milliseconds per call on a host clock around work that ends in a device synchronise (the layers read counts back, so device
events alone would miss host time); the two sides alternate round by round; median of ROUNDS x ITERS after a warm-up, spread =
max - min of the rounds.

    python scripts/generative_bench.py [--out profiles/generative_bench.txt]"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, C = 4, 32
PRUNE_ROWS, PARENTS, COUT = 200_000, 25_000, 16  # per scene
BOX = (128, 128, 32)
WARMUP, ITERS, ROUNDS = 3, 10, 5


def scenes(rows, ts=1, seed=0):
    g = torch.Generator().manual_seed(seed)
    out = []
    for b in range(B):
        cell = torch.randperm(BOX[0] * BOX[1] * BOX[2], generator=g)[:rows].sort().values
        xyz = torch.stack([cell % BOX[0], cell // BOX[0] % BOX[1], cell // (BOX[0] * BOX[1])], 1) * ts
        out.append(torch.cat([torch.full((rows, 1), b), xyz], 1))
    return torch.cat(out).int()


def timed(fn, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / iters  # milliseconds


def measure(fns):
    """{name: fn} -> {name: (median ms, spread ms)}, the candidates alternating round by round."""
    for fn in fns.values():
        for _ in range(WARMUP):
            fn()
    t = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            t[k].append(timed(fn, ITERS))
    return {k: (statistics.median(v), max(v) - min(v)) for k, v in t.items()}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("generative_bench measures on the GPU only")
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd._lib import check, lib
    from nerf_downstream_amd.minkowski import generative as G

    lines = [f"device: {torch.cuda.get_device_name(0)}; milliseconds per call, host clock to a device synchronise, median of {ROUNDS} x {ITERS} "
             f"after {WARMUP} warm-up calls, candidates alternating (spread = max - min of the rounds)",
             f"{'case':<78} {'fwd ms':>8} {'spread':>7} {'fwd+bwd ms':>11} {'spread':>7}"]

    def rows(cases):
        fwd = measure({k: f for k, (f, _) in cases.items()})
        both = measure({k: b for k, (_, b) in cases.items() if b is not None})
        for k in cases:
            tb = both.get(k)
            lines.append(f"{k:<78} {fwd[k][0]:>8.3f} {fwd[k][1]:>7.3f} " + (f"{tb[0]:>11.3f} {tb[1]:>7.3f}" if tb else f"{'-':>11} {'-':>7}"))

    # ---- pruning
    coords = scenes(PRUNE_ROWS).cuda()
    n = coords.shape[0]
    x = ME.SparseTensor(torch.randn(n, C, device="cuda").requires_grad_(True), coordinates=coords)
    mask = torch.rand(n, device="cuda") < 0.5
    k = int(mask.sum())
    dy = torch.randn(k, C, device="cuda")
    prune = ME.MinkowskiPruning()

    def new_prune():
        return prune(x, mask)

    def old_prune():
        return ME.SparseTensor(x.F[mask], coordinates=x.C[mask])

    def fwd(fn):
        def run():
            with torch.no_grad():
                fn()
        return run

    def both(fn, g):
        def run():
            x.F.grad = None
            fn().F.backward(g)
        return run

    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    m = x.coordinate_manager
    ws = torch.empty(int(L.mink_prune_workspace_bytes(n)), dtype=torch.uint8, device="cuda")
    idx = torch.empty(2 * n + B + 2, dtype=torch.int32, device="cuda")
    oc, y = torch.empty(n, 4, dtype=torch.int32, device="cuda"), torch.empty(k, C, device="cuda")
    xf = x.F.detach()

    def kernels():
        check(L.mink_prune_compact(mask.data_ptr(), x.C.data_ptr(), n, B, idx.data_ptr(), idx[n:].data_ptr(), oc.data_ptr(),
                                   idx[2 * n:].data_ptr(), idx[2 * n + B + 1:].data_ptr(), ws.data_ptr(), ws.numel(), st))
        check(L.mink_prune_gather(xf.data_ptr(), C, n, C, idx.data_ptr(), k, y.data_ptr(), C, st))

    assert m.batch_size() == B
    rows({f"pruning {n} x {C} -> {k}: ME.MinkowskiPruning": (fwd(new_prune), both(new_prune, dy)),
          f"pruning {n} x {C} -> {k}: x.F[mask] + SparseTensor(coordinates=x.C[mask])": (fwd(old_prune), both(old_prune, dy)),
          f"pruning {n} x {C} -> {k}: kernels (compaction + row gather, no map build)": (kernels, None)})
    moved = n + 16 * n + 4 * 2 * n + 16 * k + 2 * 4 * C * k  # mask, coordinates, kept + old2new, kept coordinates, rows in and out
    lines.append(f"  (the kernels row moves at least {moved / 1e6:.1f} MB)")

    # ---- one generative block
    parents = scenes(PARENTS, ts=2, seed=1).cuda()
    p = parents.shape[0]
    xp = torch.randn(p, C, device="cuda").requires_grad_(True)
    coarse = ME.SparseTensor(xp, ME.CoordinateMapKey(2), ME.CoordinateManager.from_coordinates(parents, 2, B))
    gen = ME.MinkowskiGenerativeConvolutionTranspose(C, COUT).cuda()
    up = ME.MinkowskiConvolutionTranspose(C, COUT, kernel_size=2, stride=2, dimension=3).cuda()
    up.load_state_dict(gen.state_dict())
    kids = G.generate_children(parents, 2)
    fine = ME.TensorField(coordinates=kids.float(), features=torch.zeros(8 * p, 1, device="cuda")).sparse()
    fm = fine.coordinate_manager
    ckey = fm.stride(fine.coordinate_map_key, 2)
    assert torch.equal(fm.get_coordinates(ckey), parents)
    coarse_full = ME.SparseTensor(xp, ckey, fm)
    dz = torch.randn(8 * p, COUT, device="cuda")

    def new_gen():
        return gen(coarse)

    def old_up():
        return up(coarse_full)

    def both_p(fn):
        def run():
            xp.grad = None
            fn().F.backward(dz)
        return run

    assert torch.allclose(new_gen().F, old_up().F, atol=2e-5, rtol=1e-5)  # same result before either is timed
    rows({f"generation {p} x {C} -> {8 * p} x {COUT}: ME.MinkowskiGenerativeConvolutionTranspose": (fwd(new_gen), both_p(new_gen)),
          f"generation {p} x {C} -> {8 * p} x {COUT}: MinkowskiConvolutionTranspose, prebuilt map + tables": (fwd(old_up), both_p(old_up)),
          f"generation {p} -> {8 * p}: mink_generate_children alone": (lambda: G.generate_children(parents, 2), None)})
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
