#!/usr/bin/env python
"""Times the union of sparse tensors (csrc/union.hip, minkowski/union.py) against the same result composed from torch
operations on the same device.  For the record, not a threshold.

  shape 1   two inputs of 826 k rows (the bench batch's voxel count) x 32 channels over 4 samples, about half of the rows of
            each shared with the other
  shape 2   one decoder level's own pair: the 8 n children of n = 100 k parents (tensor stride 2 -> 1) against an encoder
            tensor that holds half of those children and 50 k voxels the decoder did not generate

  kernels   mink_union_build (hash of all rows, compaction, in2out / out2in / offsets; no host read), mink_union_sum, and
            the backward: one mink_prune_gather per input
  torch     torch.cat of the coordinate lists, torch.unique(dim=0, return_inverse=True), index_add_ of every input's rows; the
            backward: dy[inverse] per input.  Its union comes out in lexicographic order, ours in the documented input order,
            so the results are compared through a lexicographic sort of ours before either is timed.
  module    ME.MinkowskiUnion end to end: the above plus the one host read of the count and the derived manager's own map
            build (CoordinateManager.from_coordinates), which the torch composition would need as well before any layer could
            run on its result.

Milliseconds per call on a host clock around work that ends in a device synchronise; the candidates alternate round by round;
median of ROUNDS x ITERS after a warm-up, spread = max - min of the rounds.  Peak memory: torch.cuda.max_memory_allocated over
one call, above what was allocated before it.

    python scripts/union_bench.py [--out profiles/union_kernels.txt]"""
import argparse
import ctypes
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

B, C = 4, 32
BOX = (128, 128, 64)
WARMUP, ITERS, ROUNDS = 3, 10, 5


def cells_to_rows(b, cell, ts=1):
    xyz = torch.stack([cell % BOX[0], cell // BOX[0] % BOX[1], cell // (BOX[0] * BOX[1])], 1) * ts
    return torch.cat([torch.full((cell.shape[0], 1), b), xyz], 1)


def overlapping_pair(rows_per_scene, seed=0):
    """Two lists of B * rows_per_scene rows; the second half of each scene's rows in the first is the first half in the second."""
    g, a, b = torch.Generator().manual_seed(seed), [], []
    half = rows_per_scene // 2
    for s in range(B):
        cell = torch.randperm(BOX[0] * BOX[1] * BOX[2], generator=g)[: rows_per_scene + half]
        a.append(cells_to_rows(s, cell[:rows_per_scene].sort().values))
        b.append(cells_to_rows(s, cell[half:].sort().values))
    return torch.cat(a).int(), torch.cat(b).int()


def decoder_pair(parents_per_scene, extra_per_scene, seed=1):
    """(children of the decoder's parents at tensor stride 1, encoder rows: half of those children + voxels it did not generate)"""
    from nerf_downstream_amd.minkowski import generative as G

    g, dec, enc = torch.Generator().manual_seed(seed), [], []
    box = (BOX[0] // 2) * (BOX[1] // 2) * (BOX[2] // 2)
    for s in range(B):
        cell = torch.randperm(box, generator=g)[: parents_per_scene + extra_per_scene // 4]

        def parents(c):
            xyz = torch.stack([c % (BOX[0] // 2), c // (BOX[0] // 2) % (BOX[1] // 2), c // ((BOX[0] // 2) * (BOX[1] // 2))], 1) * 2
            return torch.cat([torch.full((c.shape[0], 1), s), xyz], 1).int().cuda()

        kids = G.generate_children(parents(cell[:parents_per_scene].sort().values), 2).cpu()
        others = G.generate_children(parents(cell[parents_per_scene:].sort().values), 2).cpu()
        dec.append(kids)
        keep = torch.rand(kids.shape[0], generator=g) < 0.5
        enc.append(torch.cat([kids[keep], others[torch.randperm(others.shape[0], generator=g)[:extra_per_scene]]]))
    return torch.cat(dec).int(), torch.cat(enc).int()


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


def peak_mb(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2 ** 20


def case(name, ca, cb, lines):
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd._lib import check, lib

    L, st = lib(), torch.cuda.current_stream().cuda_stream
    ca, cb = ca.cuda(), cb.cuda()
    ta = ME.SparseTensor(torch.randn(ca.shape[0], C, device="cuda").requires_grad_(True), ME.CoordinateMapKey(1),
                         ME.CoordinateManager.from_coordinates(ca, 1, B))
    tb = ME.SparseTensor(torch.randn(cb.shape[0], C, device="cuda").requires_grad_(True), ME.CoordinateMapKey(1),
                         ME.CoordinateManager.from_coordinates(cb, 1, B))
    xs, ns = [ta.F.detach(), tb.F.detach()], [ca.shape[0], cb.shape[0]]
    S = sum(ns)
    offs = [t.coordinate_manager.batch_offsets(t.coordinate_map_key) for t in (ta, tb)]
    union = ME.MinkowskiUnion()

    # ---- the same result both ways, before either is timed
    coords, in2out, out2in, _ = ME.union.union_map([ta, tb])
    N = coords.shape[0]
    with torch.no_grad():
        ours = union(ta, tb)
    allc = torch.cat([ca, cb])
    uc, inv = torch.unique(allc, dim=0, return_inverse=True)
    ref = torch.zeros(uc.shape[0], C, device="cuda").index_add_(0, inv[: ns[0]], xs[0]).index_add_(0, inv[ns[0]:], xs[1])
    key = ((coords[:, 0].long() * 65536 + coords[:, 1] + 32768) * 65536 + coords[:, 2] + 32768) * 65536 + coords[:, 3] + 32768
    order = torch.argsort(key)
    assert uc.shape[0] == N and torch.equal(coords[order], uc) and torch.equal(ours.F[order], ref)  # (two addends: the order cannot matter)

    # ---- kernels alone, into buffers allocated once
    n_host = (ctypes.c_int64 * 2)(*ns)
    ws = torch.empty(int(L.mink_union_workspace_bytes(2, n_host, B)), dtype=torch.uint8, device="cuda")
    idx = torch.empty(3 * S + B + 2, dtype=torch.int32, device="cuda")
    i2o = [idx[: ns[0]], idx[ns[0]: S]]
    o2i, boff, total = idx[S: 3 * S], idx[3 * S: 3 * S + B + 1], idx[3 * S + B + 1:]
    oc = torch.empty(S, 4, dtype=torch.int32, device="cuda")
    y, dy = torch.empty(N, C, device="cuda"), torch.randn(N, C, device="cuda")
    dx = [torch.empty(n, C, device="cuda") for n in ns]
    ptr = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])  # noqa: E731
    pc, po, pi, px, ld = ptr([ca, cb]), ptr(offs), ptr(i2o), ptr(xs), (ctypes.c_int32 * 2)(C, C)

    def k_build():
        check(L.mink_union_build(2, pc, po, n_host, B, oc.data_ptr(), pi, o2i.data_ptr(), S, boff.data_ptr(), total.data_ptr(), ws.data_ptr(),
                                 ws.numel(), st))

    def k_sum():
        check(L.mink_union_sum(2, px, ld, n_host, C, o2i.data_ptr(), S, N, y.data_ptr(), C, st))

    def k_bwd():
        for rows, g in zip(i2o, dx):
            check(L.mink_prune_gather(dy.data_ptr(), C, N, C, rows.data_ptr(), rows.shape[0], g.data_ptr(), C, st))

    def t_map():
        return torch.unique(torch.cat([ca, cb]), dim=0, return_inverse=True)

    def t_sum():
        return torch.zeros(N, C, device="cuda").index_add_(0, inv[: ns[0]], xs[0]).index_add_(0, inv[ns[0]:], xs[1])

    def t_bwd():
        return dy[inv[: ns[0]]], dy[inv[ns[0]:]]

    def m_fwd():
        with torch.no_grad():
            return union(ta, tb)

    def m_both():
        ta.F.grad = tb.F.grad = None
        union(ta, tb).F.backward(dy)

    k_build(), k_sum()
    assert int(total.item()) == N and torch.equal(y, ours.F)
    t = measure({"build": k_build, "unique": t_map, "sum": k_sum, "index_add": t_sum, "gathers": k_bwd, "index": t_bwd, "module": m_fwd,
                 "module both": m_both})
    mem = {"kernels": ws.numel() / 2 ** 20 + (idx.numel() * 4 + oc.numel() * 4 + y.numel() * 4) / 2 ** 20,
           "torch": peak_mb(lambda: (t_map(), t_sum())), "module": peak_mb(m_fwd)}
    head = f"{name}: {ns[0]} + {ns[1]} rows x {C} -> {N}"
    lines.append(head)
    pairs = [("map", "mink_union_build", "build", "torch.cat + torch.unique(dim=0, return_inverse=True)", "unique"),
             ("sum", "mink_union_sum", "sum", "zeros + index_add_ per input", "index_add"),
             ("backward", "mink_prune_gather per input", "gathers", "dy[inverse] per input", "index")]
    for what, ours_name, ko, theirs_name, kt in pairs:
        lines.append(f"  {what:<9} {ours_name:<28} {t[ko][0]:>8.3f} ms (spread {t[ko][1]:.3f})   {theirs_name:<52} {t[kt][0]:>8.3f} ms (spread {t[kt][1]:.3f})"
                     f"   torch / kernels = {t[kt][0] / t[ko][0]:.2f}")
    ours_all, theirs_all = t["build"][0] + t["sum"][0] + t["gathers"][0], t["unique"][0] + t["index_add"][0] + t["index"][0]
    lines.append(f"  {'all three':<9} {'kernels':<28} {ours_all:>8.3f} ms{'':<18} {'torch composition':<52} {theirs_all:>8.3f} ms{'':<18} torch / kernels = {theirs_all / ours_all:.2f}")
    lines.append(f"  ME.MinkowskiUnion end to end (count read back, derived manager built): forward {t['module'][0]:.3f} ms (spread {t['module'][1]:.3f}), "
                 f"forward + backward {t['module both'][0]:.3f} ms (spread {t['module both'][1]:.3f})")
    moved = 16 * S + 16 * N + 4 * S + 2 * 4 * N + 4 * C * (S + N)  # coordinates in and out, in2out, out2in, rows in and out
    lines.append(f"  memory: kernels' workspace + outputs {mem['kernels']:.1f} MiB (workspace {ws.numel() / 2 ** 20:.1f}), torch composition peak {mem['torch']:.1f} MiB, "
                 f"module peak {mem['module']:.1f} MiB; build + sum move at least {moved / 1e6:.1f} MB besides the hash")


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("union_bench measures on the GPU only")
    lines = [f"device: {torch.cuda.get_device_name(0)}; milliseconds per call, host clock to a device synchronise, median of {ROUNDS} x {ITERS} "
             f"after {WARMUP} warm-up calls, candidates alternating (spread = max - min of the rounds)"]
    case("shape 1, half overlap", *overlapping_pair(826_000 // B), lines)
    case("shape 2, a decoder level", *decoder_pair(25_000, 12_500), lines)
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
