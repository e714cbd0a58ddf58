"""Times the feature-space nearest neighbour between two clouds (csrc/graph.hip mink_knn_cross through
co3d_3d/src/utils/geometry.py find_nn_gpu, k = 1 with distances) beside the torch composition in the reference's form
(geometry.py: chunks of 500 query rows, `pdist` by differences, a row `min`), in fp32 on the same GPU, and records the peak
memory of both.

    python scripts/match_bench.py [--out profiles/match_kernels.txt] [--repeats 5]

  shapes   : n0 = n1 in {5,000, 20,000, 50,000} x C in {3, 32}; and k = 64 with distances at 20,000 x 3 (the radius search of
             get_matching_indices)
  baseline : the chunked composition with the results kept on the device, and with the reference's `.cpu()` of every chunk's
             minimum and index (a host synchronisation per chunk)

Every figure is the median of `--repeats` windows of device-event time (the `.cpu()` variant: host clock around a window that
ends synchronised), each window long enough to run for a few tens of milliseconds, after a warm-up of the same shape; the
three sides alternate window by window (time_windows of scripts/dgcnn_bench.py).  Peak memory is torch's max_memory_allocated
over one call above what was allocated before it.  Needs the GPU: there is no CPU path."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dgcnn_bench import peak_mb, time_windows  # noqa: E402

from nerf_downstream_amd.co3d_3d.src.utils import geometry as GE  # noqa: E402
from nerf_downstream_amd.minkowski import graph as G  # noqa: E402

CHUNK = 500


def torch_find_nn(F0, F1, to_host):
    """The reference's find_nn_gpu(nn_max_n=500, return_distance=True): per chunk the [500, N1, C] differences, their squares
    summed, the row minimum -- and, with `to_host`, its `.cpu()` copies."""
    dists, inds = [], []
    for i in range(0, F0.shape[0], CHUNK):
        d, ind = GE.pdist(F0[i:i + CHUNK], F1, dist_type="SquareL2").min(dim=1)
        dists.append(d.unsqueeze(1).cpu() if to_host else d.unsqueeze(1))
        inds.append(ind.cpu() if to_host else ind)
    return torch.cat(inds), torch.cat(dists)


def torch_topk(F0, F1, k):
    out = []
    for i in range(0, F0.shape[0], CHUNK):
        out.append(GE.pdist(F0[i:i + CHUNK], F1, dist_type="SquareL2").topk(k, dim=1, largest=False).indices)
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 20000, 50000])
    args = ap.parse_args()
    assert torch.cuda.is_available(), "match_bench needs the GPU"
    dev = torch.device("cuda")
    lines = [f"match_bench: find_nn_gpu (mink_knn_cross, k = 1 with distances) vs chunks of {CHUNK} rows of pdist + min, fp32, "
             f"{torch.cuda.get_device_name(0)}",
             f"median [min .. max] ms per call over {args.repeats} windows; peak = allocator peak above the inputs; "
             "agree = share of rows with the same index as the composition", ""]
    g = torch.Generator().manual_seed(0)
    for n in args.sizes:
        for C in (3, 32):
            F0, F1 = torch.randn(n, C, generator=g).to(dev), torch.randn(n, C, generator=g).to(dev)
            fns = [lambda: GE.find_nn_gpu(F0, F1, nn_max_n=CHUNK, return_distance=True), lambda: torch_find_nn(F0, F1, False),
                   lambda: torch_find_nn(F0, F1, True)]
            hip, ref, refh = time_windows(fns, args.repeats)
            agree = float((fns[0]()[0] == fns[1]()[0]).float().mean())
            flops = 2.0 * n * n * C
            lines.append(f"n0 = n1 = {n:6d} C = {C:<2d}  find_nn_gpu {hip[0]:9.3f} [{hip[1]:.3f} .. {hip[2]:.3f}] ms, peak {peak_mb(fns[0]):8.2f} MB"
                         f" | on device {ref[0]:9.3f} [{ref[1]:.3f} .. {ref[2]:.3f}] ms, peak {peak_mb(fns[1]):8.1f} MB"
                         f" | .cpu() per chunk {refh[0]:9.3f} [{refh[1]:.3f} .. {refh[2]:.3f}] ms"
                         f" | {flops / 1e9:.1f} GFLOP of inner products -> {flops / hip[0] / 1e9:.2f} TFLOP/s; agree {agree:.5f}")
    n, C, k = 20000, 3, 64
    F0, F1 = torch.randn(n, C, generator=g).to(dev), torch.randn(n, C, generator=g).to(dev)
    fns = [lambda: G.knn_cross(F0, F1, k, return_distance=True), lambda: torch_topk(F0, F1, k)]
    hip, ref = time_windows(fns, args.repeats)
    lines.append(f"n0 = n1 = {n:6d} C = {C:<2d}  knn_cross k = {k} with distances {hip[0]:9.3f} [{hip[1]:.3f} .. {hip[2]:.3f}] ms, peak "
                 f"{peak_mb(fns[0]):8.2f} MB | chunked pdist + topk on device {ref[0]:9.3f} [{ref[1]:.3f} .. {ref[2]:.3f}] ms, peak "
                 f"{peak_mb(fns[1]):8.1f} MB")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
