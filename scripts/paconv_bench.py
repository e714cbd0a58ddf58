"""Times one PAConv layer (csrc/paconv.hip + the dense GEMMs, minkowski/paconv.py), forward + backward, at the layer shapes of the
reference's two PAConv networks -- 32 shapes x 2,048 points, k = 20, M = 8 -- beside the torch composition in the reference's
form on the same GPU (transform every point by the whole bank, gather [n, k, M, O], contract with the scores), in fp32, and
records the peak memory of both.

    python scripts/paconv_bench.py [--out profiles/paconv_kernels.txt] [--batch 32] [--points 2048] [--repeats 7]

  DGCNN variant    (mode "dgcnn"):    Cin -> O = 3 -> 64, 64 -> 64, 64 -> 128, 128 -> 256     (DGCNN_PAConv.py:33-37)
  PointNet variant (mode "pointnet"): Cin -> O = 64 -> 64, 64 -> 64, 64 -> 128                (PointNet_PAConv.py:47-50)

The HIP layer is timed twice: with the incoming-edge lists of the neighbour table given (the models build them once and share
them between their layers) and building them inside the call (a layer on its own).  Every figure is the median of `--repeats`
windows of device-event time after a warm-up of the same shape, with the spread (min .. max) beside it; the sides alternate
window by window.  Peak memory is torch's max_memory_allocated over one forward + backward above what was allocated before.
Needs the GPU: there is no CPU path."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dgcnn_bench import peak_mb, time_windows  # noqa: E402
from nerf_downstream_amd.minkowski import functional as Fn  # noqa: E402
from nerf_downstream_amd.minkowski import graph as G  # noqa: E402
from nerf_downstream_amd.minkowski import paconv as P  # noqa: E402

SHAPES = [("dgcnn", 3, 64), ("dgcnn", 64, 64), ("dgcnn", 64, 128), ("dgcnn", 128, 256),
          ("pointnet", 64, 64), ("pointnet", 64, 64), ("pointnet", 64, 128)]


def torch_layer(x, matrice, s, rows, mode):
    """The reference's order: feat_trans_* (one or two [n, M, O] tensors), then the [n, k, M, O] gather contracted with the scores."""
    n, cin = x.shape
    M = s.shape[2]
    if mode == "dgcnn":
        pts = torch.cat([x, x], 1).mm(matrice).view(n, M, -1)
        ctr = x.mm(matrice[:cin]).view(n, M, -1)
        t = pts[rows] - ctr[:, None]
    else:
        pts = x.mm(matrice).view(n, M, -1)
        t = 2.0 * pts[rows] - pts[:, None]
    return torch.einsum("ijm,ijmo->io", s, t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--matrices", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "paconv_bench needs the GPU"
    B, N, k, M = args.batch, args.points, args.k, args.matrices
    n = B * N
    dev = torch.device("cuda")
    boff = (torch.arange(B + 1, dtype=torch.int32) * N).to(dev)
    g = torch.Generator().manual_seed(0)
    idx = G.knn(torch.rand(n, 3, generator=g).to(dev), boff, k)  # one xyz graph for every layer, as in the models
    rows = idx.long()
    shared = Fn.lazy_index_csr(idx, n)
    shared()
    lines = [f"paconv_bench: {B} samples x {N} points (n = {n}), k = {k}, M = {M}, fp32, forward + backward of one layer, "
             f"{torch.cuda.get_device_name(0)}",
             f"command: python scripts/paconv_bench.py --batch {B} --points {N} --k {k} --matrices {M} --repeats {args.repeats} --out FILE",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time; peak = allocator peak above the inputs",
             ""]
    for mode, cin, O in SHAPES:
        x = torch.randn(n, cin, generator=g).to(dev).requires_grad_(True)
        bank_rows = 2 * cin if mode == "dgcnn" else cin
        matrice = (torch.randn(bank_rows, M * O, generator=g) * (2.0 / (bank_rows * O)) ** 0.5).to(dev).requires_grad_(True)
        s = (torch.softmax(torch.randn(n, k, M, generator=g), 2) + (0.5 if mode == "dgcnn" else 0.0)).to(dev).requires_grad_(True)
        dy = torch.randn(n, O, generator=g).to(dev)
        leaves = [x, matrice, s]

        def hip(csr):
            torch.autograd.grad(P.paconv(x, matrice, s, idx, mode, csr_fn=csr), leaves, dy)

        def ref():
            torch.autograd.grad(torch_layer(x, matrice, s, rows, mode), leaves, dy)

        fns = [lambda: hip(shared), lambda: hip(None), ref]
        with torch.no_grad():
            diff = float((P.paconv(x, matrice, s, idx, mode) - torch_layer(x, matrice, s, rows, mode)).abs().max())
        t = time_windows(fns, args.repeats)
        pk = [peak_mb(f) for f in fns]
        lines.append(f"{mode:8s} {cin:3d} -> {O:3d}  HIP, lists shared {t[0][0]:8.3f} [{t[0][1]:.3f} .. {t[0][2]:.3f}] ms, peak {pk[0]:8.1f} MB"
                     f" | HIP, lists built {t[1][0]:8.3f} [{t[1][1]:.3f} .. {t[1][2]:.3f}] ms, peak {pk[1]:8.1f} MB"
                     f" | torch composition {t[2][0]:8.3f} [{t[2][1]:.3f} .. {t[2][2]:.3f}] ms, peak {pk[2]:8.1f} MB"
                     f" | torch / HIP shared {t[2][0] / t[0][0]:.2f}x, built {t[2][0] / t[1][0]:.2f}x; max |y_hip - y_torch| {diff:.2e}"
                     f" | one transformed tensor n M O 4 = {n * M * O * 4 / 1e6:.1f} MB, gathered n k M O 4 = {n * k * M * O * 4 / 1e6:.1f} MB")
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
