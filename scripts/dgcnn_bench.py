"""Times the dynamic graph kernels (csrc/graph.hip) at the reference's DGCNN shape -- 32 shapes x 2,048 points, k = 20 -- beside
the torch composition the reference uses, in fp32 on the same GPU, and records the peak memory of both.

    python scripts/dgcnn_bench.py [--out profiles/dgcnn_kernels.txt] [--batch 32] [--points 2048] [--repeats 7]

  kNN        : mink_knn at C = 3 / 64 / 128      vs  -2 x^T x + norms, topk                         (dgcnn.py:8-13)
  edge layer : P / Q GEMMs + mink_edge_stats + mink_edge_fwd, and mink_edge_bwd + the gradient GEMMs, 64 -> 128 channels
               vs  gather, cat(x_j - x_i, x_i), 1x1 Conv2d, BatchNorm2d, LeakyReLU(0.2), max over k     (dgcnn.py:16-38,81-85)

Every figure is the median of `--repeats` windows of device-event time, each window long enough to run for a few tens of
milliseconds, after a warm-up of the same shape; the spread (min .. max of the windows) is printed beside it.  The two sides
alternate window by window.  Peak memory is torch's max_memory_allocated over one call (forward, or forward + backward) above
what was allocated before it.  Needs the GPU: there is no CPU path."""
import argparse
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from nerf_downstream_amd.minkowski import graph as G  # noqa: E402


def time_windows(fns, repeats, target_ms=40.0):
    """Median / min / max ms per call of every fn, the fns alternating window by window."""
    iters = []
    for fn in fns:  # warm-up, and the number of calls that fills a window
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        iters.append(max(1, min(200, int(target_ms / max(a.elapsed_time(b), 1e-3)))))
    out = [[] for _ in fns]
    for _ in range(repeats):
        for i, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters[i]):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[i].append(a.elapsed_time(b) / iters[i])
    return [(statistics.median(v), min(v), max(v)) for v in out]


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 1e6


def torch_knn(pts, k):
    """Dense composition: one batched GEMM for the Gram matrix, the squared norms added on both sides, topk.  pts [B, N, C]."""
    gram = torch.bmm(pts, pts.transpose(1, 2))
    sq = (pts * pts).sum(-1)
    dist = sq[:, :, None] - 2.0 * gram + sq[:, None, :]
    return dist.topk(k, dim=-1, largest=False).indices


def torch_edge_features(pts, nbr):
    """pts [B, N, C], nbr [B, N, k] (rows of the same sample) -> [B, 2 C, N, k]: the gathered neighbours minus the centre,
    concatenated with the centre, in the channels-first layout a 1x1 Conv2d reads."""
    B, N, C = pts.shape
    k = nbr.shape[-1]
    rows = (nbr + N * torch.arange(B, device=pts.device)[:, None, None]).reshape(-1)
    gathered = pts.reshape(B * N, C).index_select(0, rows).reshape(B, N, k, C)
    centre = pts[:, :, None, :].expand(B, N, k, C)
    return torch.cat([gathered - centre, centre], dim=-1).permute(0, 3, 1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--points", type=int, default=2048)
    ap.add_argument("--k", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dgcnn_bench needs the GPU"
    B, N, k = args.batch, args.points, args.k
    n = B * N
    dev = torch.device("cuda")
    boff = (torch.arange(B + 1, dtype=torch.int32) * N).to(dev)
    lines = [f"dgcnn_bench: {B} samples x {N} points (n = {n}), k = {k}, fp32, {torch.cuda.get_device_name(0)}",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time; peak = allocator peak above the inputs",
             ""]
    g = torch.Generator().manual_seed(0)
    # ---- kNN
    for C in (3, 64, 128):
        x = torch.randn(n, C, generator=g).to(dev)
        xd = x.view(B, N, C)
        (hip, ref) = time_windows([lambda: G.knn(x, boff, k), lambda: torch_knn(xd, k)], args.repeats)
        same = float((G.knn(x, boff, k).view(B, N, k).long().sort(-1).values
                      == (torch_knn(xd, k) + (torch.arange(B, device=dev) * N).view(-1, 1, 1)).sort(-1).values).float().mean())
        flops = 2.0 * B * N * N * C
        lines.append(f"knn C={C:<3d}  mink_knn {hip[0]:8.3f} [{hip[1]:.3f} .. {hip[2]:.3f}] ms, peak {peak_mb(lambda: G.knn(x, boff, k)):7.1f} MB"
                     f" | torch matmul+topk {ref[0]:8.3f} [{ref[1]:.3f} .. {ref[2]:.3f}] ms, peak {peak_mb(lambda: torch_knn(xd, k)):7.1f} MB"
                     f" | inner products {flops / 1e9:.1f} GFLOP -> {flops / hip[0] / 1e9:.2f} TFLOP/s in mink_knn; {same:.5f} of the slots in both sets")
    # ---- one edge layer, 64 -> 128
    cin, cout = 64, 128
    x = torch.randn(n, cin, generator=g).to(dev)
    idx = G.knn(x, boff, k)
    conv = torch.nn.Conv2d(2 * cin, cout, 1, bias=False).to(dev)
    bn = torch.nn.BatchNorm2d(cout).to(dev)
    dy = torch.randn(n, cout, generator=g).to(dev)
    xd = x.view(B, N, cin)
    idxd = (idx.view(B, N, k).long() - (torch.arange(B, device=dev) * N).view(-1, 1, 1))
    dyd = dy.view(B, N, cout).transpose(2, 1).contiguous()

    def hip_layer(backward):
        xl = x.detach().requires_grad_(backward)
        y, _ = G.EdgeConvFunction.apply(xl, conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, idx, True, 0.1, 1e-5)
        if backward:
            torch.autograd.grad(y, [xl, conv.weight, bn.weight, bn.bias], dy)

    def torch_layer(backward):
        xl = xd.detach().requires_grad_(backward)
        with torch.set_grad_enabled(backward):
            f = torch.nn.functional.leaky_relu(bn(conv(torch_edge_features(xl, idxd))), 0.2)
            y = f.max(dim=-1)[0]
        if backward:
            torch.autograd.grad(y, [xl, conv.weight, bn.weight, bn.bias], dyd)

    for name, bw in (("forward", False), ("forward + backward", True)):
        (hip, ref) = time_windows([lambda: hip_layer(bw), lambda: torch_layer(bw)], args.repeats)
        lines.append(f"edge layer {cin} -> {cout}, {name:18s}  HIP {hip[0]:8.3f} [{hip[1]:.3f} .. {hip[2]:.3f}] ms, peak {peak_mb(lambda: hip_layer(bw)):8.1f} MB"
                     f" | torch composition {ref[0]:8.3f} [{ref[1]:.3f} .. {ref[2]:.3f}] ms, peak {peak_mb(lambda: torch_layer(bw)):8.1f} MB")
    lines.append(f"(one edge tensor n k Cout 4 = {n * k * cout * 4 / 1e6:.1f} MB)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
