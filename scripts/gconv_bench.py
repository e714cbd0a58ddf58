"""Times the grouped-convolution kernels (csrc/gconv.hip: mink_gconv_fwd as forward and as data gradient, mink_gconv_wgrad) at
the grouped 3x3 layers of resnext50_32x4d and resnext101_32x8d at B = 32, 224^2 -- maps of 56, 28, 14 and 7 squared, each in its
stride-1 form (m -> m) and its stride-2 form (2 m -> m; 112 -> 56 is in neither network and is there for the row count) -- beside

    (a) the same layer as block-diagonal weights [K, G c, G c] through the dense gather-GEMM kernels (mink_conv_gather_gemm /
        mink_conv_wgrad, fp32 math), which do G times the multiply-adds: the grouped kernel has to be faster at every shape and pass;
    (b) torch on the same GPU: F.conv2d(groups=32) / torch.nn.grad.conv2d_input / conv2d_weight in fp32 with TF32 off, in the
        contiguous and the channels_last layout (the faster of the two is quoted).

    python scripts/gconv_bench.py [--out profiles/gconv_kernels.txt] [--repeats 5] [--window_ms 30]

Every time is the median [min .. max] of `--repeats` windows of device-event time after a warm-up of the same shape, the timed
functions alternating window by window; outputs of the library calls are torch allocations inside the window, as in training.
Needs the GPU."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dgcnn_bench import time_windows  # noqa: E402
from nerf_downstream_amd.co3d_2d.src.model import dense  # noqa: E402
from nerf_downstream_amd.minkowski import functional as Fn  # noqa: E402

B, G = 32, 32
# (network, group width) per output map
LAYERS = {56: (("resnext50_32x4d", 4), ("resnext101_32x8d", 8)), 28: (("resnext50_32x4d", 8), ("resnext101_32x8d", 16)),
          14: (("resnext50_32x4d", 16), ("resnext101_32x8d", 32)), 7: (("resnext50_32x4d", 32), ("resnext101_32x8d", 64))}


def fmt(t):
    return f"{t[0]:8.4f} [{t[1]:.4f} .. {t[2]:.4f}]"


def layer_lines(args, dev, m, cg, stride, names):
    C, hin = G * cg, m * stride
    grid = dense.Grid(B, hin, hin)
    og, nbr, nbr_t, perm = dense._conv_tables(grid, 3, stride, 1, dev)
    g = torch.Generator().manual_seed(m * 100 + cg)
    x = torch.randn(grid.rows, C, generator=g).to(dev)
    gy = torch.randn(og.rows, C, generator=g).to(dev)
    weight = (torch.randn(C, cg, 3, 3, generator=g) / (3.0 * cg ** 0.5)).to(dev)  # torch's layout
    w = weight.view(G, cg, cg, 3, 3).permute(3, 4, 0, 2, 1).reshape(9, G, cg, cg).contiguous()
    wd = torch.zeros(9, C, C, device=dev)  # block diagonal: [k][g c][g o]
    for i in range(G):
        wd[:, i * cg:(i + 1) * cg, i * cg:(i + 1) * cg] = w[:, i]
    same = stride == 1

    def g_fwd():
        return Fn.gconv(x, w, nbr, G, cg, cg)

    def g_dgrad():
        return Fn.gconv(gy, w, nbr, G, cg, cg, True, True) if same else Fn.gconv(gy, w, nbr_t, G, cg, cg, True)

    def g_wgrad():
        return Fn.gconv_wgrad(x, gy, nbr, G, cg, cg)

    def d_fwd():
        return Fn.gather_gemm(x, wd, nbr, C)

    def d_dgrad():
        if same:
            return Fn.gather_gemm(gy, wd, nbr, C, w_transposed=True, flip_k=True)
        return Fn.gather_gemm(gy, wd, nbr_t, C, w_transposed=True, row_perm=perm)

    def d_wgrad():
        return Fn.conv_wgrad(x, gy, nbr, wd.shape)

    # the three implementations agree (the dense form and torch sum in other orders)
    xi = x.view(B, hin, hin, C).permute(0, 3, 1, 2)
    gi = gy.view(B, m, m, C).permute(0, 3, 1, 2)
    rows = lambda t: t.permute(0, 2, 3, 1).reshape(-1, C)  # noqa: E731
    with torch.no_grad():
        yt = F.conv2d(xi, weight, stride=stride, padding=1, groups=G)
        dxt = torch.nn.grad.conv2d_input(xi.shape, weight, gi, stride=stride, padding=1, groups=G)
        dwt = torch.nn.grad.conv2d_weight(xi, weight.shape, gi, stride=stride, padding=1, groups=G)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())  # noqa: E731
    dw_t = dwt.view(G, cg, cg, 3, 3).permute(3, 4, 0, 2, 1).reshape(9, G, cg, cg)
    agree = (rel(g_fwd(), rows(yt)), rel(g_dgrad(), rows(dxt)), rel(g_wgrad(), dw_t), rel(d_fwd(), rows(yt)))
    del yt, dxt, dwt

    fns = [g_fwd, g_dgrad, g_wgrad, d_fwd, d_dgrad, d_wgrad]
    for fmt_ in (torch.contiguous_format, torch.channels_last):
        xc, gc, wc = (t.contiguous(memory_format=fmt_) for t in (xi, gi, weight))

        def t_fwd(xc=xc, wc=wc):
            with torch.no_grad():
                return F.conv2d(xc, wc, stride=stride, padding=1, groups=G)

        def t_dgrad(xc=xc, gc=gc, wc=wc):
            return torch.nn.grad.conv2d_input(xc.shape, wc, gc, stride=stride, padding=1, groups=G)

        def t_wgrad(xc=xc, gc=gc, wc=wc):
            return torch.nn.grad.conv2d_weight(xc, wc.shape, gc, stride=stride, padding=1, groups=G)

        fns += [t_fwd, t_dgrad, t_wgrad]
    t = time_windows(fns, args.repeats, target_ms=args.window_ms)
    macs = og.rows * C * 9 * cg
    lines = [f"{m} x {m} map, stride {stride} ({hin} -> {m}), 32 groups of {cg}: {C} channels, {grid.rows} -> {og.rows} rows, "
             f"{2 * macs / 1e9:.2f} GFLOP per pass ({', '.join(names)})"]
    worst = 1e9
    for i, name in enumerate(("forward", "data gradient", "weight gradient")):
        tt = min(t[6 + i], t[9 + i])
        lay = "contiguous" if t[6 + i][0] <= t[9 + i][0] else "channels_last"
        lines.append(f"  {name:15s} grouped {fmt(t[i])} ms {2 * macs / t[i][0] / 1e9:6.2f} TFLOP/s | block-diagonal dense {fmt(t[3 + i])} ms "
                     f"= {t[3 + i][0] / t[i][0]:6.2f}x | torch {fmt(tt)} ms ({lay}) = {tt[0] / t[i][0]:5.2f}x")
        worst = min(worst, t[3 + i][0] / t[i][0])
    lines.append(f"  max |difference| / max |value|: grouped against torch {agree[0]:.1e} {agree[1]:.1e} {agree[2]:.1e}, dense forward against torch {agree[3]:.1e}")
    lines.append("")
    print("\n".join(lines), flush=True)
    del x, gy, wd, xi, gi
    torch.cuda.empty_cache()
    return lines, worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=30.0)
    ap.add_argument("--append", default=None, help="a text file whose lines are appended (scripts/bench_2d.py --model runs)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "gconv_bench needs the GPU"
    dev = torch.device("cuda", 0)
    old = torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32
    torch.backends.cudnn.allow_tf32 = torch.backends.cuda.matmul.allow_tf32 = False
    Fn.set_conv_math("fp32")
    lines = [f"gconv_bench: fp32, {torch.cuda.get_device_name(0)}",
             f"command: python scripts/gconv_bench.py --repeats {args.repeats} --window_ms {args.window_ms} --out FILE",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time; random normal data; B = {B}",
             "x = block-diagonal dense (or torch) time / grouped time: above 1 the grouped kernel is faster", ""]
    print("\n".join(lines), flush=True)
    worst = []
    try:
        for m, nets in LAYERS.items():
            for cg in sorted({c for _, c in nets}):
                names = [n for n, c in nets if c == cg]
                for stride in (1, 2):
                    ls, wv = layer_lines(args, dev, m, cg, stride, names)
                    lines += ls
                    worst.append((wv, m, cg, stride))
    finally:
        torch.backends.cudnn.allow_tf32, torch.backends.cuda.matmul.allow_tf32 = old
    wv, m, cg, stride = min(worst)
    lines += [f"smallest block-diagonal dense / grouped ratio over all shapes and passes: {wv:.2f}x ({m} x {m}, groups of {cg}, stride {stride})", ""]
    print(lines[-2], flush=True)
    if args.append and os.path.exists(args.append):
        with open(args.append) as f:
            lines += [ln.rstrip() for ln in f] + [""]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
