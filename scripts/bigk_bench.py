"""Times the 5^3 / 7^3 sparse-convolution kernels (csrc/conv_bigk.hip: mink_kernel_map_cube, mink_conv_bigk_gather_gemm as forward
and as data gradient, mink_conv_bigk_wgrad) at

    stem7   4 scenes x ~30 k voxels, 1 -> 32, kernel size 7        stem5   the same, kernel size 5
    wide5   the bench batch (16 scenes, ~826 k rows), 28 -> 64, kernel size 5
    mid5    the tensor-stride-2 level of that batch (~173 k rows), 64 -> 64, kernel size 5

beside (a) the reference algorithm as torch operations on the same GPU -- per offset index_select -> mm -> index_add_ over the
rulebook (built outside the timed region) -- and (b) the existing 3x3x3 kernels at the same channels and rows, as time per
present (row, offset) pair.

    python scripts/bigk_bench.py [--out profiles/bigk_kernels.txt] [--repeats 3] [--window_ms 40] [--shapes stem7,stem5,wide5,mid5]

Every time is the median [min .. max] of `--repeats` windows of device-event time after a warm-up of the same shape, the timed
functions alternating window by window; outputs are torch allocations inside the window, as in training.  Peak memory is the
allocator's high-water mark over one call, above what the operands hold.  Needs the GPU."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench import make_batches  # noqa: E402
from dgcnn_bench import peak_mb, time_windows  # noqa: E402
from nerf_downstream_amd import _lib  # noqa: E402
from nerf_downstream_amd import minkowski as ME  # noqa: E402
from nerf_downstream_amd.minkowski import functional as Fn  # noqa: E402

SHAPES = {  # name: (scenes, grid, tensor stride of the level, cin, cout, kernel size)
    "stem7": (4, 96, 1, 1, 32, 7),
    "stem5": (4, 96, 1, 1, 32, 5),
    "wide5": (16, 128, 1, 28, 64, 5),
    "mid5": (16, 128, 2, 64, 64, 5),
}


def fmt(t):
    return f"{t[0]:9.4f} [{t[1]:.4f} .. {t[2]:.4f}]"


def rulebook(nbr):
    """[(k, in rows, out rows)] of the offsets that have pairs (int64 index tensors, as index_select / index_add_ take them)."""
    tt = nbr.t()
    kk, oo = (tt >= 0).nonzero(as_tuple=True)
    ins = tt[kk, oo].long()
    c = [0] + torch.bincount(kk, minlength=nbr.shape[1]).cumsum(0).tolist()
    return [(k, ins[c[k]:c[k + 1]], oo[c[k]:c[k + 1]]) for k in range(nbr.shape[1]) if c[k + 1] > c[k]]


def shape_lines(args, dev, name):
    scenes, grid, ts, cin, cout, ks = SHAPES[name]
    K = ks ** 3
    coords = make_batches(1, scenes, 0, 51, grid, 28)[0]["coordinates"].to(dev)
    m = ME.TensorField(coordinates=coords, features=torch.zeros(coords.shape[0], 1, device=dev)).coordinate_manager
    key = ME.CoordinateMapKey(1)
    while key.ts < ts:
        key = m.stride(key, 2)
    n = m.size(key)

    nbr, nbr3 = m.kernel_table(key, key, ks, 1)[0], m.kernel_table(key, key, 3, 1)[0]
    lev, L = m.levels[ts], _lib.lib()
    tab = torch.empty_like(nbr)  # (the timed builds write here: a manager would take a fresh 100+ MB from its arena every time)
    tws = torch.empty(int(L.mink_kernel_map_cube_workspace_bytes(n)), dtype=torch.uint8, device=dev)

    def table_cube():
        _lib.check(L.mink_kernel_map_cube(lev.coords.data_ptr(), n, lev.coords.data_ptr(), n, ks, ts, tab.data_ptr(), None, tws.data_ptr(),
                                          tws.numel(), torch.cuda.current_stream().cuda_stream))

    def table_3():
        m.tables.pop((ts, ts, 3, 1), None)
        return m.kernel_table(key, key, 3, 1)[0]

    t_tab, t_tab3 = time_windows([table_cube, table_3], args.repeats, args.window_ms)
    assert torch.equal(tab, nbr)
    pairs, pairs3 = int((nbr >= 0).sum()), int((nbr3 >= 0).sum())
    g = torch.Generator().manual_seed(ks + cin)
    x = torch.randn(n, cin, generator=g).to(dev)
    dy = torch.randn(n, cout, generator=g).to(dev)
    w = (torch.randn(K, cin, cout, generator=g) * (cin * K) ** -0.5).to(dev)
    c3 = cin + (-cin) % 4  # (the 3x3x3 forward takes channel counts that are multiples of 4: the module pads them)
    x3, w3 = torch.randn(n, c3, generator=g).to(dev), (torch.randn(27, c3, cout, generator=g) * (c3 * 27) ** -0.5).to(dev)
    book = rulebook(nbr)

    def fwd():
        return Fn.gather_gemm(x, w, nbr, cout)

    def dgrad():
        return Fn.gather_gemm(dy, w, nbr, cin, w_transposed=True, flip_k=True)

    def wgrad():
        return Fn.conv_wgrad(x, dy, nbr, (K, cin, cout))

    def t_fwd():
        y = torch.zeros(n, cout, device=dev)
        for k, i, o in book:
            y.index_add_(0, o, x.index_select(0, i) @ w[k])
        return y

    def t_dgrad():
        dx = torch.zeros(n, cin, device=dev)
        for k, i, o in book:
            dx.index_add_(0, i, dy.index_select(0, o) @ w[k].t())
        return dx

    def t_wgrad():
        dw = torch.zeros(K, cin, cout, device=dev)
        for k, i, o in book:
            dw[k] = x.index_select(0, i).t() @ dy.index_select(0, o)
        return dw

    def f3():
        return Fn.gather_gemm(x3, w3, nbr3, cout)

    def d3():
        return Fn.gather_gemm(dy, w3, nbr3, c3, w_transposed=True, flip_k=True)

    def w3g():
        return Fn.conv_wgrad(x3, dy, nbr3, (27, c3, cout))

    # the kernels and the torch composition agree (sums in other orders)
    scale = lambda a, b: float((a - b).abs().max() / b.abs().max().clamp_min(1e-30))  # noqa: E731
    agree = (scale(fwd(), t_fwd()), scale(dgrad(), t_dgrad()), scale(wgrad(), t_wgrad()))
    assert max(agree) < 1e-4, agree
    fns = [fwd, dgrad, wgrad, t_fwd, t_dgrad, t_wgrad, f3, d3, w3g]
    T = time_windows(fns, args.repeats, args.window_ms)
    mem = [peak_mb(f) for f in (fwd, dgrad, wgrad, t_fwd, t_dgrad, t_wgrad)]
    flop = 2.0 * pairs * cin * cout
    lines = [f"{name}: {scenes} scenes, tensor stride {ts}, {n} rows, {cin} -> {cout}, kernel size {ks} (K = {K}); "
             f"{pairs / n:.1f} present pairs per row ({100.0 * pairs / (n * K):.0f} % of K), table {4e-6 * n * K:.0f} MB; "
             f"3x3x3 at the same rows: {pairs3 / n:.1f} pairs per row",
             f"  table build (fill, insert, probe) ms {fmt(t_tab)}    (3x3x3 through the block index, from the manager: {fmt(t_tab3)})",
             "  pass        this kernel: ms, peak MB, TFLOP/s, ns per pair | torch per-offset: ms, peak MB | 3x3x3 kernel (" + str(c3) + f" -> {cout}): ms, ns per pair | torch / this"]
    for i, p in enumerate(("forward", "data grad", "weight grad")):
        a, b, c = T[i], T[3 + i], T[6 + i]
        lines.append(f"  {p:11s} {fmt(a)} {mem[i]:8.1f} {flop / a[0] * 1e-9:7.2f} {a[0] * 1e6 / pairs:7.3f} | {fmt(b)} {mem[3 + i]:8.1f} | "
                     f"{fmt(c)} {c[0] * 1e6 / pairs3:7.3f} | {b[0] / a[0]:6.2f}x")
    lines.append(f"  largest relative difference to the torch composition: forward {agree[0]:.1e}, data gradient {agree[1]:.1e}, weight gradient {agree[2]:.1e}")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bigk_kernels.txt"))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--window_ms", type=float, default=40.0)
    ap.add_argument("--shapes", default=",".join(SHAPES))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bigk_bench.py needs the MI355X"
    dev = torch.device("cuda", 0)
    lines = [f"scripts/bigk_bench.py on {torch.cuda.get_device_name(0)}: median [min .. max] of {args.repeats} windows of >= {args.window_ms:.0f} ms "
             "(or one call), device events; fp32 in every pass", ""]
    for name in args.shapes.split(","):
        lines += shape_lines(args, dev, name) + [""]
        print("\n".join(lines[-7:]), flush=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines))


if __name__ == "__main__":
    main()
