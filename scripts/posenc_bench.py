"""Times the positional-encoding kernels (csrc/posenc.hip: mink_posenc_fwd / mink_posenc_bwd) beside the torch composition in the
reference's form (sparse matrix product, add, sin; its backward through autograd) on the same GPU, and one training step of
EncodedRes16UNet beside Res16UNet on the same scenes.

    python scripts/posenc_bench.py [--out profiles/posenc_kernels.txt] [--repeats 5]

Shapes: C = 28, L = 4, n = 826 k (the rows of the B = 16 plenoxel batch) and C = 3, L = 4, n = 2 M (a point cloud's colours).
Every figure is the median [min .. max] of `--repeats` windows of device-event time after a warm-up of the same shape, the
timed functions alternating window by window; outputs are allocated once, outside the windows.  GB/s = the bytes the pass must
move (forward: x in, y out; backward: x and dy in, dx out) over the median.  Needs the GPU: there is no CPU path."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dgcnn_bench import time_windows  # noqa: E402
from nerf_downstream_amd import minkowski as ME  # noqa: E402
from nerf_downstream_amd._lib import check, lib  # noqa: E402
from nerf_downstream_amd.co3d_3d.src.models import get_model  # noqa: E402

SHAPES = ((28, 4, 826_000), (3, 4, 2_000_000))


def fmt(t):
    return f"{t[0]:8.4f} [{t[1]:.4f} .. {t[2]:.4f}]"


def operator_lines(args, dev):
    lines = []
    g = torch.Generator().manual_seed(0)
    for C, L, n in SHAPES:
        mod = ME.MinkowskiPositionalEncoding(C, num_encoding_functions=L).to(dev)
        Q = mod.out_channels
        x = (1.5 * torch.randn(n, C, generator=g)).to(dev)
        dy = torch.randn(n, Q, generator=g).to(dev)
        y, dx = torch.empty(n, Q, device=dev), torch.empty(n, C, device=dev)
        f, p = mod.frequencies.data_ptr(), mod.offset.data_ptr()
        st = torch.cuda.current_stream().cuda_stream
        mat = torch.sparse_coo_tensor(mod.coo.detach(), mod.frequencies.detach(), (C, Q), device=dev).t().coalesce()  # the reference's `mat`
        offset = mod.offset.detach()
        xg = x.clone().requires_grad_(True)

        def fwd():
            check(lib().mink_posenc_fwd(x.data_ptr(), n, C, C, f, p, L, 0, 0, y.data_ptr(), Q, st))

        def bwd():
            check(lib().mink_posenc_bwd(dy.data_ptr(), Q, x.data_ptr(), n, C, C, f, p, L, 0, 0, dx.data_ptr(), C, st))

        def torch_fwd():
            with torch.no_grad():
                return torch.sin((mat @ x.T).T + offset)

        def torch_fwd_bwd():
            xg.grad = None
            torch.sin((mat @ xg.T).T + offset).backward(dy)

        def both():
            fwd(), bwd()

        fwd(), bwd(), torch_fwd_bwd()
        diff = float((torch_fwd() - y).abs().max())
        gdiff = float((xg.grad - dx).abs().max() / xg.grad.abs().max())
        t = time_windows([fwd, bwd, both, torch_fwd, torch_fwd_bwd], args.repeats, target_ms=args.window_ms)
        fb, bb = 4 * n * (C + Q), 4 * n * (2 * C + Q)
        lines += [f"C = {C}, L = {L}, n = {n} ({Q} columns; y is {4 * n * Q / 1e6:.0f} MB)",
                  f"  mink_posenc_fwd              {fmt(t[0])} ms   {fb / t[0][0] / 1e6:7.1f} GB/s",
                  f"  mink_posenc_bwd              {fmt(t[1])} ms   {bb / t[1][0] / 1e6:7.1f} GB/s",
                  f"  fwd + bwd                    {fmt(t[2])} ms",
                  f"  torch spmm + add + sin       {fmt(t[3])} ms   {fb / t[3][0] / 1e6:7.1f} GB/s of the same bytes   torch / kernel {t[3][0] / t[0][0]:5.2f}x",
                  f"  torch fwd + autograd bwd     {fmt(t[4])} ms   torch / kernels {t[4][0] / t[2][0]:5.2f}x",
                  f"  max |y - torch| {diff:.1e}, max |dx - torch| / max |dx| {gdiff:.1e}", ""]
        print("\n".join(lines[-8:]), flush=True)
        del x, dy, y, dx, xg, mat
        torch.cuda.empty_cache()
    return lines


def step_lines(args, dev):
    """One training step (forward, cross entropy, backward, SGD) of both networks on the same four synthetic 128^3 scenes."""
    from nerf_downstream_amd.co3d_3d.src.data.synthetic import SparseVoxelDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink

    ds = SparseVoxelDataset(phase="train", num_samples=64, num_classes=20, grid=128, features=["density", "sh"])
    batch = collate_mink([ds[i] for i in range(4)])
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()}
    n = batch["coordinates"].shape[0]
    labels = torch.randint(0, 20, (n,), generator=torch.Generator().manual_seed(1)).to(dev)
    fns = []
    for name in ("Res16UNet", "EncodedRes16UNet"):
        torch.manual_seed(0)
        net = get_model(name, batch["features"].shape[1], 20).to(dev).train()
        opt = torch.optim.SGD([p for p in net.parameters() if p.requires_grad], lr=0.01, momentum=0.9)

        def step(net=net, opt=opt):
            opt.zero_grad(set_to_none=True)
            loss = F.cross_entropy(net(net.process_input({"coordinates": batch["coordinates"], "features": batch["features"]})), labels)
            loss.backward()
            opt.step()

        for _ in range(3):
            step()
        fns.append(step)
    t = time_windows(fns, args.repeats, target_ms=8 * args.window_ms)
    return [f"one training step, 4 synthetic 128^3 scenes, {n} rows, {batch['features'].shape[1]} channels, 20 classes (forward, cross entropy, "
            "backward, torch SGD; maps rebuilt every step):",
            f"  Res16UNet                    {fmt(t[0])} ms",
            f"  EncodedRes16UNet             {fmt(t[1])} ms   encoded / plain {t[1][0] / t[0][0]:5.2f}x", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=20.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "posenc_bench needs the GPU"
    dev = torch.device("cuda")
    lines = [f"posenc_bench: fp32, {torch.cuda.get_device_name(0)}",
             f"command: python scripts/posenc_bench.py --repeats {args.repeats} --window_ms {args.window_ms} --out FILE",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time", ""]
    print("\n".join(lines), flush=True)
    lines += operator_lines(args, dev)
    tail = step_lines(args, dev)
    print("\n".join(tail), flush=True)
    lines += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
