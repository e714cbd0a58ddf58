"""Times the attention kernels (csrc/attn.hip: mink_attn_fwd / mink_attn_bwd) beside the explicit torch composition
(softmax(q k^T) v on [B, H, N, D] views, its backward through autograd) and torch.nn.functional.scaled_dot_product_attention on
the same GPU and the same random data, and one training step of ViTBased("vit_small_patch16_224").

    python scripts/attn_bench.py [--out profiles/attn_kernels.txt] [--repeats 5] [--errors FILE]

Shapes: B = 32, N = 197 (a 224^2 image), D = 64, H = 6 / 12 / 16 (vit_small / base / large).  Every time is the median
[min .. max] of `--repeats` windows of device-event time after a warm-up of the same shape, the timed functions alternating
window by window; the kernels' outputs are allocated once, outside the windows.  TFLOP/s = the algorithm's 4 B H N^2 D
(forward) or 10 B H N^2 D (backward, five products; the kernels run seven) over the median, not what the kernels execute.
Peak MB = torch's peak allocation above what was live before one forward + backward.  `--errors FILE`: lines (the model-level
errors test_gpu_vit.py prints) copied to the end of the output.  Nothing is gated on these numbers.  Needs the GPU."""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dgcnn_bench import peak_mb, time_windows  # noqa: E402
from nerf_downstream_amd._lib import check, lib  # noqa: E402
from nerf_downstream_amd.minkowski import attention  # noqa: E402

B, N, D = 32, 197, 64
HEADS = (6, 12, 16)


def fmt(t):
    return f"{t[0]:8.4f} [{t[1]:.4f} .. {t[2]:.4f}]"


def operator_lines(args, dev):
    L, lines = lib(), []
    g = torch.Generator().manual_seed(0)
    st = torch.cuda.current_stream().cuda_stream
    scale = D ** -0.5
    for H in HEADS:
        W = H * D
        qkv = torch.randn(B * N, 3 * W, generator=g).to(dev)
        dout = torch.randn(B * N, W, generator=g).to(dev)
        out, dqkv = torch.empty(B * N, W, device=dev), torch.empty(B * N, 3 * W, device=dev)
        lse = torch.empty(B, H, N, device=dev)
        ws = torch.empty(L.mink_attn_bwd_workspace_bytes(B, N, H, D), dtype=torch.uint8, device=dev)
        qg = qkv.clone().requires_grad_(True)

        def fwd():
            check(L.mink_attn_fwd(qkv.data_ptr(), 3 * W, B, N, H, D, scale, out.data_ptr(), W, lse.data_ptr(), st))

        def bwd():
            check(L.mink_attn_bwd(qkv.data_ptr(), 3 * W, out.data_ptr(), W, lse.data_ptr(), dout.data_ptr(), W, B, N, H, D, scale,
                                  dqkv.data_ptr(), 3 * W, ws.data_ptr(), ws.numel(), st))

        def function():
            qg.grad = None
            attention(qg, B, N, H).backward(dout)

        def heads(x):
            return x.reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)

        def torch_fwd(x=qkv):
            q, k, v = heads(x)
            return (torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1) @ v).transpose(1, 2).reshape(B * N, W)

        def sdpa_fwd(x=qkv):
            q, k, v = heads(x)
            return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, W)

        def torch_fwd_bwd():
            qg.grad = None
            torch_fwd(qg).backward(dout)

        def sdpa_fwd_bwd():
            qg.grad = None
            sdpa_fwd(qg).backward(dout)

        def torch_fwd_only():
            with torch.no_grad():
                torch_fwd()

        def sdpa_fwd_only():
            with torch.no_grad():
                sdpa_fwd()

        def both():
            fwd(), bwd()

        both()
        with torch.no_grad():
            d_out = float((torch_fwd() - out).abs().max())
        torch_fwd_bwd()
        d_grad = float((qg.grad - dqkv).abs().max() / qg.grad.abs().max())
        t = time_windows([fwd, bwd, both, torch_fwd_only, torch_fwd_bwd, sdpa_fwd_only, sdpa_fwd_bwd], args.repeats, target_ms=args.window_ms)
        mem = [peak_mb(function), peak_mb(torch_fwd_bwd), peak_mb(sdpa_fwd_bwd)]
        ff, bf = 4.0 * B * H * N * N * D, 10.0 * B * H * N * N * D
        lines += [f"H = {H} (B = {B}, N = {N}, D = {D}; qkv is {4 * B * N * 3 * W / 1e6:.1f} MB, one [B, H, N, N] matrix would be {4 * B * H * N * N / 1e6:.1f} MB)",
                  f"  mink_attn_fwd                    {fmt(t[0])} ms   {ff / t[0][0] / 1e9:6.2f} TFLOP/s",
                  f"  mink_attn_bwd (3 launches)       {fmt(t[1])} ms   {bf / t[1][0] / 1e9:6.2f} TFLOP/s",
                  f"  fwd + bwd                        {fmt(t[2])} ms   peak {mem[0]:7.1f} MB (through AttentionFunction)",
                  f"  torch matmul-softmax-matmul fwd  {fmt(t[3])} ms   torch / kernel {t[3][0] / t[0][0]:5.2f}x",
                  f"  torch fwd + autograd bwd         {fmt(t[4])} ms   torch / kernels {t[4][0] / t[2][0]:5.2f}x   peak {mem[1]:7.1f} MB",
                  f"  F.scaled_dot_product_attention   {fmt(t[5])} ms   sdpa / kernel {t[5][0] / t[0][0]:5.2f}x",
                  f"  sdpa fwd + autograd bwd          {fmt(t[6])} ms   sdpa / kernels {t[6][0] / t[2][0]:5.2f}x   peak {mem[2]:7.1f} MB",
                  f"  max |out - torch| {d_out:.1e}, max |dqkv - torch| / max |dqkv| {d_grad:.1e}", ""]
        print("\n".join(lines[-10:]), flush=True)
        del qkv, dout, out, dqkv, lse, ws, qg
        torch.cuda.empty_cache()
    return lines


def step_lines(args, dev):
    """One training step (forward, cross entropy, backward, SGD) of ViT-Small / 16 on a batch of 32 random 224^2 images."""
    from nerf_downstream_amd.co3d_2d.src.model.models import ViTBased

    torch.manual_seed(0)
    net = ViTBased("vit_small_patch16_224").to(dev).train()
    opt = torch.optim.SGD(net.parameters(), lr=0.003, momentum=0.9)
    images, labels = torch.randn(B, 3, 224, 224, device=dev), torch.randint(0, 51, (B,), device=dev)

    def step():
        opt.zero_grad(set_to_none=True)
        F.cross_entropy(net(images), labels).backward()
        opt.step()

    for _ in range(3):
        step()
    t = time_windows([step], args.repeats, target_ms=8 * args.window_ms)
    mem = peak_mb(step)
    return [f"one training step of ViTBased('vit_small_patch16_224'), B = {B}, 224^2, fp32 (forward, cross entropy, backward, torch SGD):",
            f"  {fmt(t[0])} ms   {B / t[0][0] * 1e3:7.1f} images/s   peak {mem:7.1f} MB above the parameters and optimizer state", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=40.0)
    ap.add_argument("--errors", default=None, help="a text file whose lines are appended (the errors test_gpu_vit.py prints)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn_bench needs the GPU"
    dev = torch.device("cuda")
    lines = [f"attn_bench: fp32, {torch.cuda.get_device_name(0)}",
             f"command: python scripts/attn_bench.py --repeats {args.repeats} --window_ms {args.window_ms} --out FILE",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time; random normal data", ""]
    print("\n".join(lines), flush=True)
    lines += operator_lines(args, dev)
    tail = step_lines(args, dev)
    print("\n".join(tail), flush=True)
    lines += tail
    if args.errors and os.path.exists(args.errors):
        with open(args.errors) as f:
            lines += ["model-level errors against float64 (printed by tests/test_gpu_vit.py on the same GPU):"] + \
                     ["  " + ln.rstrip() for ln in f if ln.strip()] + [""]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
