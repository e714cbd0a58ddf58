"""Times the bf16-row attention kernels (csrc/attn16.hip: mink_attn_fwd_b16 / mink_attn_bwd_b16) beside the fp32 kernels
(csrc/attn.hip) alone, the fp32 kernels with the two casts a bf16 network would wrap around them (bf16 -> fp32 in front, fp32 ->
bf16 behind, in each direction), F.scaled_dot_product_attention on bf16 and the explicit torch composition on bf16, on the same
GPU and the same random data; then one training step of ViTBased("vit_small_patch16_224") with math="fp32" and math="bf16",
alternating in the same call, and the launch list of one bf16 step.

    python scripts/attn16_bench.py [--out profiles/attn16_kernels.txt] [--repeats 5] [--errors FILE] [--resources FILE]

The method is that of scripts/attn_bench.py: B = 32, N = 197, D = 64, H = 6 / 12 / 16; every time is the median [min .. max] of
`--repeats` windows of device-event time after a warm-up of the same shape, the candidates alternating window by window; the
kernels' outputs are allocated once, outside the windows.  TFLOP/s = the algorithm's 4 B H N^2 D (forward) or 10 B H N^2 D
(backward) over the median.  Peak MB = torch's peak allocation above what was live before one forward + backward.  The launch
list is torch.profiler's device-kernel table of one step (name, launches, total device time): the dtype casts show as torch's
copy kernels, the GELU as mink's activation kernels beside the copies that feed them.  `--errors FILE`: lines (what
tests/test_gpu_vit_bf16.py prints) copied to the end of the output; `--resources FILE`: likewise, the registers, LDS and scratch
of the kernels as `hipcc -Rpass-analysis=kernel-resource-usage` reports them when csrc/attn16.hip is compiled.  Nothing is gated on these numbers.  Needs the GPU."""
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
from nerf_downstream_amd.minkowski import attention, attention_b16  # noqa: E402

B, N, D = 32, 197, 64
HEADS = (6, 12, 16)
BF = torch.bfloat16


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
        qkv16, dout16 = qkv.to(BF), dout.to(BF)
        out, dqkv = torch.empty(B * N, W, device=dev), torch.empty(B * N, 3 * W, device=dev)
        out16, dqkv16 = torch.empty(B * N, W, device=dev, dtype=BF), torch.empty(B * N, 3 * W, device=dev, dtype=BF)
        lse = torch.empty(B, H, N, device=dev)
        ws = torch.empty(L.mink_attn_bwd_workspace_bytes(B, N, H, D), dtype=torch.uint8, device=dev)
        ws16 = torch.empty(L.mink_attn_bwd_b16_workspace_bytes(B, N, H, D), dtype=torch.uint8, device=dev)
        qg, qg16 = qkv.clone().requires_grad_(True), qkv16.clone().requires_grad_(True)

        def fwd16():
            check(L.mink_attn_fwd_b16(qkv16.data_ptr(), 3 * W, B, N, H, D, scale, out16.data_ptr(), W, lse.data_ptr(), st))

        def bwd16():
            check(L.mink_attn_bwd_b16(qkv16.data_ptr(), 3 * W, out16.data_ptr(), W, lse.data_ptr(), dout16.data_ptr(), W, B, N, H, D,
                                      scale, dqkv16.data_ptr(), 3 * W, ws16.data_ptr(), ws16.numel(), st))

        def fwd32(x=qkv, o=out):
            check(L.mink_attn_fwd(x.data_ptr(), 3 * W, B, N, H, D, scale, o.data_ptr(), W, lse.data_ptr(), st))

        def bwd32(x=qkv, o=out, go=dout, gx=dqkv):
            check(L.mink_attn_bwd(x.data_ptr(), 3 * W, o.data_ptr(), W, lse.data_ptr(), go.data_ptr(), W, B, N, H, D, scale,
                                  gx.data_ptr(), 3 * W, ws.data_ptr(), ws.numel(), st))

        def fwd32_casts():  # what a bf16 network pays around the fp32 kernel: qkv up, out down
            fwd32(qkv16.float())
            return out.to(BF)

        def bwd32_casts():  # dout up, dqkv down (qkv and out are the forward's fp32 copies)
            bwd32(go=dout16.float())
            return dqkv.to(BF)

        def both16():
            fwd16(), bwd16()

        def both32():
            fwd32(), bwd32()

        def both32_casts():
            fwd32_casts(), bwd32_casts()

        def heads(x):
            return x.reshape(B, N, 3, H, D).permute(2, 0, 3, 1, 4)

        def torch_fwd(x=qkv16):
            q, k, v = heads(x)
            return (torch.softmax((q @ k.transpose(-2, -1)) * scale, dim=-1) @ v).transpose(1, 2).reshape(B * N, W)

        def sdpa_fwd(x=qkv16):
            q, k, v = heads(x)
            return F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B * N, W)

        def torch_fwd_bwd():
            qg16.grad = None
            torch_fwd(qg16).backward(dout16)

        def sdpa_fwd_bwd():
            qg16.grad = None
            sdpa_fwd(qg16).backward(dout16)

        def torch_fwd_only():
            with torch.no_grad():
                torch_fwd()

        def sdpa_fwd_only():
            with torch.no_grad():
                sdpa_fwd()

        def function16():
            qg16.grad = None
            attention_b16(qg16, B, N, H).backward(dout16)

        def function32():
            qg.grad = None
            attention(qg, B, N, H).backward(dout)

        def function32_casts():
            qg16.grad = None
            attention(qg16.float(), B, N, H).to(BF).backward(dout16)

        both32()
        both16()
        d_out = float((out16.float() - out).abs().max())
        d_grad = float((dqkv16.float() - dqkv).abs().max() / dqkv.abs().max())
        t = time_windows([fwd16, bwd16, both16, fwd32, bwd32, both32, fwd32_casts, bwd32_casts, both32_casts, sdpa_fwd_only,
                          sdpa_fwd_bwd, torch_fwd_only, torch_fwd_bwd], args.repeats, target_ms=args.window_ms)
        mem = [peak_mb(function16), peak_mb(function32), peak_mb(function32_casts), peak_mb(sdpa_fwd_bwd), peak_mb(torch_fwd_bwd)]
        ff, bf = 4.0 * B * H * N * N * D, 10.0 * B * H * N * N * D
        lines += [f"H = {H} (B = {B}, N = {N}, D = {D}; bf16 qkv is {2 * B * N * 3 * W / 1e6:.1f} MB)",
                  f"  mink_attn_fwd_b16                   {fmt(t[0])} ms   {ff / t[0][0] / 1e9:7.2f} TFLOP/s",
                  f"  mink_attn_bwd_b16 (3 launches)      {fmt(t[1])} ms   {bf / t[1][0] / 1e9:7.2f} TFLOP/s",
                  f"  b16 fwd + bwd                       {fmt(t[2])} ms   peak {mem[0]:7.1f} MB (through AttentionB16Function)",
                  f"  mink_attn_fwd (fp32)                {fmt(t[3])} ms   fp32 / b16 {t[3][0] / t[0][0]:5.2f}x",
                  f"  mink_attn_bwd (fp32)                {fmt(t[4])} ms   fp32 / b16 {t[4][0] / t[1][0]:5.2f}x",
                  f"  fp32 fwd + bwd                      {fmt(t[5])} ms   fp32 / b16 {t[5][0] / t[2][0]:5.2f}x   peak {mem[1]:7.1f} MB",
                  f"  fp32 fwd with casts (qkv up, out down)   {fmt(t[6])} ms   / b16 {t[6][0] / t[0][0]:5.2f}x",
                  f"  fp32 bwd with casts (dout up, dqkv down) {fmt(t[7])} ms   / b16 {t[7][0] / t[1][0]:5.2f}x",
                  f"  fp32 fwd + bwd with casts           {fmt(t[8])} ms   / b16 {t[8][0] / t[2][0]:5.2f}x   peak {mem[2]:7.1f} MB",
                  f"  F.scaled_dot_product_attention bf16 {fmt(t[9])} ms   sdpa / b16 {t[9][0] / t[0][0]:5.2f}x",
                  f"  sdpa bf16 fwd + autograd bwd        {fmt(t[10])} ms   sdpa / b16 {t[10][0] / t[2][0]:5.2f}x   peak {mem[3]:7.1f} MB",
                  f"  torch matmul-softmax-matmul bf16    {fmt(t[11])} ms   torch / b16 {t[11][0] / t[0][0]:5.2f}x",
                  f"  torch bf16 fwd + autograd bwd       {fmt(t[12])} ms   torch / b16 {t[12][0] / t[2][0]:5.2f}x   peak {mem[4]:7.1f} MB",
                  f"  max |out_b16 - out_fp32| {d_out:.1e}, max |dqkv_b16 - dqkv_fp32| / max |dqkv| {d_grad:.1e} (fp32 kernels on the unrounded data)",
                  ""]
        print("\n".join(lines[-16:]), flush=True)
        del qkv, dout, out, dqkv, lse, ws, qg, qkv16, dout16, out16, dqkv16, ws16, qg16
        torch.cuda.empty_cache()
    return lines


def launch_list(step, top=40):
    """torch.profiler's device-kernel table of one call of step(): name, launches, total device microseconds"""
    from torch.profiler import ProfilerActivity, profile

    step()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    rows = {}
    for ev in prof.events():
        if getattr(ev, "device_type", None) is not None and str(ev.device_type).endswith("CUDA"):
            us = float(getattr(ev, "device_time_total", 0.0) or getattr(ev, "cuda_time_total", 0.0) or 0.0)
            n, tot = rows.get(ev.name, (0, 0.0))
            rows[ev.name] = (n + 1, tot + us)
    if not rows:
        return ["  (the profiler recorded no device kernels on this machine)"]
    total = sum(v[1] for v in rows.values())
    out = [f"  {len(rows)} distinct kernels, {sum(v[0] for v in rows.values())} launches, {total / 1e3:.3f} ms of device time; the {top} longest:",
           "    launches   total us   share  kind   kernel"]
    for name, (n, us) in sorted(rows.items(), key=lambda kv: -kv[1][1])[:top]:
        low = name.lower()
        kind = ("cast" if "copy" in low else "gelu" if "activation" in low else "attn" if "attn" in low else
                "gemm" if ("gemm" in low or "cijk" in low) else "")
        out.append(f"    {n:8d} {us:10.1f}  {100 * us / max(total, 1e-9):5.1f}%  {kind:5s}  {name[:120]}")
    casts = [(n, us) for name, (n, us) in rows.items() if "copy" in name.lower()]
    out.append(f"  torch copy kernels (dtype casts and layout copies): {sum(c[0] for c in casts)} launches, {sum(c[1] for c in casts) / 1e3:.3f} ms")
    return out


def step_lines(args, dev):
    """One training step (forward, cross entropy, backward, SGD) of ViT-Small / 16 on a batch of 32 random 224^2 images, with
    math="fp32" and math="bf16" on the same weights, alternating window by window."""
    from nerf_downstream_amd.co3d_2d.src.model.models import ViTBased

    images, labels = torch.randn(B, 3, 224, 224, device=dev), torch.randint(0, 51, (B,), device=dev)
    steps = {}
    for math in ("fp32", "bf16"):
        torch.manual_seed(0)
        net = ViTBased("vit_small_patch16_224", math=math).to(dev).train()
        opt = torch.optim.SGD(net.parameters(), lr=0.003, momentum=0.9)

        def step(net=net, opt=opt):
            opt.zero_grad(set_to_none=True)
            F.cross_entropy(net(images), labels).backward()
            opt.step()

        for _ in range(3):
            step()
        steps[math] = step
    t = time_windows([steps["fp32"], steps["bf16"]], args.repeats, target_ms=8 * args.window_ms)
    mem = [peak_mb(steps["fp32"]), peak_mb(steps["bf16"])]
    lines = [f"one training step of ViTBased('vit_small_patch16_224'), B = {B}, 224^2 (forward, cross entropy, backward, torch SGD):",
             f"  math=\"fp32\"  {fmt(t[0])} ms   {B / t[0][0] * 1e3:7.1f} images/s   peak {mem[0]:7.1f} MB above the parameters and optimizer state",
             f"  math=\"bf16\"  {fmt(t[1])} ms   {B / t[1][0] * 1e3:7.1f} images/s   peak {mem[1]:7.1f} MB   fp32 / bf16 {t[0][0] / t[1][0]:5.2f}x",
             "", "launch list of one math=\"bf16\" step:"]
    return lines + launch_list(steps["bf16"]) + [""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=40.0)
    ap.add_argument("--errors", default=None, help="a text file whose lines are appended (what tests/test_gpu_vit_bf16.py prints)")
    ap.add_argument("--resources", default=None, help="a text file whose lines are appended (the compiler's kernel resource usage)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "attn16_bench needs the GPU"
    dev = torch.device("cuda")
    lines = [f"attn16_bench: bf16 rows, {torch.cuda.get_device_name(0)}",
             f"command: python scripts/attn16_bench.py --repeats {args.repeats} --window_ms {args.window_ms} --out FILE",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time; random normal data", ""]
    print("\n".join(lines), flush=True)
    lines += operator_lines(args, dev)
    tail = step_lines(args, dev)
    print("\n".join(tail), flush=True)
    lines += tail
    for title, path in (("kernel resource usage (hipcc -Rpass-analysis=kernel-resource-usage, gfx950):", args.resources),
                        ("model-level errors against float64 (printed by tests/test_gpu_vit_bf16.py on the same GPU):", args.errors)):
        if path and os.path.exists(path):
            with open(path) as f:
                lines += [title] + ["  " + ln.rstrip() for ln in f if ln.strip()] + [""]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
