"""Times the image kernels (csrc/image.hip: mink_img_chain_round / mink_img_finish) on the 2-D loader's workload: B = 32 frames of
800x600, the reference's defaults (AugMix severity 3, width 3, stochastic depth; RandomResizedCrop to 224, ColorJitter .4/.4/.4,
flip, PCA lighting, Normalize), once with textured frames and once with frames that are one constant colour (the worst case of
the histogram: every lane of a wave hits the same bin).

    python scripts/augmix_bench.py [--out profiles/augmix_kernels.txt] [--repeats 5]

Recorded: every round of the chains (its three launches: histograms, tables, apply), the fused tail, the whole
`prepare_image_batch` (uploads of the program included, the frames already on the device) and with the host-to-device copy of the
frames; a resnet50 training step fed from such a batch beside the same step on a SyntheticRenders batch; and, where Pillow is
installed, the same recipe through Pillow per sample on one core of this machine (decode not included: it stays in the workers
either way).  Every GPU figure is the median [min .. max] of `--repeats` windows of device-event time after a warm-up of the same
shape, the timed functions alternating window by window.  Nothing is gated on these numbers.  Needs the GPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from dgcnn_bench import time_windows  # noqa: E402
from nerf_downstream_amd import gin_lite as gin  # noqa: E402
from nerf_downstream_amd._lib import check, constants, lib  # noqa: E402
from nerf_downstream_amd.co3d_2d.src.data import transforms as T  # noqa: E402
from nerf_downstream_amd.minkowski.utils import prepare_image_batch  # noqa: E402

B, W, H, S = 32, 800, 600, 224
IMG = constants("MINK_IMG_")


def fmt(t):
    return f"{t[0]:8.4f} [{t[1]:.4f} .. {t[2]:.4f}]"


def frames(kind):
    rng = np.random.default_rng(0)
    if kind == "constant":
        return [np.full((H, W, 3), rng.integers(0, 256, 3), np.uint8) for _ in range(B)]
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for _ in range(B):
        f = rng.uniform(0.01, 0.08, 6)
        img = np.stack([127 + 90 * np.sin(f[2 * c] * xx + f[2 * c + 1] * yy) for c in range(3)], -1) + rng.normal(0, 12, (H, W, 3))
        out.append(np.clip(img, 0, 255).astype(np.uint8))
    return out


def draws():
    np.random.seed(0)
    recipe = T.Compose(T.TRAIN_ORDER)
    return [T.AugMix().draw((W, H), recipe.draw) for _ in range(B)]


def pillow_ms_per_sample(images, samples, n=4):
    """The reference's path for the same draws: every chain op, crop + resize, the jitter steps, flip and the float conversion
    through Pillow and numpy, one sample at a time on this core."""
    try:
        from PIL import Image, ImageEnhance, ImageOps
    except ImportError:
        return None
    BIL, AFF = getattr(Image, "Resampling", Image).BILINEAR, getattr(Image, "Transform", Image).AFFINE
    names = {IMG["OP_AUTOCONTRAST"]: "a", IMG["OP_EQUALIZE"]: "e", IMG["OP_POSTERIZE"]: "p", IMG["OP_SOLARIZE"]: "s"}
    t0 = time.perf_counter()
    for img, smp in list(zip(images, samples))[:n]:
        base = Image.fromarray(img)
        for k, b in enumerate(smp["branches"]):
            im = base
            for op in b.get("ops", []) if k else []:
                kind = names.get(op[0])
                im = (ImageOps.autocontrast(im) if kind == "a" else ImageOps.equalize(im) if kind == "e" else
                      ImageOps.posterize(im, op[1]) if kind == "p" else ImageOps.solarize(im, op[1]) if kind == "s" else
                      im.transform(im.size, AFF, tuple(op[1:7]), resample=BIL))
            x0, y0, w, h = b["box"]
            im = im.crop((x0, y0, x0 + w, y0 + h)).resize((S, S), BIL)
            for j in b["order"]:
                if j == IMG["JIT_BRIGHTNESS"]:
                    im = ImageEnhance.Brightness(im).enhance(b["factors"][0])
                elif j == IMG["JIT_SATURATION"]:
                    im = ImageEnhance.Color(im).enhance(b["factors"][1])
                else:
                    hh, ss, vv = im.convert("HSV").split()
                    nh = ((np.array(hh, dtype=np.int32) + int(b["factors"][2] * 255)) % 256).astype(np.uint8)
                    im = Image.merge("HSV", (Image.fromarray(nh, "L"), ss, vv)).convert("RGB")
            x = np.asarray(im, dtype=np.float32).transpose(2, 0, 1) / 255.0
            x = (x[:, :, ::-1] if b["flip"] else x) + b["rgb"][:, None, None]
    return (time.perf_counter() - t0) * 1e3 / n


def kernel_lines(args, dev, kind, samples):
    images = frames(kind)
    rows = np.stack([T.compile_program(s) for s in samples])
    flat = np.concatenate([im.reshape(-1) for im in images])
    offsets = np.arange(B + 1, dtype=np.int64) * (3 * W * H)
    sizes = np.tile(np.array([[W, H]], np.int32), (B, 1))
    host = torch.from_numpy(flat).pin_memory()
    packed = host.to(dev)
    d_off, d_sz, d_rows = torch.from_numpy(offsets).to(dev), torch.from_numpy(sizes).to(dev), torch.from_numpy(rows).to(dev)
    L, n = lib(), flat.size // 3
    ws = torch.empty(L.mink_img_workspace_bytes(n, B, 3, S), dtype=torch.uint8, device=dev)
    out = torch.empty(B, 3, S, S, device=dev)
    st = torch.cuda.current_stream().cuda_stream

    def round_(r):
        return lambda: check(L.mink_img_chain_round(packed.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), d_rows.data_ptr(), n, B, 3, r,
                                                    ws.data_ptr(), ws.numel(), st))

    def finish():
        check(L.mink_img_finish(packed.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), d_rows.data_ptr(), n, B, 3, S, ws.data_ptr(),
                                ws.numel(), out.data_ptr(), None, st))

    def prepare():
        return prepare_image_batch(packed, offsets, sizes, rows, size=S)

    def copy_and_prepare():
        return prepare_image_batch(host.to(dev, non_blocking=True), offsets, sizes, rows, size=S)

    for r in range(3):
        round_(r)()
    t = time_windows([round_(0), round_(1), round_(2), finish, prepare, copy_and_prepare], args.repeats, target_ms=args.window_ms)
    depth = [sum(len(b["ops"]) > r for s in samples for b in s["branches"][1:]) for r in range(3)]
    lines = [f"{kind} frames: B = {B} of {W}x{H} ({flat.size / 1e6:.0f} MB), S = {S}; chains reaching round 0 / 1 / 2: {depth} of {3 * B}",
             *(f"  mink_img_chain_round r = {r}       {fmt(t[r])} ms" for r in range(3)),
             f"  mink_img_finish                  {fmt(t[3])} ms",
             f"  prepare_image_batch              {fmt(t[4])} ms   (program upload, three rounds, tail)",
             f"  ... with the copy of the frames  {fmt(t[5])} ms   (pinned host memory -> device)"]
    if kind == "textured":
        p = pillow_ms_per_sample(images, samples)
        if p is not None:
            lines.append(f"  the same draws through Pillow    {p:8.2f} ms per SAMPLE on one core of this machine = {p * B:.0f} ms per batch "
                         f"of CPU time ({p * B / 16:.1f} ms across 16 workers)")
    return lines + [""], t[5][0], (host, offsets, sizes, rows)


def step_lines(args, dev, batch):
    """One resnet50 training step (bf16 matrix cores, as configs/resnet50.gin) fed by a frames batch -- copy, prepare, forward,
    backward, SGD -- beside the same step on a SyntheticRenders batch (copy of the ready float tensor, forward, backward, SGD)."""
    from nerf_downstream_amd.co3d_2d.src.data.loader import SyntheticRenders
    from nerf_downstream_amd.co3d_2d.src.modules.classification import LitModel
    from nerf_downstream_amd.minkowski import functional as Fn

    gin.clear_config()
    torch.manual_seed(0)
    model = LitModel(model_name="resnet50").to(dev).train()
    opt = model.configure_optimizers()
    ds = SyntheticRenders("train")
    syn = torch.stack([ds[i]["images"] for i in range(B)]).pin_memory()
    labels = torch.arange(B, device=dev) % 51
    host, offsets, sizes, rows = batch

    def step(images):
        opt.zero_grad(set_to_none=True)
        loss, _ = model.training_step({"images": images, "labels": labels})
        loss.backward()
        opt.step()

    old = Fn.set_conv_math("bf16")
    try:
        fns = [lambda: step(syn.to(dev, non_blocking=True)),
               lambda: step(prepare_image_batch(host.to(dev, non_blocking=True), offsets, sizes, rows, size=S))]
        for f in fns:
            for _ in range(3):
                f()
        t = time_windows(fns, args.repeats, target_ms=8 * args.window_ms)
    finally:
        Fn.set_conv_math(old)
    return [f"one resnet50 training step, batch {B}, bf16 matrix cores (forward, loss, backward, torch SGD), input copy included:",
            f"  SyntheticRenders batch           {fmt(t[0])} ms",
            f"  frames batch (source = files)    {fmt(t[1])} ms   difference {t[1][0] - t[0][0]:.3f} ms = "
            f"{100 * (t[1][0] - t[0][0]) / t[0][0]:.1f} % of the step", ""]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=40.0)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "augmix_bench needs the GPU"
    dev = torch.device("cuda", 0)
    lines = [f"augmix_bench: {torch.cuda.get_device_name(0)}",
             f"command: python scripts/augmix_bench.py --repeats {args.repeats} --window_ms {args.window_ms} --out FILE",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time", ""]
    print("\n".join(lines), flush=True)
    samples = draws()
    batch = None
    for kind in ("textured", "constant"):
        got, _, b = kernel_lines(args, dev, kind, samples)
        batch = batch or b
        print("\n".join(got), flush=True)
        lines += got
        torch.cuda.empty_cache()
    tail = step_lines(args, dev, batch)
    print("\n".join(tail), flush=True)
    lines += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
