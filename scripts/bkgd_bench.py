"""Times the background paste (csrc/paste.hip: mink_img_paste) on the 2-D loader's workload, at the shape of
scripts/augmix_bench.py: B = 32 background frames of 800x600, every sample pasting an 800x600 render through an 800x600 mask,
the scales spread evenly over BackgroundAug's range 0.5 .. 1.5 (resized frames of 400x300 .. 1200x900; from scale 1 on the
rectangle is the whole slot).

    python scripts/bkgd_bench.py [--out profiles/bkgd_kernels.txt] [--repeats 5]

Recorded: the paste alone; `prepare_image_batch` without and with it (the yardstick is the call without, re-measured here: the
parent commit's whole device-side preparation); the same pastes through Pillow and numpy per sample on one core of this machine,
where Pillow is installed; and a resnet50 training step fed from host batches as `collate_images` builds them for bkgd_aug = 0,
0.5 and 1.0 (a pasting sample sends three images over the host link instead of one).  The paste works in place, so every timed
call after the first composites over a composite: the work does not depend on the bytes.  Every GPU figure is the median
[min .. max] of `--repeats` windows of device-event time after a warm-up of the same shape, the timed functions alternating
window by window.  Nothing is gated on these numbers.  Needs the GPU."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from augmix_bench import B, H, S, W, draws, fmt, frames  # noqa: E402
from dgcnn_bench import time_windows  # noqa: E402
from nerf_downstream_amd import gin_lite as gin  # noqa: E402
from nerf_downstream_amd._lib import check, constants, lib  # noqa: E402
from nerf_downstream_amd.co3d_2d.src.data import transforms as T  # noqa: E402
from nerf_downstream_amd.minkowski.utils import image_paste_check, prepare_image_batch  # noqa: E402

P = constants("MINK_PASTE_")


def masks():
    yy, xx = np.mgrid[0:H, 0:W]
    out = []
    for b in range(B):
        d = np.hypot((xx - W / 2) / (W * (0.25 + 0.01 * b)), (yy - H / 2) / (H * 0.35))
        out.append(np.clip(255 * (1.2 - d) / 0.4, 0, 255).astype(np.uint8))
    return out


def table_of(pasting, sizes_rw_rh):
    t = np.zeros((B, P["PARAMS"]), np.int64)
    fo = mo = 0
    for b in range(B):
        if not pasting[b]:
            continue
        t[b, [P["FG_OFFSET"], P["MASK_OFFSET"], P["FG_W"], P["FG_H"], P["MASK_W"], P["MASK_H"], P["RW"], P["RH"]]] = [
            fo, mo, W, H, W, H, sizes_rw_rh[b][0], sizes_rw_rh[b][1]]
        fo, mo = fo + 3 * W * H, mo + W * H
    return t, fo, mo


def pillow_ms_per_sample(bgs, fgs, mks, sizes_rw_rh, n=8):
    """The reference's path for the same pastes: two Image.resize calls and the float64 composite, one sample at a time."""
    try:
        from PIL import Image
    except ImportError:
        return None
    idx = np.linspace(0, B - 1, n).astype(int)  # (spread over the scales)
    t0 = time.perf_counter()
    for b in idx:
        rw, rh = sizes_rw_rh[b]
        fg = np.asarray(Image.fromarray(fgs[b]).resize((rw, rh)))
        m = np.asarray(Image.fromarray(np.repeat(mks[b][..., None], 3, -1)).resize((rw, rh)))[..., 0] / 255
        out = np.array(bgs[b])
        top, left = max(0, (H - rh) // 2), max(0, (W - rw) // 2)
        eh, ew = min(H, (H + rh) // 2) - top, min(W, (W + rw) // 2) - left
        y, x = rh // 2 - eh // 2, rw // 2 - ew // 2
        mm = m[y:y + eh, x:x + ew, None]
        out[top:top + eh, left:left + ew] = fg[y:y + eh, x:x + ew] * mm + (1 - mm) * out[top:top + eh, left:left + ew]
    return (time.perf_counter() - t0) * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--window_ms", type=float, default=40.0)
    ap.add_argument("--no_step", action="store_true", help="leave the resnet50 step out")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bkgd_bench needs the GPU"
    dev = torch.device("cuda", 0)
    lines = [f"bkgd_bench: {torch.cuda.get_device_name(0)}",
             f"command: python scripts/bkgd_bench.py --repeats {args.repeats} --window_ms {args.window_ms} --out FILE",
             f"median [min .. max] ms per call over {args.repeats} windows of device-event time", ""]
    bgs, mks = frames("textured"), masks()
    fgs = [np.ascontiguousarray(f[::-1, ::-1]) for f in bgs[1:] + bgs[:1]]  # other frames, turned round
    scales = np.linspace(0.5, 1.5, B)
    sizes_rw_rh = [(int(W * s), int(H * s)) for s in scales]
    rows = np.stack([T.compile_program(s) for s in draws()])
    offsets = np.arange(B + 1, dtype=np.int64) * (3 * W * H)
    sizes = np.tile(np.array([[W, H]], np.int32), (B, 1))
    h_packed = torch.from_numpy(np.concatenate([f.reshape(-1) for f in bgs])).pin_memory()
    h_fg = torch.from_numpy(np.concatenate([f.reshape(-1) for f in fgs])).pin_memory()
    h_mask = torch.from_numpy(np.concatenate([m.reshape(-1) for m in mks])).pin_memory()
    packed, fg, mask = h_packed.to(dev), h_fg.to(dev), h_mask.to(dev)
    table, fo, mo = table_of([True] * B, sizes_rw_rh)
    max_w, max_h = image_paste_check(table, sizes, fo, mo)
    d_off, d_sz, d_tab = torch.from_numpy(offsets).to(dev), torch.from_numpy(sizes).to(dev), torch.from_numpy(table).to(dev)
    L, st = lib(), torch.cuda.current_stream().cuda_stream

    def paste_alone():
        check(L.mink_img_paste(packed.data_ptr(), d_off.data_ptr(), d_sz.data_ptr(), packed.numel() // 3, B, fg.data_ptr(), fo,
                               mask.data_ptr(), mo, d_tab.data_ptr(), max_w, max_h, st))

    def prepare():
        return prepare_image_batch(packed, offsets, sizes, rows, size=S)

    def prepare_with_paste():
        return prepare_image_batch(packed, offsets, sizes, rows, size=S, paste={"fg": fg, "mask": mask, "table": table})

    t = time_windows([paste_alone, prepare, prepare_with_paste], args.repeats, target_ms=args.window_ms)
    px = sum(min(W, rw) * min(H, rh) for rw, rh in sizes_rw_rh)
    lines += [f"B = {B} slots of {W}x{H} ({packed.numel() / 1e6:.0f} MB), every sample pasting a {W}x{H} render through a {W}x{H} mask "
              f"({(fo + mo) / 1e6:.0f} MB more), scales {scales[0]:.2f} .. {scales[-1]:.2f}, {px / 1e6:.1f} M composited pixels",
              f"  mink_img_paste                   {fmt(t[0])} ms   ({px / t[0][0] / 1e6:.2f} G pixels/s)",
              f"  prepare_image_batch              {fmt(t[1])} ms   (the yardstick: program upload, three rounds, tail)",
              f"  prepare_image_batch(paste=...)   {fmt(t[2])} ms   (table upload and the paste before them)",
              f"  the paste alone is {100 * t[0][0] / t[1][0]:.0f} % of the call without it"]
    p = pillow_ms_per_sample(bgs, fgs, mks, sizes_rw_rh)
    if p is not None:
        lines.append(f"  the same pastes through Pillow   {p:8.2f} ms per SAMPLE on one core of this machine = {p * B:.0f} ms per batch of "
                     f"CPU time ({p * B / 16:.1f} ms across 16 workers)")
    lines.append("")
    print("\n".join(lines), flush=True)
    if not args.no_step:
        tail = step_lines(args, dev, (h_packed, h_fg, h_mask, offsets, sizes, rows, sizes_rw_rh))
        print("\n".join(tail), flush=True)
        lines += tail
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def step_lines(args, dev, batch):
    """One resnet50 training step (bf16 matrix cores, as configs/resnet50.gin) fed from pinned host batches -- copies, prepare,
    forward, backward, SGD -- with none, every second and every sample pasting."""
    from nerf_downstream_amd.co3d_2d.src.modules.classification import LitModel
    from nerf_downstream_amd.minkowski import functional as Fn

    h_packed, h_fg, h_mask, offsets, sizes, rows, sizes_rw_rh = batch
    gin.clear_config()
    torch.manual_seed(0)
    model = LitModel(model_name="resnet50").to(dev).train()
    opt = model.configure_optimizers()
    labels = torch.arange(B, device=dev) % 51

    def feed(share):
        pasting = [share == 1.0 or (share == 0.5 and b % 2 == 0) for b in range(B)]
        table, fo, mo = table_of(pasting, sizes_rw_rh)
        hf, hm = h_fg[:fo], h_mask[:mo]  # (what collate_images packs: only the pasting samples' frames and masks)

        def step():
            paste = None
            if fo:
                paste = {"fg": hf.to(dev, non_blocking=True), "mask": hm.to(dev, non_blocking=True), "table": table}
            images = prepare_image_batch(h_packed.to(dev, non_blocking=True), offsets, sizes, rows, size=S, paste=paste)
            opt.zero_grad(set_to_none=True)
            loss, _ = model.training_step({"images": images, "labels": labels})
            loss.backward()
            opt.step()

        return step, (h_packed.numel() + fo + mo) / 1e6

    old = Fn.set_conv_math("bf16")
    try:
        fns, mbs = zip(*(feed(s) for s in (0.0, 0.5, 1.0)))
        for f in fns:
            for _ in range(3):
                f()
        t = time_windows(list(fns), args.repeats, target_ms=8 * args.window_ms)
    finally:
        Fn.set_conv_math(old)
    out = [f"one resnet50 training step, batch {B}, bf16 matrix cores (forward, loss, backward, torch SGD), host-to-device copies included:"]
    for share, ti, mb in zip((0.0, 0.5, 1.0), t, mbs):
        out.append(f"  bkgd_aug = {share:.1f} ({mb:4.0f} MB over the host link)   {fmt(ti)} ms"
                   + ("" if share == 0 else f"   + {ti[0] - t[0][0]:.3f} ms = {100 * (ti[0] - t[0][0]) / t[0][0]:.1f} % of the step without"))
    return out + [""]


if __name__ == "__main__":
    main()
