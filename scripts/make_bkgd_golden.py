#!/usr/bin/env python3
"""Record what Pillow and numpy compute for the background paste -> tests/golden/bkgd_pillow_v1.npz.

    python scripts/make_bkgd_golden.py

Per case: the frame `fg`, band 0 of its mask, the background `bg`, the resized size (rw, rh) and the result of Pillow's
`Image.resize` with its default filter followed by numpy's float64 composite on a writable copy of `bg`.  The fixture is data;
tests/test_paste_cpu.py holds tests/paste_restate.py to it and the GPU tests hold csrc/paste.hip to the restatement, so no test
needs Pillow.  The mask goes through Pillow as an RGB image whose other two bands hold something else: only band 0 may matter.

Frames are flat 5x5 blocks of a few colours (so the archive deflates) with one band of noise and one of gradients."""
import os

import numpy as np
import PIL
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tests", "golden", "bkgd_pillow_v1.npz")

# name, fg (w, h), bg (w, h), mask (w, h) or None = fg's, scale, mask kind
CASES = [
    ("p_073_soft", (40, 30), (33, 47), None, 0.73, "soft"),
    ("p_127_binary", (33, 47), (40, 30), None, 1.27, "binary"),
    ("both_passes_skipped", (64, 64), (64, 64), None, 1.0, "soft"),
    ("p_05_thin", (17, 9), (5, 70), None, 0.5, "soft"),
    ("p_14999_thin", (70, 5), (9, 17), None, 1.4999, "binary"),
    ("one_pixel", (2, 2), (3, 3), None, 0.5, "soft"),
    ("p_05000001", (31, 29), (31, 29), None, 0.5000001, "soft"),
    ("p_0999", (31, 29), (31, 29), None, 0.999, "binary"),
    ("p_random", (40, 30), (33, 47), None, None, "soft"),
    ("all_255", (31, 29), (31, 29), None, 1.27, "noise255"),
    ("inside_odd_odd", (40, 30), (64, 64), None, 0.73, "soft"),       # (29, 21) in 64x64: differences 35 and 43
    ("inside_even_even", (40, 30), (64, 47), None, 0.5, "binary"),    # (20, 15) in 64x47: differences 44 and 32
    ("larger_than_bg", (33, 47), (40, 30), None, 1.4999, "soft"),     # (49, 70) over 40x30: differences -9 and -40
    ("wider_but_shorter", (70, 5), (40, 30), None, 1.27, "soft"),     # (88, 6) over 40x30
    ("horizontal_skipped", (3, 40), (9, 17), None, 1.3, "soft"),      # (3, 52): the width does not change
    ("most_taps_odd_sides", (31, 29), (40, 30), None, 0.5, "soft"),   # (15, 14)
    ("mask_of_another_size", (40, 30), (33, 47), (23, 51), 0.73, "soft"),
    ("mask_all_0", (40, 30), (33, 47), None, 1.27, "zeros"),
    ("mask_all_255", (40, 30), (33, 47), None, 1.27, "ones"),
    ("several_tiles", (300, 70), (280, 100), None, 0.9, "soft"),      # (270, 63)
    ("several_row_passes", (70, 300), (64, 64), None, 0.3, "soft"),   # (21, 90): 3.3 source rows per output row
]


def make_image(W, H, rng):
    pal = rng.integers(0, 256, (6, 3))
    img = pal[rng.integers(0, 6, (H // 5 + 1, W // 5 + 1))].repeat(5, 0).repeat(5, 1)[:H, :W].astype(np.float64)
    yy, xx = np.mgrid[0:H, 0:W]
    noisy = (yy % 23) < 5
    img[noisy] = rng.integers(0, 256, (int(noisy.sum()), 3))
    ramp = ((yy % 23) >= 5) & ((yy % 23) < 9)
    img[ramp] = np.stack([255.0 * xx / max(W - 1, 1), 255.0 * yy / max(H - 1, 1), 255 - 255.0 * xx / max(W - 1, 1)], -1)[ramp]
    return np.clip(img, 0, 255).astype(np.uint8)


def make_mask(W, H, kind, rng):
    if kind == "zeros":
        return np.zeros((H, W), np.uint8)
    if kind == "ones":
        return np.full((H, W), 255, np.uint8)
    if kind == "noise255":
        return rng.integers(0, 256, (H, W), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    d = np.hypot((xx + 0.5) / W - 0.5, (yy + 0.5) / H - 0.5)
    if kind == "binary":
        return np.where(d < 0.38, 255, 0).astype(np.uint8)
    soft = np.clip(255 * (0.48 - d) / 0.2, 0, 255)
    soft[: max(H // 6, 1)] = rng.integers(0, 256, (max(H // 6, 1), W))  # a strip of every value
    return soft.astype(np.uint8)


def pillow_paste(fg, mask_plane, bg, size):
    """The frame and the mask through Image.resize (no filter named), then the float64 blend written into a copy of bg."""
    rw, rh = size
    fg_r = np.asarray(Image.fromarray(fg).resize((rw, rh)))
    mask_rgb = np.stack([mask_plane, 255 - mask_plane, mask_plane // 2 + 7], -1).astype(np.uint8)
    m = np.asarray(Image.fromarray(mask_rgb).resize((rw, rh)))[..., 0] / 255
    out = np.array(bg)
    bH, bW = bg.shape[:2]
    top, left = max(0, (bH - rh) // 2), max(0, (bW - rw) // 2)
    bottom, right = min(bH, (bH + rh) // 2), min(bW, (bW + rw) // 2)
    eh, ew = bottom - top, right - left
    y, x = rh // 2 - eh // 2, rw // 2 - ew // 2
    mm = m[y:y + eh, x:x + ew, None]
    out[top:bottom, left:right] = fg_r[y:y + eh, x:x + ew] * mm + (1 - mm) * out[top:bottom, left:right]
    return out


def main():
    rng = np.random.default_rng(20)
    out = {"pillow_version": np.array(PIL.__version__), "names": np.array([c[0] for c in CASES])}
    for name, fg_wh, bg_wh, mask_wh, s, kind in CASES:
        if s is None:
            s = rng.random() * (1.5 - 0.5) + 0.5
        fg, bg = make_image(*fg_wh, rng), make_image(*bg_wh, rng)
        if kind == "noise255":
            fg[:], bg[:] = 255, 255
        mask = make_mask(*(mask_wh or fg_wh), kind, rng)
        size = (int(fg_wh[0] * s), int(fg_wh[1] * s))
        out[f"{name}_fg"], out[f"{name}_mask"], out[f"{name}_bg"] = fg, mask, bg
        out[f"{name}_scale"], out[f"{name}_size"] = np.array(s, np.float64), np.array(size, np.int32)
        out[f"{name}_out"] = pillow_paste(fg, mask, bg, size)
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(CASES)} cases, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
