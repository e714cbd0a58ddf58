#!/usr/bin/env python3
"""Record what Pillow computes for the pieces of the 2-D recipe -> tests/golden/augmix_pillow_v1.npz.

    python scripts/make_augmix_golden.py

The fixture is data (images in, images out); tests/test_image_cpu.py holds tests/image_restate.py to it and the GPU tests hold
csrc/image.hip to the restatement, so no test needs Pillow.  Images are W x H = 1x1, 1x7, 37x53 and 61x83: flat 6x6 blocks of
twelve colours (so the archive deflates) around a band of smooth gradients, patches of black, white, grey and saturated pixels, and
a green channel confined to a narrow band (autocontrast stretches it; on 61x83 equalize's table runs past 255 and is clamped)."""
import os

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), os.pardir, "tests", "golden", "augmix_pillow_v1.npz")
SIZES = [(1, 1), (1, 7), (37, 53), (61, 83)]
RESAMPLE = getattr(Image, "Resampling", Image).BILINEAR
AFFINE = getattr(Image, "Transform", Image).AFFINE
S = 16
GEOMETRIC = {"rotate": 7, "shear_x": 0.21, "shear_y": 0.13, "translate_x": 5, "translate_y": 3}


def make_image(W, H, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    pal = rng.integers(0, 256, (12, 3))
    blocks = pal[rng.integers(0, 12, (H // 6 + 1, W // 6 + 1))].repeat(6, 0).repeat(6, 1)[:H, :W].astype(np.float64)
    band = (yy >= 8) & (yy < 20)  # twelve rows of smooth gradients; the rest is flat 6x6 blocks of twelve colours
    r = np.where(band, 128 + 100 * np.sin(xx / 9.0 + yy / 17.0), blocks[..., 0])
    g = 120 + np.where(band, 12 * np.cos(xx / 5.0), blocks[..., 1] / 12.0 - 10)  # the narrow band
    b = np.where(band, 255.0 * (xx + yy) / max(W + H - 2, 1), blocks[..., 2])
    img = np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)
    if H > 8:
        img[:4, :4] = [[0, 0, 0], [255, 255, 255], [77, 77, 77], [255, 0, 0]]  # black, white, grey, saturated columns
        img[4:8, :4] = [[0, 255, 0], [0, 0, 255], [255, 255, 0], [1, 0, 0]]
    return img


def crop_cases(W, H):
    """(box x0, y0, w, h; target OW, OH; window wx, wy): an upscale, a downscale, a box on two borders, the centre-crop form."""
    cases = [((0, 0, min(W, 5), min(H, 5)), (S, S), (0, 0)), ((0, 0, W, H), (S, S), (0, 0)),
             ((W - max(W // 2, 1), H - max(H // 3, 1), max(W // 2, 1), max(H // 3, 1)), (S, S), (0, 0))]
    if W <= H:
        ow, oh = S, int(S * H / W)
    else:
        oh, ow = S, int(S * W / H)
    cases.append(((0, 0, W, H), (ow, oh), (int(round((ow - S) / 2.0)), int(round((oh - S) / 2.0)))))
    return cases


def main():
    out = {"pillow_version": np.array(PIL.__version__), "sizes": np.array(SIZES, np.int32), "S": np.array(S),
           "geometric_names": np.array(list(GEOMETRIC)), "geometric_params": np.array(list(GEOMETRIC.values()), np.float64)}
    for n, (W, H) in enumerate(SIZES):
        arr = make_image(W, H, 100 + n)
        im = Image.fromarray(arr)
        put = lambda name, v: out.__setitem__(f"i{n}_{name}", np.asarray(v))  # noqa: E731
        put("image", arr)
        put("autocontrast", ImageOps.autocontrast(im))
        put("equalize", ImageOps.equalize(im))
        for bits in (3, 4):
            put(f"posterize_{bits}", ImageOps.posterize(im, bits))
        for t in (256 - 76, 256 - 3):
            put(f"solarize_{t}", ImageOps.solarize(im, t))
        for name, p in GEOMETRIC.items():
            for sign in (1, -1):
                v = sign * p
                if name == "rotate":
                    res = im.rotate(v, resample=RESAMPLE)
                else:
                    m = {"shear_x": (1, v, 0, 0, 1, 0), "shear_y": (1, 0, 0, v, 1, 0), "translate_x": (1, 0, v, 0, 1, 0),
                         "translate_y": (1, 0, 0, 0, 1, v)}[name]
                    res = im.transform(im.size, AFFINE, m, resample=RESAMPLE)
                put(f"{name}_{'p' if sign > 0 else 'm'}", res)
        cases = crop_cases(W, H)
        put("crop_cases", np.array([list(b) + list(t) + list(w) for b, t, w in cases], np.int32))
        for c, (box, target, window) in enumerate(cases):
            x0, y0, w, h = box
            res = im.crop((x0, y0, x0 + w, y0 + h)).resize(target, RESAMPLE)
            put(f"crop_{c}", np.asarray(res)[window[1]:window[1] + S, window[0]:window[0] + S])
        for f in (0.63, 1.37):
            put(f"brightness_{f}", ImageEnhance.Brightness(im).enhance(f))
            put(f"saturation_{f}", ImageEnhance.Color(im).enhance(f))
        hsv = im.convert("HSV")
        put("hsv", hsv)
        for shift in (0, 37, -101):
            h, s, v = hsv.split()
            nh = np.array(h, dtype=np.uint8)
            with np.errstate(over="ignore"):
                nh += np.array(shift).astype(np.uint8)
            put(f"hsv_to_rgb_{shift}", Image.merge("HSV", (Image.fromarray(nh, "L"), s, v)).convert("RGB"))
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    np.savez_compressed(OUT, **out)
    print(f"{OUT}: {os.path.getsize(OUT)} bytes, {len(out)} arrays, Pillow {PIL.__version__}")


if __name__ == "__main__":
    main()
