"""numpy restatement of the 2-D recipe (AugMix chains, crop + resize, ColorJitter, flip, ToTensor, PCA lighting, Normalize) with
Pillow's arithmetic: integers stay integers, every float has the width Pillow / torch compute it in (float32 where Pillow's C code
holds a `float`, float64 where it holds a `double` or Python computes it).  tests/test_image_cpu.py holds it to the recorded
Pillow results of tests/golden/augmix_pillow_v1.npz; the GPU tests hold csrc/image.hip to it.

Nothing here reads the library under test except the layout of the program row (`MINK_IMG_*` of include/mink_hip.h)."""
import math

import numpy as np

f32 = np.float32
MEAN = np.array([123.68 / 255, 116.779 / 255, 103.939 / 255]).astype(f32)
STD = np.array([58.393 / 255, 57.12 / 255, 57.375 / 255]).astype(f32)
OPS = ("autocontrast", "equalize", "posterize", "rotate", "solarize", "shear_x", "shear_y", "translate_x", "translate_y")
PRECISION_BITS = 32 - 8 - 2


# ------------------------------------------------------------------------------------------------------------- point ops
def histogram(img):
    return np.stack([np.bincount(img[..., c].ravel(), minlength=256) for c in range(3)]).astype(np.int64)


def autocontrast_lut(h):
    lut = np.arange(256, dtype=np.int64)
    nz = np.nonzero(h)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return lut.astype(np.uint8)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return np.array([min(max(int(i * scale + off), 0), 255) for i in range(256)], np.uint8)


def equalize_lut(h):
    nz = np.nonzero(h)[0]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return np.arange(256, dtype=np.uint8)
    lut, n = [], step // 2
    for i in range(256):
        lut.append(min(n // step, 255))
        n += int(h[i])
    return np.array(lut, np.uint8)


def posterize_lut(bits):
    return (np.arange(256) & (~((1 << (8 - int(bits))) - 1) & 255)).astype(np.uint8)


def solarize_lut(threshold):
    i = np.arange(256)
    return np.where(i < int(threshold), i, 255 - i).astype(np.uint8)


def apply_luts(img, luts):
    return np.stack([luts[c][img[..., c]] for c in range(3)], -1)


def autocontrast(img):
    return apply_luts(img, [autocontrast_lut(h) for h in histogram(img)])


def equalize(img):
    return apply_luts(img, [equalize_lut(h) for h in histogram(img)])


def posterize(img, bits):
    return apply_luts(img, [posterize_lut(bits)] * 3)


def solarize(img, threshold):
    return apply_luts(img, [solarize_lut(threshold)] * 3)


# --------------------------------------------------------------------------------------------------------- geometric ops
def rotate_matrix(degrees, W, H):
    theta = -math.radians(degrees % 360.0)
    m = [round(math.cos(theta), 15), round(math.sin(theta), 15), 0.0, round(-math.sin(theta), 15), round(math.cos(theta), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    x, y = -cx, -cy
    m[2] = m[0] * x + m[1] * y + m[2]
    m[5] = m[3] * x + m[4] * y + m[5]
    m[2] += cx
    m[5] += cy
    return m


def op_matrix(name, p, W, H):
    """The six doubles of a geometric op: p = signed degrees (rotate), shear (shear_*) or whole pixels (translate_*)."""
    if name == "rotate":
        return rotate_matrix(p, W, H)
    return {"shear_x": [1.0, p, 0.0, 0.0, 1.0, 0.0], "shear_y": [1.0, 0.0, 0.0, p, 1.0, 0.0],
            "translate_x": [1.0, 0.0, p, 0.0, 1.0, 0.0], "translate_y": [1.0, 0.0, 0.0, 0.0, 1.0, p]}[name]


def affine(img, m):
    """Image.transform(size, AFFINE, m, BILINEAR) with zero fill, in float64 without contraction."""
    H, W = img.shape[:2]
    a = [np.float64(v) for v in m]
    ys, xs = np.mgrid[0:H, 0:W]
    xs, ys = xs + 0.5, ys + 0.5
    xin = a[0] * xs + a[1] * ys + a[2]
    yin = a[3] * xs + a[4] * ys + a[5]
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    x0, y0 = np.floor(xin).astype(np.int64), np.floor(yin).astype(np.int64)
    dx, dy = (xin - x0)[..., None], (yin - y0)[..., None]
    xa, xb, yc = np.clip(x0, 0, W - 1), np.clip(x0 + 1, 0, W - 1), np.clip(y0, 0, H - 1)
    p = img.astype(np.float64)
    v1 = p[yc, xa] + (p[yc, xb] - p[yc, xa]) * dx
    has = ((y0 + 1 >= 0) & (y0 + 1 < H))[..., None]
    yn = np.clip(y0 + 1, 0, H - 1)
    v2 = np.where(has, p[yn, xa] + (p[yn, xb] - p[yn, xa]) * dx, v1)
    out = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    return np.where(inside[..., None], out, 0).astype(np.uint8)


def apply_op(img, name, p=None):
    if name == "autocontrast":
        return autocontrast(img)
    if name == "equalize":
        return equalize(img)
    if name == "posterize":
        return posterize(img, p)
    if name == "solarize":
        return solarize(img, p)
    return affine(img, op_matrix(name, p, img.shape[1], img.shape[0]))


# ---------------------------------------------------------------------------------------------------------------- resize
def resize_coeffs(length, out):
    """Per output index of a BILINEAR resize of `length` samples to `out`: (first tap, integer coefficients)."""
    scale = length / out
    fs = max(scale, 1.0)
    support = 1.0 * fs
    ss = 1.0 / fs
    rows = []
    for i in range(out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), length)
        w = [max(0.0, 1.0 - abs((x + xmin - center + 0.5) * ss)) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        k = [(v / ww if ww != 0.0 else v) for v in w]
        rows.append((xmin, np.array([int(0.5 + v * (1 << PRECISION_BITS)) for v in k], np.int64)))
    return rows


def _pass(img, rows, lo, n, axis):
    """One pass along `axis` of a [H, W, 3] uint8 image: outputs lo .. lo + n - 1 of the coefficient rows."""
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((n,) + a.shape[1:], np.int64)
    for j in range(n):
        x0, k = rows[lo + j]
        out[j] = np.clip(((1 << (PRECISION_BITS - 1)) + np.tensordot(k, a[x0:x0 + len(k)], 1)) >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def crop_resize(img, box, target, window, S):
    """img[box].resize(target, BILINEAR)[window : window + S]: box = (x0, y0, w, h), target = (OW, OH), window = (wx, wy).
    Horizontal pass first, 8 bits after each pass."""
    x0, y0, w, h = box
    crop = img[y0:y0 + h, x0:x0 + w]
    hor = _pass(crop, resize_coeffs(w, target[0]), window[0], S, 1)
    return _pass(hor, resize_coeffs(h, target[1]), window[1], S, 0)


def center_crop_geometry(W, H, S):
    """CenterCrop of the recipe = Resize(S) + centre crop: (box, target, window)."""
    if W <= H:
        ow, oh = S, int(S * H / W)
    else:
        oh, ow = S, int(S * W / H)
    return (0, 0, W, H), (ow, oh), (int(round((ow - S) / 2.0)), int(round((oh - S) / 2.0)))


# ------------------------------------------------------------------------------------------------------------ ColorJitter
def blend(p, d, f):
    """Pillow's Image.blend(degenerate, image, f) on uint8 planes, float32."""
    f = f32(f)
    t = (d.astype(f32) + f * (p.astype(np.int32) - d.astype(np.int32)).astype(f32)).astype(f32)
    if 0.0 <= f <= 1.0:
        return t.astype(np.int32).astype(np.uint8)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, t.astype(np.int32))).astype(np.uint8)


def luma(img):
    r, g, b = (img[..., c].astype(np.int64) for c in range(3))
    return ((19595 * r + 38470 * g + 7471 * b + 0x8000) >> 16).astype(np.uint8)


def brightness(img, f):
    return blend(img, np.zeros_like(img), f)


def saturation(img, f):
    return blend(img, np.repeat(luma(img)[..., None], 3, -1), f)


def rgb_to_hsv(img):
    r, g, b = (img[..., c].astype(np.int32) for c in range(3))
    mx, mn = np.maximum(np.maximum(r, g), b), np.minimum(np.minimum(r, g), b)
    cr = (mx - mn).astype(f32)
    crs = np.where(cr == 0, f32(1), cr)
    s = (cr / np.where(mx == 0, 1, mx).astype(f32)).astype(f32)
    rc, gc, bc = ((mx - r).astype(f32) / crs), ((mx - g).astype(f32) / crs), ((mx - b).astype(f32) / crs)
    rd, bd, gd = rc.astype(np.float64), bc.astype(np.float64), gc.astype(np.float64)
    # `bc - gc` is a float expression, `2.0 + rc - bc` a double one (the literal), both stored to a float
    h = np.where(r == mx, (bc - gc).astype(np.float64), np.where(g == mx, 2.0 + rd - bd, 4.0 + gd - rd)).astype(f32)
    h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(f32)
    uh = (h.astype(np.float64) * 255.0).astype(np.int32)
    us = (s.astype(np.float64) * 255.0).astype(np.int32)
    grey = mx == mn
    return np.stack([np.where(grey, 0, uh), np.where(grey, 0, us), mx], -1).astype(np.uint8)


def hsv_to_rgb(hsv):
    h, s, v = (hsv[..., c].astype(f32) for c in range(3))
    h6 = (h * f32(6.0) / f32(255.0)).astype(f32)
    i = np.floor(h6)
    f = (h6 - i).astype(f32)
    fs = (s / f32(255.0)).astype(f32)
    one = f32(1.0)
    rnd = lambda x: np.floor(x.astype(f32) + f32(0.5)).astype(np.int32)  # noqa: E731
    p = rnd(v * (one - fs))
    q = rnd(v * (one - fs * f))
    t = rnd(v * (one - fs * (one - f)))
    vi = v.astype(np.int32)
    sext = i.astype(np.int32) % 6
    table = [(vi, t, p), (q, vi, p), (p, vi, t), (p, q, vi), (t, p, vi), (vi, p, q)]
    out = np.zeros(hsv.shape, np.int32)
    for n, (r, g, b) in enumerate(table):
        m = sext == n
        out[..., 0][m], out[..., 1][m], out[..., 2][m] = r[m], g[m], b[m]
    grey = hsv[..., 1] == 0
    out[grey] = vi[grey][..., None]
    return np.clip(out, 0, 255).astype(np.uint8)


def hue_shift(f):
    return int(float(f) * 255) % 256  # np.uint8(f * 255): truncation, then modulo 256


def hue(img, f):
    hsv = rgb_to_hsv(img)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int32) + hue_shift(f)) % 256).astype(np.uint8)
    return hsv_to_rgb(hsv)


JITTER = {1: brightness, 2: saturation, 3: hue}  # MINK_IMG_JIT_*


# --------------------------------------------------------------------------------------------------------- a program row
def layout():
    from nerf_downstream_amd._lib import constants

    return constants("MINK_IMG_")


def run_branch(img, br, S, chain=True):
    """One branch of a program row on one image: (uint8 [S,S,3] after the flip, float32 [3,S,S] after Normalize, chain image)."""
    I = layout()
    x = img
    if chain:
        for r in range(int(br[I["B_DEPTH"]])):
            op = br[I["B_OPS"] + r * I["OP_STRIDE"]: I["B_OPS"] + (r + 1) * I["OP_STRIDE"]]
            kind = int(op[0])
            name = OPS[kind - 1]
            if name == "autocontrast" or name == "equalize":
                x = apply_op(x, name)
            elif name == "posterize" or name == "solarize":
                x = apply_op(x, name, int(op[1]))
            else:
                x = affine(x, list(op[1:7]))
    chained = x
    box = tuple(int(v) for v in br[I["B_BOX"]:I["B_BOX"] + 4])
    target = tuple(int(v) for v in br[I["B_TARGET"]:I["B_TARGET"] + 2])
    window = tuple(int(v) for v in br[I["B_WINDOW"]:I["B_WINDOW"] + 2])
    x = crop_resize(x, box, target, window, S)
    for slot in range(3):
        kind = int(br[I["B_ORDER"] + slot])
        if kind:
            x = JITTER[kind](x, br[I["B_FACTORS"] + kind - 1])
    if br[I["B_FLIP"]] != 0:
        x = x[:, ::-1]
    x = np.ascontiguousarray(x)
    t = (x.astype(f32) / f32(255.0)).astype(f32).transpose(2, 0, 1)
    t = (t + br[I["B_RGB"]:I["B_RGB"] + 3].astype(f32)[:, None, None]).astype(f32)
    t = ((t - MEAN[:, None, None]) / STD[:, None, None]).astype(f32)
    return x, t, chained


def run_program(img, row, S):
    """A whole program row: (float32 [3,S,S], stages uint8 [width+1,S,S,3], the chain images)."""
    I = layout()
    width = int(row[I["WIDTH"]])
    m = f32(row[I["M"]])
    stages, chains, pre = [], [], []
    for k in range(width + 1):
        br = row[I["BRANCH"] + k * I["BRANCH_STRIDE"]: I["BRANCH"] + (k + 1) * I["BRANCH_STRIDE"]]
        u8, t, ch = run_branch(img, br, S, chain=k > 0)
        stages.append(u8), pre.append(t), chains.append(ch)
    mix = np.zeros_like(pre[0])
    for k in range(1, width + 1):
        mix = (mix + f32(row[I["WS"] + k - 1]) * pre[k]).astype(f32)
    out = ((f32(1) - m) * pre[0] + m * mix).astype(f32)
    return out, np.stack(stages), chains


def pack(images):
    """HWC uint8 images -> (packed bytes, int64 byte offsets [B+1], int32 sizes [B,2] = (w, h))."""
    flat = [np.ascontiguousarray(im).reshape(-1) for im in images]
    offsets = np.concatenate([[0], np.cumsum([f.size for f in flat])]).astype(np.int64)
    sizes = np.array([[im.shape[1], im.shape[0]] for im in images], np.int32)
    return np.concatenate(flat), offsets, sizes
