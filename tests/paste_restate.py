"""numpy restatement of the background paste (the reference's BackgroundAug, co3d_2d/src/data/transforms.py:113-159): Pillow's
default `Image.resize` of a frame and its mask (BICUBIC, two passes of 8 bits), the centred rectangle, and the float64 composite
`fg * m + (1 - m) * bg` truncated to uint8.  tests/test_paste_cpu.py holds it to the recorded Pillow results of
tests/golden/bkgd_pillow_v1.npz (and to live Pillow where it imports); the GPU tests hold csrc/paste.hip to it.

Nothing here reads the library under test except the layout of the table row (`MINK_PASTE_*` of include/mink_hip.h)."""
import numpy as np

PRECISION_BITS = 32 - 8 - 2


def bicubic(x):
    """Pillow's bicubic_filter: a = -0.5, support 2."""
    a = -0.5
    if x < 0.0:
        x = -x
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def resize_coeffs(length, out):
    """Per output index of a BICUBIC resize of `length` samples to `out`: (first tap, integer coefficients).  Negative
    coefficients round half away from zero, as the positive ones do."""
    scale = length / out
    fs = max(scale, 1.0)
    support = 2.0 * fs
    ss = 1.0 / fs
    rows = []
    for i in range(out):
        center = (i + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), length)
        w = [bicubic((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        k = [(v / ww if ww != 0.0 else v) for v in w]
        rows.append((xmin, np.array([int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in k],
                                    np.int64)))
    return rows


def _pass(img, rows, axis):
    a = np.moveaxis(img.astype(np.int64), axis, 0)
    out = np.empty((len(rows),) + a.shape[1:], np.int64)
    for j, (x0, k) in enumerate(rows):
        out[j] = np.clip(((1 << (PRECISION_BITS - 1)) + np.tensordot(k, a[x0:x0 + len(k)], 1)) >> PRECISION_BITS, 0, 255)
    return np.moveaxis(out, 0, axis).astype(np.uint8)


def resize(img, size):
    """Image.resize(size) of a uint8 [H, W] or [H, W, C] image with the default filter: horizontal pass first, 8 bits after each
    pass, a pass skipped when its side does not change."""
    rw, rh = int(size[0]), int(size[1])
    H, W = img.shape[:2]
    if W != rw:
        img = _pass(img, resize_coeffs(W, rw), 1)
    if H != rh:
        img = _pass(img, resize_coeffs(H, rh), 0)
    return np.ascontiguousarray(img)


def resized_size(fg_size, s):
    """(rw, rh) of a frame of fg_size = (w, h) at scale s."""
    return int(fg_size[0] * s), int(fg_size[1] * s)


def geometry(bg_hw, rh, rw):
    """((H_start, H_end, W_start, W_end) of the rectangle in bg, (first row, first column) of the window in the resized frame)."""
    bH, bW = bg_hw
    hs, ws = max(0, (bH - rh) // 2), max(0, (bW - rw) // 2)
    he, we = min(bH, (bH + rh) // 2), min(bW, (bW + rw) // 2)
    return (hs, he, ws, we), (rh // 2 - (he - hs) // 2, rw // 2 - (we - ws) // 2)


def composite(fg_resized, mask_resized, bg):
    """The paste of an already resized frame [rh, rw, 3] through its mask plane [rh, rw] into a copy of bg."""
    rh, rw = fg_resized.shape[:2]
    (hs, he, ws, we), (y0, x0) = geometry(bg.shape[:2], rh, rw)
    m = (mask_resized / 255)[y0:y0 + (he - hs), x0:x0 + (we - ws), None]
    out = np.array(bg, dtype=np.uint8)
    out[hs:he, ws:we] = fg_resized[y0:y0 + (he - hs), x0:x0 + (we - ws)] * m + (1 - m) * out[hs:he, ws:we]
    return out


def paste(fg, mask, bg, size):
    """BackgroundAug with the drawn (rw, rh) = size: fg uint8 [h, w, 3], mask uint8 [mh, mw] (band 0), bg uint8 [H, W, 3]."""
    return composite(resize(fg, size), resize(mask, size), bg)


# ------------------------------------------------------------------------------------------------------------- a table row
def layout():
    from nerf_downstream_amd._lib import constants

    return constants("MINK_PASTE_")


def pack_paste(jobs):
    """jobs: per sample None or (fg, mask, (rw, rh)) -> (fg bytes, mask bytes, int64 table [B, MINK_PASTE_PARAMS])."""
    P = layout()
    table = np.zeros((len(jobs), P["PARAMS"]), np.int64)
    fgs, masks, fo, mo = [], [], 0, 0
    for b, job in enumerate(jobs):
        if job is None:
            continue
        fg, mask, (rw, rh) = job
        table[b, [P["FG_OFFSET"], P["MASK_OFFSET"], P["FG_W"], P["FG_H"], P["MASK_W"], P["MASK_H"], P["RW"], P["RH"]]] = [
            fo, mo, fg.shape[1], fg.shape[0], mask.shape[1], mask.shape[0], rw, rh]
        fgs.append(np.ascontiguousarray(fg).reshape(-1)), masks.append(np.ascontiguousarray(mask).reshape(-1))
        fo, mo = fo + fgs[-1].size, mo + masks[-1].size
    cat = lambda v: np.concatenate(v) if v else np.zeros(0, np.uint8)  # noqa: E731
    return cat(fgs), cat(masks), table
