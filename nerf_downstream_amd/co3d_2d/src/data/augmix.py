"""AugMix for the 2-D loader (counterpart of the reference's co3d_2d/src/data/augmix.py:43-215, itself Google's AugMix).  The
workers only DRAW: which ops a chain runs and with which parameter.  The ops run on the GPU (csrc/image.hip, `mink_img_chain_round`)
on the full-size uint8 frame, every one with Pillow's arithmetic.

A drawn op is a row (kind, p0 .. p5) of the program (include/mink_hip.h, MINK_IMG_OP_*): no argument for autocontrast / equalize,
the bits kept for posterize, the threshold for solarize, and for the five geometric ops the six doubles of the affine matrix that
`Image.rotate` / `Image.transform(AFFINE)` would be handed -- the device only warps."""
import math

import numpy as np

from nerf_downstream_amd._lib import constants

IMG = constants("MINK_IMG_")


def int_parameter(level, maxval):
    return int(level * maxval / 10)


def float_parameter(level, maxval):
    return float(level) * maxval / 10.0


def sample_level(n):
    return np.random.uniform(low=0.1, high=n)


def rotate_matrix(degrees, size):
    """Image.rotate(degrees, BILINEAR) about the centre as its affine matrix (Pillow's Image.rotate: the angle modulo 360, sine and
    cosine rounded to 15 places, then the translation that keeps the centre fixed)."""
    W, H = size
    theta = -math.radians(degrees % 360.0)
    m = [round(math.cos(theta), 15), round(math.sin(theta), 15), 0.0, round(-math.sin(theta), 15), round(math.cos(theta), 15), 0.0]
    cx, cy = W / 2.0, H / 2.0
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def autocontrast(size, _):
    return (IMG["OP_AUTOCONTRAST"],)


def equalize(size, _):
    return (IMG["OP_EQUALIZE"],)


def posterize(size, level):
    level = int_parameter(sample_level(level), 4)
    return (IMG["OP_POSTERIZE"], 4 - level)


def rotate(size, level):
    degrees = int_parameter(sample_level(level), 30)
    if np.random.uniform() > 0.5:
        degrees = -degrees
    return (IMG["OP_ROTATE"], *rotate_matrix(degrees, size))


def solarize(size, level):
    level = int_parameter(sample_level(level), 256)
    return (IMG["OP_SOLARIZE"], 256 - level)


def shear_x(size, level):
    level = float_parameter(sample_level(level), 0.3)
    if np.random.uniform() > 0.5:
        level = -level
    return (IMG["OP_SHEAR_X"], 1, level, 0, 0, 1, 0)


def shear_y(size, level):
    level = float_parameter(sample_level(level), 0.3)
    if np.random.uniform() > 0.5:
        level = -level
    return (IMG["OP_SHEAR_Y"], 1, 0, 0, level, 1, 0)


def translate_x(size, level):
    level = int_parameter(sample_level(level), size[0] / 3)
    if np.random.random() > 0.5:
        level = -level
    return (IMG["OP_TRANSLATE_X"], 1, 0, level, 0, 1, 0)


def translate_y(size, level):
    level = int_parameter(sample_level(level), size[1] / 3)
    if np.random.random() > 0.5:
        level = -level
    return (IMG["OP_TRANSLATE_Y"], 1, 0, 0, 0, 1, level)


augmentations = [autocontrast, equalize, posterize, rotate, solarize, shear_x, shear_y, translate_x, translate_y]


def augment_and_mix_draw(size, recipe, severity=3, width=3, depth=-1, alpha=1.0):
    """The draws of the reference's `augment_and_mix(image, preprocess)` for an image of `size` = (W, H): the Dirichlet weights and
    the Beta coefficient as float32, per chain its ops, and one draw of `recipe` (a callable size -> branch description, see
    transforms.py) per chain and one more for the untouched image -- the reference calls `preprocess` afresh each time, so every
    branch has its own crop box, jitter, flip and lighting.  (Its further call whose result only shapes `zeros_like` is not drawn.)
    Returns {"width", "ws", "m", "branches": [branch 0 = the image, chain 1, ...]}, each chain branch with "ops"."""
    if not 1 <= width <= IMG["MAX_WIDTH"]:
        raise NotImplementedError(f"AugMix width {width}: the device program holds 1 .. {IMG['MAX_WIDTH']} chains")
    if depth > IMG["MAX_DEPTH"]:
        raise NotImplementedError(f"AugMix depth {depth}: the device program holds chains of at most {IMG['MAX_DEPTH']} ops")
    ws = np.float32(np.random.dirichlet([alpha] * width))
    m = np.float32(np.random.beta(alpha, alpha))
    chains = []
    for _ in range(width):
        d = depth if depth > 0 else np.random.randint(1, 4)
        ops = [augmentations[np.random.randint(len(augmentations))](size, severity) for _ in range(d)]
        branch = recipe(size)
        branch["ops"] = ops
        chains.append(branch)
    return {"width": width, "ws": ws, "m": m, "branches": [recipe(size)] + chains}
