"""The 2-D recipe (counterpart of the reference's co3d_2d/src/data/transforms.py, which subclasses torchvision's transforms): the
same class names, gin names and constructor arguments, but a class here only DRAWS.  `draw(branch)` adds what it drew to a branch
description (a dict that starts as {"size": (W, H)}), `compile_program` folds a sample's branches into one MINK_IMG_* program row
(include/mink_hip.h), and csrc/image.hip applies the whole batch (`minkowski.utils.prepare_image_batch`) -- as
co3d_3d/src/data/transforms.py does for point clouds.

torchvision is not a dependency.  What is said about it below is from knowledge of torchvision 0.9-0.11 and marked [tv-recall]."""
import math

import numpy as np

from nerf_downstream_amd import gin_lite as gin
from nerf_downstream_amd._lib import constants

from .augmix import augment_and_mix_draw

IMG = constants("MINK_IMG_")
# the order the device applies a branch in; a recipe is a subsequence of one of these
TRAIN_ORDER = ("RandomResizedCrop", "ColorJitter", "RandomHorizontalFlip", "ToTensor", "PCALoss", "Normalize")
EVAL_ORDER = ("CenterCrop", "ToTensor", "Normalize")


class _OnDevice:
    def __call__(self, x):
        raise RuntimeError(f"{type(self).__name__} runs on the GPU: collect draw() into a branch, fold the sample with "
                           "compile_program and hand the batch to minkowski.utils.prepare_image_batch")


class Normalize(_OnDevice):
    mean = [123.68 / 255, 116.779 / 255, 103.939 / 255]  # (the CO3D statistics the device holds as float32, not ImageNet's)
    std = [58.393 / 255, 57.12 / 255, 57.375 / 255]

    def draw(self, branch):
        branch["normalize"] = True


@gin.configurable
class ColorJitter(_OnDevice):
    """[tv-recall] ColorJitter(brightness, saturation, hue): a random order of the four slots (the contrast slot is empty), factors
    uniform in [max(0, 1 - b), 1 + b], [max(0, 1 - s), 1 + s] and [-h, h]; every step works on the 8-bit image."""

    def __init__(self, brightness=0.4, saturation=0.4, hue=0.4):
        if not 0 <= hue <= 0.5:
            raise ValueError(f"ColorJitter: hue {hue} (0 .. 0.5)")
        self.brightness, self.saturation, self.hue = float(brightness), float(saturation), float(hue)

    def draw(self, branch):
        order, factors = [], [1.0, 1.0, 0.0]
        for slot in np.random.permutation(4):  # 0 brightness, 1 contrast, 2 saturation, 3 hue
            if slot == 0 and self.brightness > 0:
                factors[0] = np.random.uniform(max(0.0, 1 - self.brightness), 1 + self.brightness)
                order.append(IMG["JIT_BRIGHTNESS"])
            elif slot == 2 and self.saturation > 0:
                factors[1] = np.random.uniform(max(0.0, 1 - self.saturation), 1 + self.saturation)
                order.append(IMG["JIT_SATURATION"])
            elif slot == 3 and self.hue > 0:
                factors[2] = np.random.uniform(-self.hue, self.hue)
                order.append(IMG["JIT_HUE"])
        branch["order"], branch["factors"] = order, factors


def center_crop_geometry(W, H, S):
    """[tv-recall] Resize(S) puts the shorter side at S and the longer at int(S * long / short); CenterCrop(S) then starts at
    int(round((len - S) / 2)).  Returns (box, target, window)."""
    if W <= H:
        ow, oh = S, int(S * H / W)
    else:
        oh, ow = S, int(S * W / H)
    return (0, 0, W, H), (ow, oh), (int(round((ow - S) / 2.0)), int(round((oh - S) / 2.0)))


@gin.configurable
class CenterCrop(_OnDevice):
    def __init__(self, image_size=224):
        self.image_size = int(image_size)

    def draw(self, branch):
        W, H = branch["size"]
        branch["box"], branch["target"], branch["window"] = center_crop_geometry(W, H, self.image_size)
        branch["S"] = self.image_size


@gin.configurable
class RandomResizedCrop(_OnDevice):
    """[tv-recall] RandomResizedCrop(image_size): scale (0.08, 1), ratio (3/4, 4/3), a log-uniform aspect, ten tries, then the
    central crop of the nearest legal aspect; the box is resized to image_size (BILINEAR, antialiased as Pillow's resize is)."""
    scale, ratio = (0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0)

    def __init__(self, image_size=(224, 224)):
        image_size = (image_size, image_size) if isinstance(image_size, int) else tuple(image_size)
        if image_size[0] != image_size[1]:
            raise NotImplementedError(f"RandomResizedCrop{image_size}: the device writes square S x S inputs")
        self.image_size = int(image_size[0])

    def get_params(self, W, H):
        area = H * W
        log_ratio = (math.log(self.ratio[0]), math.log(self.ratio[1]))
        for _ in range(10):
            target_area = area * np.random.uniform(self.scale[0], self.scale[1])
            aspect = math.exp(np.random.uniform(log_ratio[0], log_ratio[1]))
            w, h = int(round(math.sqrt(target_area * aspect))), int(round(math.sqrt(target_area / aspect)))
            if 0 < w <= W and 0 < h <= H:
                return int(np.random.randint(0, W - w + 1)), int(np.random.randint(0, H - h + 1)), w, h
        in_ratio = float(W) / float(H)
        if in_ratio < min(self.ratio):
            w = W
            h = int(round(w / min(self.ratio)))
        elif in_ratio > max(self.ratio):
            h = H
            w = int(round(h * max(self.ratio)))
        else:
            w, h = W, H
        w, h = max(1, min(w, W)), max(1, min(h, H))
        return (W - w) // 2, (H - h) // 2, w, h

    def draw(self, branch):
        S = self.image_size
        branch["box"], branch["target"], branch["window"], branch["S"] = self.get_params(*branch["size"]), (S, S), (0, 0), S


class ToTensor(_OnDevice):
    def draw(self, branch):
        branch["tensor"] = True


class Resize(_OnDevice):
    """Resize(S) alone leaves a W x H that is square only for square frames; followed by a crop it is `CenterCrop` above."""

    def __init__(self, image_size=224):
        self.image_size = int(image_size)

    def draw(self, branch):
        W, H = branch["size"]
        box, target, _ = center_crop_geometry(W, H, self.image_size)
        if target[0] != target[1]:
            raise NotImplementedError(f"Resize({self.image_size}) of a {W}x{H} frame is {target[0]}x{target[1]}: the device writes "
                                      "square inputs, use CenterCrop")
        branch["box"], branch["target"], branch["window"], branch["S"] = box, target, (0, 0), self.image_size


class RandomHorizontalFlip(_OnDevice):
    def __init__(self, p=0.5):
        self.p = p

    def draw(self, branch):
        branch["flip"] = bool(np.random.random() < self.p)


@gin.configurable
class PCALoss(_OnDevice):
    """AlexNet's PCA lighting: alpha ~ N(0, alphastd)^3, rgb[c] = sum_j eigvec[c][j] * alpha[j] * eigval[j] in float32, added to
    every pixel of channel c after ToTensor."""
    eigval = (np.array([55.46, 4.794, 1.148], np.float32) / np.float32(255.0)).astype(np.float32)
    eigvec = np.array([[-0.5675, 0.7192, 0.4009], [-0.5808, -0.0045, -0.8140], [-0.5836, -0.6948, 0.4203]], np.float32)

    def __init__(self, alphastd=0.1):
        self.alphastd = alphastd

    def draw(self, branch):
        alpha = np.random.normal(0, self.alphastd, 3).astype(np.float32)
        rgb = np.zeros(3, np.float32)
        for j in range(3):
            rgb = (rgb + (self.eigvec[:, j] * alpha[j]).astype(np.float32) * self.eigval[j]).astype(np.float32)
        branch["rgb"] = rgb


@gin.configurable
class AugMix(_OnDevice):
    def __init__(self, severity=3, width=3, depth=-1, alpha=1.0):
        self.severity, self.width, self.depth, self.alpha = severity, width, depth, alpha

    def draw(self, size, recipe):
        return augment_and_mix_draw(size, recipe, severity=self.severity, width=self.width, depth=self.depth, alpha=self.alpha)


@gin.configurable
class BackgroundAug(_OnDevice):
    """The render, resized by a random scale with Pillow's default filter, pasted through its mask over the centre of another
    scene's background (csrc/paste.hip: `mink_img_paste`).  `draw(fg_size)` is the reference's one `np.random.random()`: the
    resized size (rw, rh) of a frame of fg_size = (w, h)."""

    def __init__(self, rescale_range=(0.5, 1.5)):
        lo, hi = float(rescale_range[0]), float(rescale_range[1])
        if not 0.25 <= lo <= hi <= 4.0:
            raise ValueError(f"BackgroundAug: rescale_range {tuple(rescale_range)} (0.25 <= min <= max <= 4)")
        self.rescale_min, self.rescale_max = lo, hi

    def draw(self, fg_size):
        s = np.random.random() * (self.rescale_max - self.rescale_min) + self.rescale_min
        rw, rh = int(fg_size[0] * s), int(fg_size[1] * s)
        if rw < 1 or rh < 1:
            raise ValueError(f"BackgroundAug: a {fg_size[0]}x{fg_size[1]} frame at scale {s:.3f} has no pixels left")
        return rw, rh

    def __call__(self, fg=None, bg=None, mask=None):
        return _OnDevice.__call__(self, fg)


_BY_NAME = {c.__name__: c for c in (RandomResizedCrop, ColorJitter, RandomHorizontalFlip, ToTensor, PCALoss, Normalize, CenterCrop,
                                    Resize)}


class Compose:
    """A recipe from the reference's lists of class names (loader.py:78-81,115).  `draw(size)` is one fresh draw of every class:
    a branch description.  The device applies crop, jitter, flip, ToTensor, PCA, Normalize in that order, so the list must be
    in that order, must crop, and must end in ToTensor ... Normalize."""

    def __init__(self, names):
        names = list(names)
        unknown = [n for n in names if n not in _BY_NAME]
        if unknown:
            raise ValueError(f"unknown transformations {unknown}: {sorted(_BY_NAME)}")
        canon = [("Resize" if n == "CenterCrop" and "Resize" in names else n) for n in
                 (TRAIN_ORDER if "RandomResizedCrop" in names else EVAL_ORDER)]
        it = iter(canon)
        if not all(n in it for n in names) or names[0] != canon[0] or "ToTensor" not in names or "Normalize" not in names:
            raise NotImplementedError(f"recipe {names}: the device applies {canon} in this order; a recipe is a sub-list that starts "
                                      "with the crop and holds ToTensor and Normalize")
        self.names, self.transforms = names, [_BY_NAME[n]() for n in names]

    def draw(self, size):
        branch = {"size": (int(size[0]), int(size[1]))}
        for t in self.transforms:
            t.draw(branch)
        return branch

    __call__ = _OnDevice.__call__


def compile_program(sample):
    """One sample's draws -> its program row, float64 [MINK_IMG_PARAMS].  `sample` is what `augment_and_mix_draw` returns, or a
    single branch description (evaluation: width 0, out = pre_0)."""
    if "branches" not in sample:
        sample = {"width": 0, "ws": [], "m": 0.0, "branches": [sample]}
    P = np.zeros(IMG["PARAMS"], np.float64)
    width = int(sample["width"])
    if len(sample["branches"]) != width + 1 or not 0 <= width <= IMG["MAX_WIDTH"]:
        raise ValueError(f"{len(sample['branches'])} branches for width {width} (width + 1, width <= {IMG['MAX_WIDTH']})")
    P[IMG["WIDTH"]], P[IMG["M"]] = width, np.float32(sample["m"])
    P[IMG["WS"]:IMG["WS"] + width] = np.asarray(sample["ws"], np.float32)
    sizes = {b["S"] for b in sample["branches"]}
    if len(sizes) != 1:
        raise ValueError(f"branches of output sizes {sorted(sizes)} in one sample")
    for k, b in enumerate(sample["branches"]):
        o = IMG["BRANCH"] + k * IMG["BRANCH_STRIDE"]
        ops = b.get("ops", []) if k else []
        if len(ops) > IMG["MAX_DEPTH"]:
            raise ValueError(f"a chain of {len(ops)} ops (at most {IMG['MAX_DEPTH']})")
        P[o + IMG["B_DEPTH"]] = len(ops)
        for r, op in enumerate(ops):
            P[o + IMG["B_OPS"] + r * IMG["OP_STRIDE"]: o + IMG["B_OPS"] + r * IMG["OP_STRIDE"] + len(op)] = op
        W, H = b["size"]
        x0, y0, w, h = b["box"]
        S = b["S"]
        if not (0 <= x0 and 0 <= y0 and w >= 1 and h >= 1 and x0 + w <= W and y0 + h <= H):
            raise ValueError(f"crop box {b['box']} outside the {W}x{H} frame")
        if not (b["window"][0] >= 0 and b["window"][1] >= 0 and b["window"][0] + S <= b["target"][0] and b["window"][1] + S <= b["target"][1]):
            raise ValueError(f"window {b['window']} + {S} outside the resized {b['target']}")
        P[o + IMG["B_BOX"]:o + IMG["B_BOX"] + 4] = b["box"]
        P[o + IMG["B_TARGET"]:o + IMG["B_TARGET"] + 2] = b["target"]
        P[o + IMG["B_WINDOW"]:o + IMG["B_WINDOW"] + 2] = b["window"]
        order = list(b.get("order", []))
        P[o + IMG["B_ORDER"]:o + IMG["B_ORDER"] + len(order)] = order
        P[o + IMG["B_FACTORS"]:o + IMG["B_FACTORS"] + 3] = b.get("factors", [1.0, 1.0, 0.0])
        P[o + IMG["B_FLIP"]] = 1.0 if b.get("flip") else 0.0
        P[o + IMG["B_RGB"]:o + IMG["B_RGB"] + 3] = np.asarray(b.get("rgb", np.zeros(3)), np.float32)
    return P
