"""Segmentation scene augmentations: the PeRFception-ScanNet recipe of the reference (configs/scannet_plenoxel.gin:
RandomRotation, RandomCrop, RandomAffine, CoordinateDropout, RandomFeatureJitter, RandomHorizontalFlip, RandomTranslation,
ElasticDistortion) as one device program per scene (include/mink_hip.h MINK_SEGAUG_*, `mink_augment_seg_scenes`).

The two stages that only segmentation uses live here, not in transforms.py, so that the CO3D datasets (which accept any
class of transforms.py that can draw) keep refusing them:

* RandomCrop (reference transforms.py:194-244) -- stage ("crop", size[3], u[max_retries, 3]);
* ElasticDistortion (:535-594) -- stage ("elastic", ((granularity, magnitude), ...)).

Differences from the reference, by design (beside the per-voxel coin dropout of transforms.py):
* RandomCrop draws all `max_retries` box corners up front (np.random.rand(max_retries, 3)) whatever the scene; the
  reference draws one np.random.rand(1, 3) per try and stops at the first non-empty box (none when the crop size covers
  the scene).  The first box is the reference's first box; the rest of the recipe sees a numpy stream advanced further.
* ElasticDistortion draws only its gate on the host; the noise grid is drawn on the device (Philox, keyed by grid node).

The colour stages of the point-cloud recipe (configs/scannet_semseg.gin: ChromaticTranslation, ChromaticJitter,
NormalizeColor) form a program of their own (MINK_COLORAUG_*, `mink_color_augment_scenes`): `PointCompose` draws every
stage in list order and splits the stages before compiling, so colour stages may sit anywhere, after ElasticDistortion
too.  ChromaticJitter draws only its gate on the host; its normals are Philox on the device, keyed by the raw point.

The ScanNet raw feature layout RandomFeatureJitter indexes is [xyzs 0:3 | dists 3 | density 4 | sh 5:32] (reference
scannet.py:623-635): RandomFeatureJitter(start_ind=4, feature_dim=27) jitters density and sh[0:26], as there."""
import random

import numpy as np

from nerf_downstream_amd import gin_lite as gin
from nerf_downstream_amd._lib import constants

from .transforms import (CoordinateDropout, CoordinateUniformTranslation, RandomAffine, RandomFeatureJitter,  # noqa: F401
                         RandomHorizontalFlip, RandomRotation, RandomScale, RandomTranslation)

SEG = constants("MINK_SEGAUG_")  # columns of a scene's parameter row, and the limits of the device program
RAW_COLUMNS = {"xyzs": [0, 1, 2], "dists": [3], "density": [4], "sh": list(range(5, 32)), "ones": [-1]}  # reference scannet.py:623-635
# |Box-Muller normal| <= sqrt(-2 ln 2^-24) = sqrt(48 ln 2) = 5.7683 (the device's u1 is at least 2^-24)
NORMAL_MAX = 5.77


def raw_columns(feature_names):
    """ScanNet raw-layout column of every selected feature column."""
    return [c for f in feature_names for c in RAW_COLUMNS[f]]


@gin.configurable()
class RandomCrop:
    def __init__(self, x, y, z, application_ratio=1, max_retries=10):
        assert x > 0 and y > 0 and z > 0
        if not 1 <= max_retries <= SEG["MAX_TRIES"]:
            raise NotImplementedError(f"RandomCrop.max_retries = {max_retries}: the device program holds 1..{SEG['MAX_TRIES']} boxes")
        self.max_size = np.array([x, y, z], np.float64)
        self.application_ratio, self.max_retries = application_ratio, int(max_retries)

    def draw(self, stages):
        if random.random() > self.application_ratio:  # (the reference's gate is `>`, transforms.py:206)
            return
        stages.append(("crop", self.max_size.copy(), np.random.rand(self.max_retries, 3)))


@gin.configurable()
class ElasticDistortion:
    def __init__(self, distortion_params=((4, 16), (8, 24)), application_ratio=0.9):
        self.distortion_params = None if distortion_params is None else tuple((float(g), float(m)) for g, m in distortion_params)
        self.application_ratio = application_ratio
        if self.distortion_params is not None:
            if len(self.distortion_params) > SEG["MAX_ELASTIC"]:
                raise NotImplementedError(f"{len(self.distortion_params)} (granularity, magnitude) pairs: the device program "
                                          f"runs at most {SEG['MAX_ELASTIC']}")
            if any(g <= 0 for g, _ in self.distortion_params):
                raise ValueError(f"granularity must be positive: {self.distortion_params}")

    def draw(self, stages):
        if self.distortion_params is not None and random.random() < self.application_ratio:
            stages.append(("elastic", self.distortion_params))


COLOR = constants("MINK_COLORAUG_")  # layout of a scene's colour program, and its op kinds
# colour stages of the reference (transforms.py) that have no device counterpart here
UNSUPPORTED_COLOR = ("ChromaticAutoContrast", "HueSaturationTranslation", "RandomDropout", "ChromaticJitterPerChannel")


@gin.configurable()
class ChromaticTranslation:
    """Reference transforms.py:43-61: with probability application_ratio, add (rand(1, 3) - 0.5) * 255 * 2 * ratio to the
    colours and clip them to [0, 255]."""

    def __init__(self, translation_range_ratio=1e-1, application_ratio=0.9):
        self.trans_range_ratio, self.application_ratio = translation_range_ratio, application_ratio

    def draw(self, ops):
        if random.random() < self.application_ratio:
            ops.append(("translate", ((np.random.rand(1, 3) - 0.5) * 255 * 2 * self.trans_range_ratio).reshape(3)))


@gin.configurable()
class ChromaticJitter:
    """Reference transforms.py:97-111: with probability application_ratio, add N(0, (std * 255)^2) to the colours and clip
    them to [0, 255].  Only the gate is drawn here; the normals are Philox on the device, keyed by the row's raw point
    (the reference draws np.random.randn(N, 3) on the host, which this stream does not)."""

    def __init__(self, std=0.01, application_ratio=0.9):
        self.std, self.application_ratio = std, application_ratio

    def draw(self, ops):
        if random.random() < self.application_ratio:
            ops.append(("jitter", self.std * 255))


@gin.configurable()
class NormalizeColor:
    """Reference transforms.py:114-122: (colours - mean) / std in float32.  Draws nothing."""

    def __init__(self, mean=(128, 128, 128), std=(256, 256, 256)):
        self.mean, self.std = np.array(mean, np.float32).reshape(3), np.array(std, np.float32).reshape(3)

    def draw(self, ops):
        ops.append(("normalize", self.mean, self.std))


COLOR_STAGES = (ChromaticTranslation, ChromaticJitter, NormalizeColor)


def compile_color_program(ops):
    """Fold one scene's drawn colour ops into a MINK_COLORAUG_* row (float64 [PARAMS]), in list order."""
    if len(ops) > COLOR["MAX_OPS"]:
        raise NotImplementedError(f"{len(ops)} colour ops in one scene: the device program holds {COLOR['MAX_OPS']}")
    P = np.zeros(COLOR["PARAMS"], np.float64)
    P[COLOR["COUNT"]] = len(ops)
    for k, op in enumerate(ops):
        o = COLOR["OPS"] + k * COLOR["OP_STRIDE"]
        if op[0] == "translate":
            P[o], P[o + 1:o + 4] = COLOR["TRANSLATE"], np.asarray(op[1], np.float64).reshape(3)
        elif op[0] == "jitter":
            P[o], P[o + 1] = COLOR["JITTER"], op[1]
        elif op[0] == "normalize":
            P[o], P[o + 1:o + 4], P[o + 4:o + 7] = COLOR["NORMALIZE"], op[1], op[2]
        else:
            raise NotImplementedError(f"colour op {op[0]!r}")
    return P


def split_color_stages(transforms):
    """-> (geometric transforms, colour transforms), each in list order.  Colour stages touch only the colour columns and
    the geometric ones only move or select rows, so the two programs commute; only the order within each is kept.
    A colour class of the reference without a device counterpart raises NotImplementedError naming it."""
    geo, col = [], []
    for t in transforms:
        name = type(t).__name__ if not isinstance(t, str) else t
        if name in UNSUPPORTED_COLOR:
            raise NotImplementedError(f"colour stage {name} has no device counterpart (supported: "
                                      f"{[c.__name__ for c in COLOR_STAGES]})")
        (col if isinstance(t, COLOR_STAGES) else geo).append(t)
    return geo, col


class PointCompose:
    """The recipe of the point-cloud dataset: every transform draws in list order, as the reference's Compose applies
    them (colour stages draw their gates and values at their place in the list), then the stages are split into the
    geometric program (a MINK_SEGAUG_* row, None without geometric stages) and the colour program (a MINK_COLORAUG_* row,
    None without colour stages)."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        geo, col = split_color_stages(self.transforms)
        self.geometric = SegCompose(geo) if geo else None
        self.color = bool(col)

    def draw(self):
        stages, ops = [], []
        for t in self.transforms:
            t.draw(ops if isinstance(t, COLOR_STAGES) else stages)
        return stages, ops

    def sample(self, extent):
        """-> (geometric row or None, colour row or None, stream id) for one scene of raw per-axis extent `extent`."""
        stages, ops = self.draw()
        geo = compile_seg_program(stages, extent) if self.geometric is not None else None
        col = compile_color_program(ops) if self.color else None
        return geo, col, int(np.random.randint(0, 2 ** 32, dtype=np.uint64))

    def __repr__(self):
        return f"PointCompose({[type(t).__name__ for t in self.transforms]})"


_KIND = {RandomRotation: "linear", RandomAffine: "linear", RandomScale: "linear", RandomTranslation: "translate",
         CoordinateUniformTranslation: "translate", RandomHorizontalFlip: "flip", CoordinateDropout: "dropout",
         RandomFeatureJitter: "feature_jitter", RandomCrop: "crop", ElasticDistortion: "elastic"}
SUPPORTED = frozenset(c.__name__ for c in _KIND)  # class names a segmentation recipe may list
_PROBE = {"linear": ("linear", np.eye(3)), "translate": ("translate", np.zeros(3)), "flip": ("flip", (0,)),
          "dropout": ("dropout", 0.0), "feature_jitter": ("feature_jitter", 0.0, 0, 0), "crop": ("crop", np.ones(3), np.zeros((1, 3))),
          "elastic": ("elastic", ())}  # one stage of every kind: the order check of a recipe, whatever its gates draw


def compile_seg_program(stages, extent=(0.0, 0.0, 0.0)):
    """Fold one scene's drawn stage list into a MINK_SEGAUG_* row (float64 [PARAMS]).  Linear / translate stages before
    the crop become (A0, a0), between the crop and the flip (A1, a1), after the flip (B, b).  `extent` is the scene's raw
    per-axis extent (max - min of its coordinates): it sizes the noise grids on the host (`grid_bounds`).

    Supported: the reference recipe, any recipe obtained by dropping its stages, and linear / translate stages anywhere
    before ElasticDistortion.  NotImplementedError: a crop after the dropout or the flip, anything after
    ElasticDistortion, a repeated crop / flip / dropout / feature jitter / elastic stage, CoordinateJitter."""
    P = np.zeros(SEG["PARAMS"], np.float64)
    M, t = [np.eye(3) for _ in range(3)], [np.zeros(3) for _ in range(3)]
    region = 0
    seen = set()
    for s in stages:
        kind = s[0]
        if "elastic" in seen:
            raise NotImplementedError(f"{kind} stage after ElasticDistortion")
        if kind in ("crop", "flip", "dropout", "feature_jitter", "elastic"):
            if kind in seen:
                raise NotImplementedError(f"more than one {kind} stage per scene")
            seen.add(kind)
        if kind == "linear":
            L = np.asarray(s[1], np.float64).reshape(3, 3)
            M[region], t[region] = M[region] @ L, t[region] @ L
        elif kind == "translate":
            t[region] = t[region] + np.asarray(s[1], np.float64).reshape(3)
        elif kind == "crop":
            if "dropout" in seen or "flip" in seen:
                raise NotImplementedError("RandomCrop after CoordinateDropout or RandomHorizontalFlip")
            size, u = np.asarray(s[1], np.float64).reshape(3), np.asarray(s[2], np.float64).reshape(-1, 3)
            if not 1 <= len(u) <= SEG["MAX_TRIES"]:
                raise NotImplementedError(f"{len(u)} crop boxes (at most {SEG['MAX_TRIES']})")
            P[SEG["CROP"]], P[SEG["CROP_SIZE"]:SEG["CROP_SIZE"] + 3], P[SEG["CROP_TRIES"]] = 1, size, len(u)
            P[SEG["CROP_U"]:SEG["CROP_U"] + u.size] = u.reshape(-1)
            region = 1
        elif kind == "flip":
            for ax in s[1]:
                P[SEG["FLIP"] + ax] = 1
            P[SEG["FLIP_ALL"]] = 0 if "dropout" in seen else 1
            region = 2
        elif kind == "dropout":
            if not 0 <= s[1] < 1:
                raise ValueError(f"dropout ratio {s[1]}")
            P[SEG["DROPOUT"]] = s[1]
        elif kind == "feature_jitter":
            if s[2] < 0 or s[3] < 0:
                raise ValueError(f"RandomFeatureJitter start_ind {s[2]} / feature_dim {s[3]}: both must be >= 0")
            P[SEG["FEAT_STD"]], P[SEG["FEAT_START"]], P[SEG["FEAT_DIM"]] = s[1], s[2], s[3]
        elif kind == "elastic":
            for e, (g, m) in enumerate(s[1]):
                P[SEG["ELASTIC"] + 2 * e], P[SEG["ELASTIC"] + 2 * e + 1] = g, m
        else:
            raise NotImplementedError(f"augmentation stage {kind!r} has no place in the segmentation program")
    for r, (Mk, ak) in enumerate((("A0", "a0"), ("A1", "a1"), ("B", "b"))):
        P[SEG[Mk]:SEG[Mk] + 9], P[SEG[ak]:SEG[ak] + 3] = M[r].reshape(-1), t[r]
    P[SEG["EXTENT"]:SEG["EXTENT"] + 3] = np.asarray(extent, np.float64).reshape(3)
    return P


def grid_bounds(params):
    """Upper bound of every elastic noise grid's dims, per scene and axis (int64 [S, 3]), from the parameter rows alone
    (no read-back): the raw extent pushed through the folded linear maps with interval arithmetic (|M|^T w), clamped by
    the crop size where a crop was drawn (a crop keeps lo < n < lo + size), a flip changing no width; a pass moves every
    point by at most NORMAL_MAX * magnitude per axis (blur and trilinear weights are non-negative and sum to at most 1),
    which widens the next pass's extent by twice that.  dim = floor(width / g) + 3, plus one for rounding.
    The bound sizes the workspace; it need not hold.  A scene whose crop keeps no box keeps its full extent and can
    exceed the clamped bound: the device then stores no grid for it and evaluates the blurred noise at each of its points
    from the Philox noise of the surrounding nodes (the same values; reported in status[1] of `mink_augment_seg_scenes`)."""
    P = np.atleast_2d(np.asarray(params, np.float64))
    out = np.zeros((len(P), 3), np.int64)
    for s, row in enumerate(P):
        w = np.abs(row[SEG["EXTENT"]:SEG["EXTENT"] + 3])
        w = np.abs(row[SEG["A0"]:SEG["A0"] + 9].reshape(3, 3)).T @ w
        if row[SEG["CROP"]]:
            w = np.minimum(w, row[SEG["CROP_SIZE"]:SEG["CROP_SIZE"] + 3])
        w = np.abs(row[SEG["A1"]:SEG["A1"] + 9].reshape(3, 3)).T @ w
        w = np.abs(row[SEG["B"]:SEG["B"] + 9].reshape(3, 3)).T @ w
        w = w * (1 + 1e-9) + 1e-6
        for e in range(SEG["MAX_ELASTIC"]):
            g, m = row[SEG["ELASTIC"] + 2 * e], row[SEG["ELASTIC"] + 2 * e + 1]
            if g > 0:
                out[s] = np.maximum(out[s], np.floor(w / g).astype(np.int64) + 4)
                w = w + 2 * NORMAL_MAX * abs(m)
    return out


def elastic_passes(params):
    """Elastic passes the batch needs (the largest number any scene drew)."""
    P = np.atleast_2d(np.asarray(params, np.float64))
    g = P[:, SEG["ELASTIC"]:SEG["ELASTIC"] + 2 * SEG["MAX_ELASTIC"]:2] > 0
    return int(max((e + 1 for e in range(g.shape[1]) if g[:, e].any()), default=0))


class SegCompose:
    """The segmentation recipe: every transform draws in list order (as the reference's Compose applies them) and the
    stage list is folded into one MINK_SEGAUG_* row.  Orders the device program cannot express are refused here, from
    the class list, whatever the gates draw."""

    def __init__(self, transforms):
        self.transforms = list(transforms)
        kinds = []
        for t in self.transforms:
            kind = _KIND.get(type(t))
            if kind is None:
                raise NotImplementedError(f"{type(t).__name__} is not part of the segmentation program (supported: "
                                          f"{sorted(c.__name__ for c in _KIND)})")
            kinds.append(_PROBE[kind])
        compile_seg_program(kinds)  # raises on an order the program cannot express

    def draw(self):
        stages = []
        for t in self.transforms:
            t.draw(stages)
        return stages

    def sample(self, extent):
        """-> (params float64 [PARAMS], stream id) for one scene of raw per-axis extent `extent`."""
        return compile_seg_program(self.draw(), extent), int(np.random.randint(0, 2 ** 32, dtype=np.uint64))

    def __repr__(self):
        return f"SegCompose({[type(t).__name__ for t in self.transforms]})"
