"""numpy restatement of the LiDAR input (include/mink_hip.h "LiDAR scans", minkowski/utils.py prepare_lidar_batch), for the
tests and scripts/lidar_bench.py: the raw-id -> class table as the reference builds it, the decode of a scan, the voxel
down-sampling of tests/pc_restate.py on the MAPPED classes, the folded segmentation program of tests/seg_restate.py in
float64, and the finish step (the transformed metric coordinates as float features, then one float division)."""
import os

import numpy as np

from nerf_downstream_amd.co3d_3d.src.data.seg_transforms import SEG
from pc_restate import downsample
from seg_restate import canonical, row_coins

CLASS_LABELS = ("car", "bicycle", "motorcycle", "truck", "other-vehicle", "person", "bicyclist", "motorcyclist", "road", "parking",
                "sidewalk", "other-ground", "building", "fence", "vegetation", "trunk", "terrain", "pole", "traffic-sign")
STATIC = {10: "car", 11: "bicycle", 13: "bus", 15: "motorcycle", 16: "on-rails", 18: "truck", 20: "other-vehicle", 30: "person",
          31: "bicyclist", 32: "motorcyclist", 40: "road", 44: "parking", 48: "sidewalk", 49: "other-ground", 50: "building",
          51: "fence", 52: "other-structure", 60: "lane-marking", 70: "vegetation", 71: "trunk", 72: "terrain", 80: "pole",
          81: "traffic-sign", 99: "other-object"}
MOVING = {252: "car", 253: "bicyclist", 254: "person", 255: "motorcyclist", 256: "on-rails", 257: "bus", 258: "truck",
          259: "other-vehicle"}


def label_table(ignore_label=-100, size=260):
    """-> (table int64 [size], inverse int64 [size]): evaluated static ids take 0..18 in ascending id order, a moving id the
    class of its static name, every other id (named or not) `ignore_label`."""
    table, inv = np.full(size, ignore_label, np.int64), np.zeros(size, np.int64)
    for cls, raw in enumerate(sorted(r for r, name in STATIC.items() if name in CLASS_LABELS)):
        table[raw], inv[cls] = cls, raw
    by_name = {STATIC[inv[c]]: c for c in range(len(CLASS_LABELS))}
    for raw, name in MOVING.items():
        if name in by_name:
            table[raw] = by_name[name]
    return table, inv


def decode(scans, words, table, ignore_label):
    """scans [f32 [n_s,4]], words [uint32 [n_s] or None] -> (coords f32 [n,4], feats f32 [n,4], labels int64 [n], rows whose id
    the table does not hold)."""
    coords, feats, labels, bad = [], [], [], 0
    for s, (scan, w) in enumerate(zip(scans, words)):
        scan = np.asarray(scan, np.float32).reshape(-1, 4)
        ids = np.zeros(len(scan), np.int64) if w is None else (np.asarray(w).astype(np.uint32) & np.uint32(0xFFFF)).astype(np.int64)
        ok = ids < len(table)
        bad += int((~ok).sum())
        labels.append(np.where(ok, table[np.minimum(ids, len(table) - 1)], ignore_label))
        coords.append(np.concatenate([np.full((len(scan), 1), s, np.float32), scan[:, :3]], 1))
        feats.append(scan.copy())
    return np.concatenate(coords), np.concatenate(feats), np.concatenate(labels), bad


def finish(r, voxel_size):
    """r float64 [k,3] (or float32) -> (coordinates f32(r) / f32(voxel_size), xyz feature f32(r))."""
    f = np.asarray(r).astype(np.float32)
    return f / np.float32(voxel_size), f


def prepare_scene(scan, words, table, q, voxel_size, ignore_label, P=None, stream=0, seed=0):
    """One scan through the whole preparation -> (coordinates f32 [k,3], feats f32 [k,4] = xyzi, classes int64 [k], raw rows
    int64 [k]).  P: the scan's MINK_SEGAUG_* row (no elastic pass) or None."""
    _, feats, mapped, _ = decode([scan], [words], table, ignore_label)
    reps, xyz, voted = downsample(feats[:, :3], mapped, q, 1.0, ignore_label)
    if P is None:
        keep, r = np.ones(len(reps), bool), xyz
    else:
        assert not P[SEG["ELASTIC"]:SEG["ELASTIC"] + 2 * SEG["MAX_ELASTIC"]].any()
        keep, r = canonical(xyz, P, row_coins(len(reps), stream, seed))
    c, fx = finish(r, voxel_size)
    rows = reps[keep]
    return c, np.concatenate([fx, feats[rows, 3:4]], 1), voted[keep], rows


def synthetic_scan(rng, n, label_noise=0.03):
    """A KITTI-shaped scan: n returns of a ring sensor over +-80 m (negative coordinates), ground and some vertical
    structure, intensity in [0, 1); the last tenth are second returns within a centimetre of the first tenth, so that voxels
    of a few centimetres hold more than one point.  Label words: a semantic id shared by a 2 m cell but for a few (for
    three in ten of the second returns), drawn from the named ids, with a random instance id in the upper 16 bits."""
    rad = 80.0 * np.sqrt(rng.random(n))
    ang = rng.random(n) * 2 * np.pi
    z = np.where(rng.random(n) < 0.7, -1.7 + rng.normal(0, 0.03, n), rng.uniform(-1.7, 4.0, n))
    scan = np.stack([rad * np.cos(ang), rad * np.sin(ang), z, rng.random(n)], 1).astype(np.float32)
    m = n // 10
    scan[n - m:, :3] = scan[:m, :3] + rng.uniform(-0.01, 0.01, (m, 3)).astype(np.float32)
    ids = np.array(sorted(STATIC) + sorted(MOVING) + [0, 1], np.int64)
    cell = np.floor(scan[:, :2] / 2.0).astype(np.int64)
    sem = ids[np.abs(cell[:, 0] * 31 + cell[:, 1] * 17) % len(ids)]
    flip = rng.random(n) < np.where(np.arange(n) >= n - m, 0.3, label_noise)
    sem[flip] = ids[rng.integers(0, len(ids), int(flip.sum()))]
    words = (sem.astype(np.uint32) | (rng.integers(0, 1 << 16, n).astype(np.uint32) << np.uint32(16)))
    return scan, words


def write_kitti_tree(root, scans, sequences=("00", "08"), labels=True):
    """Write scans [(scan f32 [n,4], words uint32 [n])] round-robin into `<root>/dataset/sequences/<seq>/velodyne/*.bin` and
    `labels/*.label` (the sequences of every other split get an empty velodyne directory); `labels`: True, False or one
    flag per scan.  -> the relative paths written, per sequence."""
    from nerf_downstream_amd.co3d_3d.src.data.semantic_kitti import SEQUENCES

    for seq in sorted({s for v in SEQUENCES.values() for s in v}):
        os.makedirs(os.path.join(root, "dataset", "sequences", seq, "velodyne"), exist_ok=True)
    flags = [labels] * len(scans) if isinstance(labels, bool) else list(labels)
    out = {s: [] for s in sequences}
    for i, (scan, words) in enumerate(scans):
        seq = sequences[i % len(sequences)]
        base = os.path.join(root, "dataset", "sequences", seq)
        name = f"{i:06d}"
        np.asarray(scan, np.float32).tofile(os.path.join(base, "velodyne", name + ".bin"))
        if flags[i]:
            os.makedirs(os.path.join(base, "labels"), exist_ok=True)
            np.asarray(words, np.uint32).tofile(os.path.join(base, "labels", name + ".label"))
        out[seq].append(os.path.join(seq, "velodyne", name + ".bin"))
    return out


def write_s3dis_tree(root, scenes):
    """Write scenes [(xyz, colours, raw ids 0..13)] as PLY files under root, listed in stanford_{train,val,test}.txt."""
    from pc_restate import write_scannet_tree

    return write_scannet_tree(root, scenes, phase_files=("stanford_train.txt", "stanford_val.txt", "stanford_test.txt"),
                              with_ext=(False, True, True))
