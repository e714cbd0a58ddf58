"""numpy restatement of the point-cloud input (include/mink_hip.h MINK_VOXDS_*, MINK_COLORAUG_*), for the tests and
scripts/scannet_pc_bench.py: ME.utils.sparse_quantize with label voting under this project's representative convention
(first row of each voxel, representatives in first-row order), and the colour ops in float64 / float32 as the reference's
transforms compute them."""
import os

import numpy as np

from nerf_downstream_amd.co3d_3d.src.data.seg_transforms import COLOR
from seg_restate import box_muller
from oracle.augment import philox4x32_10


def downsample(xyz, labels, q, voxel_size, ignore_label):
    """One scene -> (representative rows int64 [k], coordinates f32 [k,3], voted raw labels int64 [k])."""
    xyz = np.asarray(xyz, np.float32)
    labels = np.asarray(labels, np.int64)
    if q > 0:
        keys = np.floor(xyz / np.float32(q)).astype(np.int64)
        _, first, inv = np.unique(keys, axis=0, return_index=True, return_inverse=True)  # (first: first occurrence)
        order = np.argsort(first, kind="stable")
        reps = first[order]
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        u = rank[np.asarray(inv).reshape(-1)]
        lo = np.full(len(reps), np.iinfo(np.int64).max)
        hi = np.full(len(reps), np.iinfo(np.int64).min)
        np.minimum.at(lo, u, labels)
        np.maximum.at(hi, u, labels)
        voted = np.where(lo == hi, lo, ignore_label)
    else:
        reps, voted = np.arange(len(xyz)), labels.copy()
    return reps, xyz[reps] / np.float32(voxel_size), voted


def color_normals(rows, k, stream, seed):
    """float64 normals [len(rows), 3] of colour op k (Philox counter (row, k, stream, 2))."""
    w = philox4x32_10(np.asarray(rows, np.uint32), k, int(stream), 2, seed & 0xFFFFFFFF, seed >> 32)
    x, y = box_muller(w[0], w[1])
    z, _ = box_muller(w[2], w[3])
    return np.stack([x, y, z], 1)


def color_program(colors, P, rows, stream, seed):
    """The MINK_COLORAUG_* row P applied to colours f32 [k,3] whose raw rows in their scene are `rows`."""
    c = np.asarray(colors, np.float32).copy()
    for k in range(int(P[COLOR["COUNT"]])):
        op = P[COLOR["OPS"] + k * COLOR["OP_STRIDE"]:]
        if op[0] == COLOR["TRANSLATE"]:
            c = np.clip(op[1:4] + c.astype(np.float64), 0, 255).astype(np.float32)
        elif op[0] == COLOR["JITTER"]:
            c = np.clip(color_normals(rows, k, stream, seed) * op[1] + c, 0, 255).astype(np.float32)
        elif op[0] == COLOR["NORMALIZE"]:
            c = (c - op[1:4].astype(np.float32)) / op[4:7].astype(np.float32)
    return c


def synthetic_scene(rng, n, label_noise=0.05):
    """A ScanNet-shaped scene: xyz in metres over a room, colours 0..255, raw ids 0..40 shared by the points of a
    2 cm cell but for a few."""
    ext = np.array([rng.uniform(4, 8), rng.uniform(4, 8), rng.uniform(2, 3)])
    xyz = (rng.random((n, 3)) * ext - np.array([0.5, 0.5, 0.0]) * ext).astype(np.float32)
    cell = np.floor(xyz / 0.02).astype(np.int64)
    labels = (np.abs(cell[:, 0] * 7 + cell[:, 1] * 13 + cell[:, 2] * 3) // 11) % 41
    flip = rng.random(n) < label_noise
    labels[flip] = rng.integers(0, 41, int(flip.sum()))
    colors = rng.integers(0, 256, (n, 3)).astype(np.float32)
    return xyz, colors, labels.astype(np.int32)


def room_scene(rng, n_points, other_labels=0.02):
    """A ScanNet-like room sampled on SURFACES, not in a volume: a floor, three or four walls and boxes as furniture (axis-
    aligned and turned about z; top and four sides).  Points are spread over the surfaces by area, so a 2 cm voxel has the
    in-plane neighbours a scanned surface gives it.  Colours are smooth over each surface plus noise, raw labels 0..40 are
    per surface, and a fraction `other_labels` of the points carries another label."""
    X, Y, H = rng.uniform(4.5, 6.5), rng.uniform(4.0, 6.0), rng.uniform(2.4, 3.0)
    quads = [((0, 0, 0), (X, 0, 0), (0, Y, 0), 2)]  # (origin, edge u, edge v, raw label): the floor
    walls = [((0, 0, 0), (X, 0, 0)), ((0, Y, 0), (X, 0, 0)), ((0, 0, 0), (0, Y, 0)), ((X, 0, 0), (0, Y, 0))]
    for j in rng.permutation(4)[: int(rng.integers(3, 5))]:
        quads.append((walls[j][0], walls[j][1], (0, 0, H), 1))
    for _ in range(int(rng.integers(5, 9))):  # furniture
        w, d, h = rng.uniform(0.4, 1.8), rng.uniform(0.4, 1.2), rng.uniform(0.4, 1.6)
        cx, cy = rng.uniform(0.6, X - 0.6), rng.uniform(0.6, Y - 0.6)
        a = rng.uniform(0, np.pi / 2) if rng.random() < 0.5 else 0.0
        u, v = np.array([np.cos(a), np.sin(a), 0.0]), np.array([-np.sin(a), np.cos(a), 0.0])
        o = np.array([cx, cy, 0.0]) - 0.5 * w * u - 0.5 * d * v
        lab = int(rng.integers(3, 41))
        z = np.array([0.0, 0.0, h])
        quads += [(o + z, w * u, d * v, lab), (o, w * u, z, lab), (o + d * v, w * u, z, lab), (o, d * v, z, lab),
                  (o + w * u, d * v, z, lab)]
    area = np.array([np.linalg.norm(np.cross(np.asarray(q[1], float), np.asarray(q[2], float))) for q in quads])
    count = rng.multinomial(n_points, area / area.sum())
    xyz, colors, labels = [], [], []
    for (o, eu, ev, lab), k in zip(quads, count):
        st = rng.random((k, 2))
        xyz.append(np.asarray(o, float) + st[:, :1] * np.asarray(eu, float) + st[:, 1:] * np.asarray(ev, float))
        base, grad = rng.uniform(40, 215, 3), rng.uniform(-30, 30, (2, 3))
        colors.append(np.clip(base + st @ grad + rng.normal(0, 6, (k, 3)), 0, 255))
        labels.append(np.full(k, lab, np.int64))
    xyz = np.concatenate(xyz) + rng.normal(0, 0.002, (n_points, 3))  # (sensor noise off the surface)
    labels = np.concatenate(labels)
    other = rng.random(n_points) < other_labels
    labels[other] = rng.integers(0, 41, int(other.sum()))
    order = rng.permutation(n_points)
    return (xyz[order].astype(np.float32), np.concatenate(colors)[order].astype(np.float32),
            labels[order].astype(np.int32))


def write_scannet_tree(root, scenes, phase_files=("scannetv2_train.txt", "scannetv2_val.txt"), with_ext=(False, True)):
    """Write scenes [(xyz, colours, labels)] as binary PLY files under root and list them, without and with `.ply`, in the
    split files."""
    from nerf_downstream_amd.co3d_3d.src.data.ply import write_ply

    names = []
    for i, (xyz, rgb, lab) in enumerate(scenes):
        name = f"scene{i:04d}_00.ply"
        write_ply(os.path.join(root, name), [("x", xyz[:, 0]), ("y", xyz[:, 1]), ("z", xyz[:, 2]),
                                             ("red", rgb[:, 0].astype(np.uint8)), ("green", rgb[:, 1].astype(np.uint8)),
                                             ("blue", rgb[:, 2].astype(np.uint8)), ("label", lab.astype(np.uint16))])
        names.append(name)
    for f, ext in zip(phase_files, with_ext):
        with open(os.path.join(root, f), "w") as fh:
            fh.write("\n".join(n if ext else n[:-4] for n in names) + "\n")
    return names
