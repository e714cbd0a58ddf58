"""ME.utils subset.  Runs in DataLoader worker processes (reference data_module.py:54-65), so it
is pure-CPU torch and must never touch HIP."""
import ctypes

import numpy as np
import torch


def _t(a):
    return torch.from_numpy(a) if isinstance(a, np.ndarray) else a


def batched_coordinates(coords, dtype=torch.int32, device=None):
    n = [int(c.shape[0]) for c in coords]
    D = int(coords[0].shape[1])
    out = torch.zeros(sum(n), D + 1, dtype=dtype, device=device)
    s = 0
    for j, c in enumerate(coords):
        out[s : s + n[j], 1:] = _t(c).to(dtype)
        out[s : s + n[j], 0] = j
        s += n[j]
    return out


def sparse_collate(coords, feats, labels=None, dtype=torch.int32, device=None):
    """A11 (reference data/utils.py:25-30): concatenate per-sample coordinates with the batch
    index in column 0 and concatenate the features; labels (if given) are concatenated too."""
    bcoords = batched_coordinates(coords, dtype=dtype, device=device)
    bfeats = torch.cat([_t(f) for f in feats], 0)
    if labels is None:
        return bcoords, bfeats
    return bcoords, bfeats, torch.cat([_t(l) for l in labels], 0)


def decode_plenoxel_batch(batch, reso=None):
    """Compact PeRFception `data.npz` batch (device tensors: links, density, sh_q, scene_offsets,
    sh_scale, sh_min + `feature_names`) -> (coordinates int32 [N,4], features f32 [N,C]) with one
    HIP kernel (`mink_decode_plenoxel`; reference co3d.py:160-166,196-229)."""
    import torch

    from .._lib import check, lib

    links = batch["links"]
    if not links.is_cuda:
        raise RuntimeError("decode_plenoxel_batch runs on the GPU: move the batch to cuda first")
    reso = tuple(reso or batch.get("reso") or (128, 128, 128))  # data.npz: 128^3; last.ckpt scenes: 256^3
    names = list(batch["feature_names"])
    width = {"density": 1, "sh": 27, "ones": 1, "xyzs": 3}
    col, C = {"density": -1, "sh": -1, "ones": -1, "xyzs": -1}, 0
    for f in names:
        if f not in width or col[f] >= 0:
            raise ValueError(f"feature {f!r} cannot be decoded on the GPU (supported once each: xyzs, density, sh, ones)")
        col[f] = C
        C += width[f]
    n = links.shape[0]
    coords = torch.empty(n, 4, dtype=torch.int32, device=links.device)
    feats = torch.empty(n, C, dtype=torch.float32, device=links.device)
    n_scenes = batch["scene_offsets"].numel() - 1
    scratch = torch.empty(n_scenes, dtype=torch.float32, device=links.device) if col["xyzs"] >= 0 else None  # per-scene max norm
    stream = torch._C._cuda_getCurrentRawStream(links.device.index)
    check(
        lib().mink_decode_plenoxel(
            links.data_ptr(), batch["density"].data_ptr(), batch["sh_q"].data_ptr(), batch["scene_offsets"].data_ptr(),
            batch["scene_offsets"].numel() - 1, batch["sh_scale"].data_ptr(), batch["sh_min"].data_ptr(), n, reso[1], reso[2],
            col["density"], col["sh"], col["ones"], col["xyzs"], None if scratch is None else scratch.data_ptr(), C,
            coords.data_ptr(), feats.data_ptr(), C, stream,
        )
    )
    return coords, feats


def augment_batch(coords, feats, scene_offsets, params, streams, seed, raw_cols, count_async=False):
    """Apply the drawn per-scene augmentation programs to a whole batch with `mink_augment_scenes`
    (reference transforms.py, applied per scene on the CPU at co3d.py:216-219).

    coords int32/f32 [N,4] (batch,x,y,z) sorted by batch, feats f32 [N,C], scene_offsets int32 [S+1],
    params f32 [S, MINK_AUG_PARAMS], streams int32 [S] (uint32 bits) -- all on the device; `raw_cols`
    a host list (transforms.raw_columns).  Returns float coordinates and features of the surviving
    voxels.  The survivor count is read back (one small synchronisation of the current stream) unless
    `params` is a host tensor whose DROPOUT column is all zero (then every voxel survives).
    `count_async=True` never blocks: it returns (coords, feats, pending) with full-length buffers and
    pending = None or (pinned int32 count, event recorded after its copy) for the caller to slice later."""
    import torch

    from .._lib import check, lib
    from ..co3d_3d.src.data.transforms import AUG

    if not coords.is_cuda:
        raise RuntimeError("augment_batch runs on the GPU: move the batch to cuda first")
    n, C = coords.shape[0], feats.shape[1]
    dev = coords.device
    if coords.dtype not in (torch.int32, torch.float32) or feats.dtype != torch.float32:
        raise TypeError("augment_batch: coordinates int32 or float32, features float32")
    coords, feats = coords.contiguous(), feats.contiguous()
    host_params = params if not params.is_cuda else None
    params = params.to(dev, torch.float32, non_blocking=True).contiguous()
    out_c = torch.empty(n, 4, dtype=torch.float32, device=dev)
    out_f = torch.empty(n, C, dtype=torch.float32, device=dev)
    kept = torch.empty(1, dtype=torch.int32, device=dev)
    n_scenes = scene_offsets.numel() - 1
    offs = scene_offsets.to(dev, torch.int32, non_blocking=True).contiguous()
    strm = streams.to(dev, torch.int32, non_blocking=True).contiguous()
    ws = torch.empty(max(1, lib().mink_augment_workspace_bytes(n, n_scenes)), dtype=torch.uint8, device=dev)
    cols = (ctypes.c_int32 * C)(*[int(c) for c in raw_cols])
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    check(
        lib().mink_augment_scenes(
            coords.data_ptr(), int(coords.dtype == torch.int32), feats.data_ptr(), C, C, n,
            offs.data_ptr(), n_scenes, params.data_ptr(), strm.data_ptr(),
            int(seed) & (2 ** 64 - 1), ctypes.cast(cols, ctypes.c_void_p), out_c.data_ptr(), out_f.data_ptr(), C,
            kept.data_ptr(), ws.data_ptr(), ws.numel(), stream,
        )
    )
    # without dropout every voxel survives and the count is known on the host
    if host_params is not None and not bool((host_params[:, AUG["DROPOUT"]] != 0).any()):
        return (out_c, out_f, None) if count_async else (out_c, out_f)
    if count_async:
        count = torch.empty(1, dtype=torch.int32, pin_memory=True)
        count.copy_(kept, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return out_c, out_f, (count, ev)
    k = int(kept.item())
    return out_c[:k], out_f[:k]


class AugmentBoundError(RuntimeError):
    """An elastic noise grid of `mink_augment_seg_scenes` has more than 65535 nodes along an axis (or a NaN extent):
    its nodes cannot be keyed, and the pass was not applied to that scene."""


def seg_status_check(status):
    """Raise if the device reported elastic passes it could not apply (status = host int32 [survivors, passes evaluated
    without a stored grid, passes not applied]).  A grid over its host-side bound is not an error: the device evaluates
    it point by point (status[1], informational)."""
    if int(status[2]) != 0:
        raise AugmentBoundError(f"augment_seg_batch: {int(status[2])} elastic noise grid(s) with more than 65535 nodes along "
                                "an axis (or a non-finite extent): the pass was not applied to those scenes")


def augment_seg_batch(coords, feats, scene_offsets, params, streams, seed, raw_cols, count_async=False, grid_bound=None):
    """Apply the drawn segmentation programs (data/seg_transforms.py, include/mink_hip.h MINK_SEGAUG_*) to a whole batch
    with `mink_augment_seg_scenes`.

    coords int32/f32 [N,4] sorted by batch, feats f32 [N,C], scene_offsets int32 [S+1], streams int32 [S] on the device;
    params float64 [S, MINK_SEGAUG_PARAMS] on the HOST (its EXTENT columns size the noise grids: `grid_bounds`; a device
    tensor is copied back first).  `grid_bound` int [S,3] replaces the computed bound.  Returns float coordinates,
    features and the int32 source row of every survivor; the survivor count and the status are read back (one small
    synchronisation) unless `count_async=True`, which returns (coords, feats, rows, (pinned int32 [3] status, event)) with
    full-length buffers for the caller to slice once the event has completed (`seg_status_check` on the status)."""
    import torch

    out_c, out_f, rows, status = _augment_seg_launch(coords, feats, scene_offsets, params, streams, seed, raw_cols, grid_bound)
    if count_async:
        host = torch.empty(3, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return out_c, out_f, rows, (host, ev)
    st = status.cpu()
    seg_status_check(st)
    k = int(st[0])
    return out_c[:k], out_f[:k], rows[:k]


def _augment_seg_launch(coords, feats, scene_offsets, params, streams, seed, raw_cols, grid_bound=None):
    """`mink_augment_seg_scenes` on the current stream -> full-length (coords, feats, rows) and the device status int32 [3]."""
    import torch

    from .._lib import check, lib
    from ..co3d_3d.src.data.seg_transforms import SEG, elastic_passes, grid_bounds

    if not coords.is_cuda:
        raise RuntimeError("augment_seg_batch runs on the GPU: move the batch to cuda first")
    n, C = coords.shape[0], feats.shape[1]
    dev = coords.device
    if coords.dtype not in (torch.int32, torch.float32) or feats.dtype != torch.float32:
        raise TypeError("augment_seg_batch: coordinates int32 or float32, features float32")
    coords, feats = coords.contiguous(), feats.contiguous()
    n_scenes = scene_offsets.numel() - 1
    P = params.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(params) else np.array(params, np.float64)
    if P.shape != (n_scenes, SEG["PARAMS"]):
        raise ValueError(f"augment_seg_batch: parameter rows {P.shape}, ({n_scenes}, {SEG['PARAMS']}) expected")
    bound = grid_bounds(P) if grid_bound is None else np.asarray(grid_bound, np.int64).reshape(n_scenes, 3)
    P[:, SEG["GRID_BOUND"]:SEG["GRID_BOUND"] + 3] = bound
    grid_nodes = int(np.prod(bound, axis=1).sum())
    n_elastic = elastic_passes(P)
    dparams = torch.from_numpy(P).pin_memory().to(dev, non_blocking=True)
    out_c = torch.empty(n, 4, dtype=torch.float32, device=dev)
    out_f = torch.empty(n, C, dtype=torch.float32, device=dev)
    rows = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(3, dtype=torch.int32, device=dev)
    offs = scene_offsets.to(dev, torch.int32, non_blocking=True).contiguous()
    strm = streams.to(dev, torch.int32, non_blocking=True).contiguous()
    ws = torch.empty(max(1, lib().mink_augment_seg_workspace_bytes(n, n_scenes, grid_nodes)), dtype=torch.uint8, device=dev)
    cols = (ctypes.c_int32 * C)(*[int(c) for c in raw_cols])
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    check(
        lib().mink_augment_seg_scenes(
            coords.data_ptr(), int(coords.dtype == torch.int32), feats.data_ptr(), C, C, n, offs.data_ptr(), n_scenes,
            dparams.data_ptr(), strm.data_ptr(), int(seed) & (2 ** 64 - 1), ctypes.cast(cols, ctypes.c_void_p), n_elastic,
            grid_nodes, out_c.data_ptr(), out_f.data_ptr(), C, rows.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(),
            stream,
        )
    )
    return out_c, out_f, rows, status


class VoxelRangeError(RuntimeError):
    """A voxel key of `mink_voxel_downsample_scenes` fell outside the packable range (|floor(xyz / q)| > 32767)."""


def points_status_check(status):
    """Raise on a failed point-cloud preparation (status = host int32 [survivors, elastic passes evaluated without a stored
    grid, elastic passes not applied, MINK_STATUS_* bits of the down-sampling])."""
    from .._lib import CONSTANTS

    seg_status_check(status)
    if int(status[3]) & CONSTANTS["MINK_STATUS_RANGE"]:
        raise VoxelRangeError("voxel_downsample: a voxel key outside [-32768, 32767] (coordinates / quantisation size too large)")


def voxel_downsample_batch(coords, feats, labels, scene_offsets, params):
    """`mink_voxel_downsample_scenes` (include/mink_hip.h MINK_VOXDS_*) on the current stream: ME.utils.sparse_quantize with
    label voting, per scene.  coords f32 [N,4] (batch, x, y, z) sorted by batch, feats f32 [N,C], labels int [N],
    scene_offsets int32 [S+1], params float64 [S, MINK_VOXDS_PARAMS], all on the device.  Nothing is read back: returns
    full-length (coords f32 [N,4], feats [N,C], voted raw labels int32 [N], input row int32 [N] of every representative,
    scene row ranges int32 [S+2] (the last range is the unused tail), device status int32 [2] = (representatives,
    MINK_STATUS_* bits))."""
    import torch

    from .._lib import check, constants, lib

    if not coords.is_cuda:
        raise RuntimeError("voxel_downsample_batch runs on the GPU: move the batch to cuda first")
    if coords.dtype != torch.float32 or feats.dtype != torch.float32:
        raise TypeError("voxel_downsample_batch: float32 coordinates and features")
    dev, n, C = coords.device, coords.shape[0], feats.shape[1]
    n_scenes = scene_offsets.numel() - 1
    coords, feats = coords.contiguous(), feats.contiguous()
    labels = labels.to(dev, torch.int32).contiguous()
    offs = scene_offsets.to(dev, torch.int32).contiguous()
    P = params.to(dev, torch.float64).contiguous()
    width = constants("MINK_VOXDS_")["PARAMS"]
    if P.shape != (n_scenes, width):
        raise ValueError(f"voxel_downsample_batch: parameter rows {tuple(P.shape)}, ({n_scenes}, {width}) expected")
    out_c = torch.empty(n, 4, dtype=torch.float32, device=dev)
    out_f = torch.empty(n, C, dtype=torch.float32, device=dev)
    out_l = torch.empty(n, dtype=torch.int32, device=dev)
    rows = torch.empty(n, dtype=torch.int32, device=dev)
    out_offs = torch.empty(n_scenes + 2, dtype=torch.int32, device=dev)
    status = torch.empty(2, dtype=torch.int32, device=dev)
    ws = torch.empty(lib().mink_voxel_downsample_workspace_bytes(n), dtype=torch.uint8, device=dev)
    check(
        lib().mink_voxel_downsample_scenes(
            coords.data_ptr(), feats.data_ptr(), C, C, labels.data_ptr(), n, offs.data_ptr(), n_scenes, P.data_ptr(),
            out_c.data_ptr(), out_f.data_ptr(), C, out_l.data_ptr(), rows.data_ptr(), out_offs.data_ptr(), status.data_ptr(),
            ws.data_ptr(), ws.numel(), torch._C._cuda_getCurrentRawStream(dev.index),
        )
    )
    return out_c, out_f, out_l, rows, out_offs, status


def color_augment_batch(feats, scene_offsets, params, streams, seed, key_rows, key_offsets, cols=(0, 1, 2)):
    """`mink_color_augment_scenes` (MINK_COLORAUG_*) IN PLACE on the colour columns `cols` of feats f32 [N,C], rows
    [0, scene_offsets[S]); params float64 [S, MINK_COLORAUG_PARAMS], streams int32 [S]; the jitter of row i in scene b is
    keyed by key_rows[i] - key_offsets[b].  All on the device; returns feats."""
    import torch

    from .._lib import check, lib

    if not feats.is_cuda or feats.dtype != torch.float32 or not feats.is_contiguous():
        raise TypeError("color_augment_batch: contiguous float32 features on the GPU")
    dev, n = feats.device, feats.shape[0]
    n_scenes = params.shape[0]
    P = params.to(dev, torch.float64).contiguous()
    offs = scene_offsets.to(dev, torch.int32).contiguous()
    if offs.numel() < n_scenes + 1:
        raise ValueError(f"color_augment_batch: {offs.numel()} scene offsets for {n_scenes} scenes")
    strm = streams.to(dev, torch.int32).contiguous()
    krows, koffs = key_rows.to(dev, torch.int32).contiguous(), key_offsets.to(dev, torch.int32).contiguous()
    c = (ctypes.c_int32 * 3)(*[int(x) for x in cols])
    check(
        lib().mink_color_augment_scenes(
            feats.data_ptr(), feats.shape[1], ctypes.cast(c, ctypes.c_void_p), n, offs.data_ptr(), n_scenes, P.data_ptr(),
            strm.data_ptr(), int(seed) & (2 ** 64 - 1), krows.data_ptr(), koffs.data_ptr(),
            torch._C._cuda_getCurrentRawStream(dev.index),
        )
    )
    return feats


def prepare_point_batch(batch, count_async=False):
    """The point-cloud input of a batch of ScannetDataset (data/scannet.py), on the current stream: voxel down-sampling with
    label voting, the colour programs, then the geometric programs (MINK_SEGAUG_*) when the loader drew them.  Colour ops
    touch only colour columns and their noise is keyed by the raw row of the representative, so they commute with the
    geometric stages, which only move or select rows: they run first, on the representatives.

    batch (device): coordinates f32 [N,4] (metres), features f32 [N,3] (colours), labels int [N] (raw), scene_offsets int32
    [S+1], ds_params f64 [S, MINK_VOXDS_PARAMS], class_lut int [NUM_LABELS] (raw label -> class); optional color_params f64
    [S, MINK_COLORAUG_PARAMS], aug_params f64 [S, MINK_SEGAUG_PARAMS] (host), aug_streams, aug_seed.
    Returns (coords f32 [k,4], feats f32 [k,3], labels int64 [k] (classes), raw row int32 [k] of every row); with
    `count_async=True` full-length buffers and (pinned host status int32 [4], event) instead, for the caller to slice
    (`points_status_check` on the status).  Rows past the representatives run through the geometric program as one more
    scene whose dropout ratio (2) removes every row."""
    import torch

    from .._lib import constants
    from ..co3d_3d.src.data.seg_transforms import SEG

    coords, feats = batch["coordinates"], batch["features"]
    if not coords.is_cuda:
        raise RuntimeError("the point-cloud input is prepared on the GPU: move the batch to cuda first")
    n, dev = coords.shape[0], coords.device
    offs = batch["scene_offsets"].to(dev, torch.int32)
    n_scenes = offs.numel() - 1
    c, f, raw, src, ds_offs, ds_status = voxel_downsample_batch(coords.float(), feats.float(), batch["labels"], offs, batch["ds_params"])
    lut = batch["class_lut"].to(dev, torch.int64)
    ignore = batch["ds_params"][0, constants("MINK_VOXDS_")["IGNORE"]]
    raw = raw.long()
    labels = torch.where((raw >= 0) & (raw < lut.numel()), lut[raw.clamp(0, lut.numel() - 1)], ignore.to(dev, torch.int64))
    if "color_params" in batch:
        color_augment_batch(f, ds_offs, batch["color_params"], batch["aug_streams"], batch["aug_seed"], src, offs)
    status = torch.zeros(4, dtype=torch.int32, device=dev)
    status[3:] = ds_status[1:]
    if "aug_params" in batch:
        P = batch["aug_params"].detach().cpu().numpy().astype(np.float64) if torch.is_tensor(batch["aug_params"]) else np.array(batch["aug_params"], np.float64)
        sink = np.zeros((1, SEG["PARAMS"]), np.float64)
        for M in ("A0", "A1", "B"):
            sink[0, SEG[M]:SEG[M] + 9] = np.eye(3).reshape(-1)
        sink[0, SEG["DROPOUT"]] = 2.0  # (coins are < 1: the tail past the representatives is dropped)
        streams = torch.cat([batch["aug_streams"].to(dev, torch.int32), torch.zeros(1, dtype=torch.int32, device=dev)])
        c, f, rows, seg_status = _augment_seg_launch(c, f, ds_offs, np.concatenate([P, sink]), streams, batch["aug_seed"],
                                                     [-1] * f.shape[1])
        rows = rows.long().clamp_(0, max(n - 1, 0))  # (rows past the survivors are not written: any index will do there)
        labels, src = labels[rows], src[rows]
        status[:3] = seg_status
    else:
        status[0] = ds_status[0]
    if count_async:
        host = torch.empty(4, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return c, f, labels, src, (host, ev)
    st = status.cpu()
    points_status_check(st)
    k = int(st[0])
    return c[:k], f[:k], labels[:k], src[:k]


class LidarLabelError(RuntimeError):
    """A raw label word of `mink_lidar_decode_scans` carries a semantic id (its low 16 bits) past the end of the table."""


def lidar_status_check(status):
    """Raise on the status word of `mink_lidar_decode_scans` (a host int or a one-element tensor): the number of rows whose
    semantic id the table does not hold.  The reference's `label_map[all_labels & 0xFFFF]` raises an IndexError there."""
    s = int(status)
    if s:
        raise LidarLabelError(f"lidar_decode: {s} raw label word(s) with a semantic id past the end of the label table "
                              "(those rows got the ignore label)")


def lidar_decode_batch(scan, raw_labels, scene_offsets, lut, ignore_label):
    """`mink_lidar_decode_scans` on the current stream: scan f32 [n,4] (x, y, z, intensity: the .bin file), raw_labels int32 /
    uint32 words [n] or None (no .label file: every word 0), scene_offsets int32 [S+1], lut int [lut_size], all on the device.
    Nothing is read back: returns (coords f32 [n,4] = (scene, x, y, z), feats f32 [n,4] = xyzi, labels
    int32 [n] = lut[word & 0xFFFF], device status int32 [1] for `lidar_status_check`)."""
    import torch

    from .._lib import check, lib

    if not scan.is_cuda:
        raise RuntimeError("lidar_decode_batch runs on the GPU: move the batch to cuda first")
    if scan.dtype != torch.float32 or scan.dim() != 2 or scan.shape[1] != 4:
        raise TypeError(f"lidar_decode_batch: scan of shape {tuple(scan.shape)} {scan.dtype}, float32 [n, 4] expected")
    dev, n = scan.device, scan.shape[0]
    scan = scan.contiguous()
    if raw_labels is not None:
        if raw_labels.dtype not in (torch.int32, getattr(torch, "uint32", torch.int32)) or raw_labels.numel() != n:
            raise TypeError(f"lidar_decode_batch: {raw_labels.numel()} label words of {raw_labels.dtype} for {n} points (32-bit words)")
        raw_labels = raw_labels.to(dev).contiguous()
    offs = scene_offsets.to(dev, torch.int32).contiguous()
    table = lut.to(dev, torch.int32).contiguous()
    coords = torch.empty(n, 4, dtype=torch.float32, device=dev)
    feats = torch.empty(n, 4, dtype=torch.float32, device=dev)
    labels = torch.empty(n, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    check(
        lib().mink_lidar_decode_scans(
            scan.data_ptr(), None if raw_labels is None else raw_labels.data_ptr(), n, offs.data_ptr(), offs.numel() - 1,
            table.data_ptr(), table.numel(), int(ignore_label), coords.data_ptr(), feats.data_ptr(), 4, labels.data_ptr(),
            status.data_ptr(), torch._C._cuda_getCurrentRawStream(dev.index),
        )
    )
    return coords, feats, labels, status


def lidar_finish_rows(coords, feats, n_rows, voxel_size):
    """`mink_lidar_finish_rows` IN PLACE on the current stream: for every row below the DEVICE int32 count `n_rows` (a
    one-element tensor or view), feats[:, 0:3] = coords[:, 1:4] and coords[:, 1:4] /= f32(voxel_size).  Returns (coords, feats)."""
    import torch

    from .._lib import check, lib

    if not (coords.is_cuda and coords.dtype == torch.float32 and coords.is_contiguous() and coords.dim() == 2 and coords.shape[1] == 4):
        raise TypeError("lidar_finish_rows: contiguous float32 coordinates [n, 4] on the GPU")
    if not (feats.is_cuda and feats.dtype == torch.float32 and feats.is_contiguous() and feats.shape[0] == coords.shape[0]):
        raise TypeError("lidar_finish_rows: contiguous float32 features on the GPU, one row per coordinate row")
    if not (n_rows.is_cuda and n_rows.dtype == torch.int32 and n_rows.numel() == 1):
        raise TypeError("lidar_finish_rows: the row count is one int32 on the device")
    check(lib().mink_lidar_finish_rows(coords.data_ptr(), coords.shape[0], n_rows.data_ptr(), float(voxel_size), feats.data_ptr(),
                                       feats.shape[1], 0, torch._C._cuda_getCurrentRawStream(coords.device.index)))
    return coords, feats


def lidar_batch_status_check(status):
    """Raise on a failed LiDAR preparation (status = host int32 [survivors, elastic passes evaluated without a stored grid,
    elastic passes not applied, MINK_STATUS_* bits of the down-sampling, label words outside the table])."""
    points_status_check(status[:4])
    lidar_status_check(status[4])


def prepare_lidar_batch(batch, count_async=False):
    """The input of a batch of SemanticKITTIDataset (data/semantic_kitti.py), on the current stream, in the reference's order
    (semantic_kitti.py:183-209): the label table (`mink_lidar_decode_scans`), voxel down-sampling with the vote over the
    MAPPED classes (`mink_voxel_downsample_scenes`, VOXEL = 1: the coordinates stay in metres), the drawn geometric program
    (MINK_SEGAUG_*, in metres) when there is one, then `mink_lidar_finish_rows`: the transformed coordinates become the xyz
    of the `xyzi` feature and are divided by the voxel size.

    batch (device): scan f32 [N,4], raw_labels int32 [N] (absent: no scan had a .label file), scene_offsets int32 [S+1],
    label_lut int [lut_size]; on the HOST lidar_params f64 [S,3] (numpy) = (down-sampling voxel size, voxel size, ignore label;
    one voxel size and ignore label per batch) and the optional aug_params f64 [S, MINK_SEGAUG_PARAMS]; aug_streams, aug_seed.
    Nothing is read back from the device before the status word: with `count_async=True` the call never blocks.
    Returns (coords f32 [k,4], feats f32 [k,4] = xyzi, labels int64 [k] (classes), raw row int32 [k]); with `count_async=True`
    full-length buffers and (pinned host status int32 [5], event) instead, for the caller to slice (`lidar_batch_status_check`
    on the status).  Rows past the representatives run through the geometric program as one more scene whose dropout ratio
    (2) removes every row, as in `prepare_point_batch`.  A semantic id the table does not hold raises `LidarLabelError`."""
    import torch

    from .._lib import constants
    from ..co3d_3d.src.data.seg_transforms import SEG

    feature_names = list(batch.get("feature_names") or ["xyzi"])
    if feature_names != ["xyzi"]:
        raise NotImplementedError(f"features {feature_names}: the LiDAR preparation produces ['xyzi']")
    scan = batch["scan"]
    if not scan.is_cuda:
        raise RuntimeError("the LiDAR input is prepared on the GPU: move the batch to cuda first")
    n, dev = scan.shape[0], scan.device
    offs = batch["scene_offsets"].to(dev, torch.int32)
    n_scenes = offs.numel() - 1
    lp = batch["lidar_params"]
    if torch.is_tensor(lp):
        if lp.is_cuda:  # (a read-back here would stall the host behind the batch's copies: what the deferred count exists to avoid)
            raise TypeError("prepare_lidar_batch: lidar_params are host values (a numpy array or a CPU tensor), not a device tensor")
        lp = lp.detach().numpy()
    lp = np.asarray(lp, np.float64).reshape(n_scenes, 3)
    voxel_size, ignore = float(lp[0, 1]), int(lp[0, 2])
    if not ((lp[:, 1] == lp[0, 1]).all() and (lp[:, 2] == lp[0, 2]).all()):
        raise ValueError("prepare_lidar_batch: one voxel size and one ignore label per batch")
    c, f, mapped, lut_status = lidar_decode_batch(scan.float(), batch.get("raw_labels"), offs, batch["label_lut"], ignore)
    VD = constants("MINK_VOXDS_")
    ds = np.zeros((n_scenes, VD["PARAMS"]), np.float64)
    ds[:, VD["Q"]], ds[:, VD["VOXEL"]], ds[:, VD["IGNORE"]] = np.maximum(lp[:, 0], 0.0), 1.0, ignore
    c, f, labels, src, ds_offs, ds_status = voxel_downsample_batch(c, f, mapped, offs, torch.from_numpy(ds).pin_memory().to(dev, non_blocking=True))
    labels = labels.long()
    status = torch.zeros(5, dtype=torch.int32, device=dev)
    status[3:4] = ds_status[1:]
    status[4:] = lut_status
    if "aug_params" in batch:
        P = batch["aug_params"].detach().cpu().numpy().astype(np.float64) if torch.is_tensor(batch["aug_params"]) else np.array(batch["aug_params"], np.float64)
        sink = np.zeros((1, SEG["PARAMS"]), np.float64)
        for M in ("A0", "A1", "B"):
            sink[0, SEG[M]:SEG[M] + 9] = np.eye(3).reshape(-1)
        sink[0, SEG["DROPOUT"]] = 2.0  # (coins are < 1: the tail past the representatives is dropped)
        streams = torch.cat([batch["aug_streams"].to(dev, torch.int32), torch.zeros(1, dtype=torch.int32, device=dev)])
        c, f, rows, seg_status = _augment_seg_launch(c, f, ds_offs, np.concatenate([P, sink]), streams, batch["aug_seed"],
                                                     [-1] * f.shape[1])
        rows = rows.long().clamp_(0, max(n - 1, 0))  # (rows past the survivors are not written: any index will do there)
        labels, src = labels[rows], src[rows]
        status[:3] = seg_status
    else:
        status[0] = ds_status[0]
    lidar_finish_rows(c, f, status[:1], voxel_size)
    if count_async:
        host = torch.empty(5, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return c, f, labels, src, (host, ev)
    st = status.cpu()
    lidar_batch_status_check(st)
    k = int(st[0])
    return c[:k], f[:k], labels[:k], src[:k]


def image_batch_check(offsets, sizes, programs, n_bytes):
    """Host check of an image batch before it goes to the device (`collate_images` hands these over as host arrays): offsets
    int64 [B+1] in bytes, sizes int32 [B,2] = (w, h), programs float64 [B, MINK_IMG_PARAMS].  Returns (B, width of the widest
    sample).  The kernels skip a sample that does not fit (its output is NaN); here the same thing raises."""
    from .._lib import constants

    I = constants("MINK_IMG_")
    offsets, sizes, programs = np.asarray(offsets), np.asarray(sizes), np.asarray(programs)
    B = sizes.shape[0]
    if offsets.shape != (B + 1,) or sizes.shape != (B, 2) or programs.shape != (B, I["PARAMS"]):
        raise ValueError(f"image batch: offsets {offsets.shape}, sizes {sizes.shape}, programs {programs.shape} for {B} images "
                         f"([B+1], [B,2], [B,{I['PARAMS']}])")
    if B == 0:
        return 0, 0
    nbytes = 3 * sizes[:, 0].astype(np.int64) * sizes[:, 1].astype(np.int64)
    if (sizes < 1).any() or (nbytes > 3 * 0x7FFFFFFF).any() or offsets[0] != 0 or (np.diff(offsets) != nbytes).any() or offsets[-1] != n_bytes:
        raise ValueError("image batch: offsets are not the running sum of 3 * w * h over the images of the packed buffer")
    widths = programs[:, I["WIDTH"]]
    if not ((widths >= 0) & (widths <= I["MAX_WIDTH"]) & (widths == np.floor(widths))).all():
        raise ValueError(f"image batch: chain widths {widths} (whole numbers 0 .. {I['MAX_WIDTH']})")
    return B, int(widths.max())


def image_paste_check(table, sizes, fg_bytes, mask_bytes):
    """Host check of the paste table of an image batch (`collate_images`: "paste_table"): int64 [B, MINK_PASTE_PARAMS] against the
    batch's sizes int32 [B,2] = (w, h) and the byte counts of the packed frames and masks.  Returns (max_w, max_h), the largest
    paste rectangle of the batch per axis, (0, 0) when no sample pastes.  `mink_img_paste` skips a sample whose row does not fit;
    here the same thing raises."""
    from .._lib import constants

    P = constants("MINK_PASTE_")
    table, sizes = np.asarray(table), np.asarray(sizes)
    B = sizes.shape[0]
    if table.shape != (B, P["PARAMS"]) or table.dtype != np.int64 or sizes.shape != (B, 2):
        raise ValueError(f"paste table: {table.dtype} {table.shape} for {B} images (int64 [B,{P['PARAMS']}])")
    max_w = max_h = 0
    for b in np.nonzero(table[:, P["RW"]])[0]:
        fo, mo, fw, fh, mw, mh, rw, rh = (int(table[b, P[k]]) for k in ("FG_OFFSET", "MASK_OFFSET", "FG_W", "FG_H", "MASK_W", "MASK_H",
                                                                        "RW", "RH"))
        if not all(1 <= v <= P["MAX_SIDE"] for v in (fw, fh, mw, mh, rw, rh)):
            raise ValueError(f"paste table, sample {b}: sides {(fw, fh)}, {(mw, mh)}, {(rw, rh)} (1 .. {P['MAX_SIDE']})")
        if fo < 0 or fo + 3 * fw * fh > fg_bytes or mo < 0 or mo + mw * mh > mask_bytes:
            raise ValueError(f"paste table, sample {b}: frame at byte {fo} of {fg_bytes} or mask at byte {mo} of {mask_bytes} does "
                             "not lie inside its buffer")
        w, h = int(sizes[b, 0]), int(sizes[b, 1])
        max_w, max_h = max(max_w, min(w, rw)), max(max_h, min(h, rh))
    return max_w, max_h


def prepare_image_batch(packed, offsets, sizes, programs, size=224, stages=False, paste=None):
    """The input of a batch of decoded frames (co3d_2d/src/data/loader.py: `collate_images`), on the current stream: the three
    rounds of the AugMix chains (`mink_img_chain_round`) and the fused crop / resize / ColorJitter / flip / PCA / Normalize / mix
    tail (`mink_img_finish`).  packed: uint8 [n_bytes] on the device, the HWC RGB images one after the other; offsets int64 [B+1]
    (bytes), sizes int32 [B,2] = (w, h) and programs float64 [B, MINK_IMG_PARAMS] (co3d_2d/src/data/transforms.py:
    `compile_program`) as HOST arrays or CPU tensors: they are checked here and copied.  Nothing is read back.
    paste: None, or {"fg": uint8 vector on the device, the packed frames to paste, "mask": uint8 vector on the device, their mask
    planes, "table": HOST int64 [B, MINK_PASTE_PARAMS]} (`image_paste_check`): before the chains run, `mink_img_paste` composites
    every pasting sample over its slot, so `packed` IS MODIFIED: such a slot holds the background on entry and the composite after.
    Returns float32 [B,3,size,size]; with `stages=True` also uint8 [B, width+1, size, size, 3], every branch after its flip."""
    from .._lib import check, lib

    if not (torch.is_tensor(packed) and packed.is_cuda and packed.dtype == torch.uint8 and packed.dim() == 1):
        raise TypeError("prepare_image_batch: the packed frames are one uint8 vector on the GPU (move the batch to cuda first)")
    host = [v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v) for v in (offsets, sizes, programs)]
    offs, szs, progs = host[0].astype(np.int64), host[1].astype(np.int32), np.ascontiguousarray(host[2], np.float64)
    B, width = image_batch_check(offs, szs, progs, packed.numel())
    if paste is not None:
        fg, mask = paste["fg"], paste["mask"]
        for v in (fg, mask):
            if not (torch.is_tensor(v) and v.device == packed.device and v.dtype == torch.uint8 and v.dim() == 1 and v.is_contiguous()):
                raise TypeError("prepare_image_batch: paste['fg'] and paste['mask'] are contiguous uint8 vectors on the device of `packed`")
        if not packed.is_contiguous():
            raise TypeError("prepare_image_batch: the paste writes into `packed`, which must be contiguous")
        tab = paste["table"]
        tab = np.ascontiguousarray(tab.detach().cpu().numpy() if torch.is_tensor(tab) else tab)
        paste_extent = image_paste_check(tab, szs, fg.numel(), mask.numel())
    dev, S = packed.device, int(size)
    out = torch.empty(B, 3, S, S, dtype=torch.float32, device=dev)
    st = torch.empty(B, width + 1, S, S, 3, dtype=torch.uint8, device=dev) if stages else None
    if B == 0:
        return (out, st) if stages else out
    if not packed.is_contiguous():
        packed = packed.contiguous()
    up = lambda a: torch.from_numpy(a).pin_memory().to(dev, non_blocking=True)  # noqa: E731
    d_offs, d_szs, d_progs = up(offs), up(np.ascontiguousarray(szs)), up(progs)
    n_pix = packed.numel() // 3
    L = lib()
    ws = torch.empty(max(1, L.mink_img_workspace_bytes(n_pix, B, width, S)), dtype=torch.uint8, device=dev)
    stream = torch._C._cuda_getCurrentRawStream(dev.index)
    from .._lib import constants

    if paste is not None and paste_extent[0] > 0:  # (no sample pastes: no upload, no launch)
        d_tab = up(tab)
        check(L.mink_img_paste(packed.data_ptr(), d_offs.data_ptr(), d_szs.data_ptr(), n_pix, B, fg.data_ptr(), fg.numel(),
                               mask.data_ptr(), mask.numel(), d_tab.data_ptr(), paste_extent[0], paste_extent[1], stream))
    I = constants("MINK_IMG_")
    depth = 0
    for k in range(1, width + 1):
        col = progs[:, I["BRANCH"] + k * I["BRANCH_STRIDE"] + I["B_DEPTH"]]
        depth = max(depth, int(col[progs[:, I["WIDTH"]] >= k].max(initial=0)))
    for r in range(min(depth, I["MAX_DEPTH"])):  # (a round no chain reaches is not launched)
        check(L.mink_img_chain_round(packed.data_ptr(), d_offs.data_ptr(), d_szs.data_ptr(), d_progs.data_ptr(), n_pix, B, width, r,
                                     ws.data_ptr(), ws.numel(), stream))
    check(L.mink_img_finish(packed.data_ptr(), d_offs.data_ptr(), d_szs.data_ptr(), d_progs.data_ptr(), n_pix, B, width, S,
                            ws.data_ptr(), ws.numel(), out.data_ptr(), None if st is None else st.data_ptr(), stream))
    return (out, st) if stages else out


class SampleSceneError(RuntimeError):
    """`mink_fps_scenes` left a scene unsampled: it is empty (or its offsets leave the matrix), its first pick lies outside
    it, or it holds more rows than the caller's bound."""


def fps_status_check(status):
    """Raise on the status word of `mink_fps_scenes` (a host int or a one-element tensor)."""
    from .._lib import FPS_BAD_START, FPS_EMPTY_SCENE, FPS_SCENE_TOO_LARGE

    s = int(status)
    if s:
        why = [t for bit, t in ((FPS_EMPTY_SCENE, "an empty scene (or offsets outside the matrix)"),
                                (FPS_BAD_START, "a first pick outside its scene"),
                                (FPS_SCENE_TOO_LARGE, "a scene above the n_max bound")) if s & bit]
        raise SampleSceneError("farthest_point_sample: " + ", ".join(why) + f" (status {s}); such a scene's picks are -1")


def farthest_point_sample(xyz, offsets, num_points, start, n_max=None, status_async=False):
    """Farthest-point sampling of every scene of a batch with `mink_fps_scenes` (reference transforms.py:597-630, one scene at
    a time on the CPU): -> int64 [B, num_points] on the device, the GLOBAL rows picked, in pick order.

    xyz f32 [n, >= 3] on the device, rows of any pitch with unit column stride (a `[:, 1:4]` view of float coordinates goes in
    without a copy; int32 coordinates are converted); offsets int32 [B + 1]; start int32 [B] = the scene-local row of every
    scene's first pick (the reference's `np.random.randint(0, N)`).  `n_max`: a bound on the largest scene (default: all rows),
    which sizes the workspace.  The status word is read back (one small synchronisation) and a rejected scene raises
    `SampleSceneError`, unless `status_async`: then (idx, (pinned status, event)) comes back for `fps_status_check` later."""
    from .._lib import check, lib

    if not xyz.is_cuda:
        raise RuntimeError("farthest_point_sample runs on the GPU: move the batch to cuda first")
    dev = xyz.device
    if xyz.dim() != 2 or xyz.shape[1] < 3:
        raise ValueError(f"farthest_point_sample: xyz of shape {tuple(xyz.shape)}, [n, >= 3] expected")
    if xyz.dtype != torch.float32 or xyz.stride(1) != 1 or xyz.stride(0) < 3:
        xyz = xyz[:, :3].float().contiguous()
    n, ld, m = int(xyz.shape[0]), int(xyz.stride(0)), int(num_points)
    offs = offsets.to(dev, torch.int32, non_blocking=True).contiguous()
    first = torch.as_tensor(start).to(dev, torch.int32, non_blocking=True).contiguous()
    B = offs.numel() - 1
    if first.numel() != B:
        raise ValueError(f"farthest_point_sample: {first.numel()} first picks for {B} scenes")
    n_max = n if n_max is None else min(int(n_max), n)
    idx = torch.empty(B, m, dtype=torch.int32, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    ws = torch.empty(max(1, lib().mink_fps_workspace_bytes(n_max, B)), dtype=torch.uint8, device=dev)
    check(lib().mink_fps_scenes(xyz.data_ptr(), n, ld, offs.data_ptr(), first.data_ptr(), B, m, n_max, idx.data_ptr(),
                                status.data_ptr(), ws.data_ptr(), ws.numel(), torch._C._cuda_getCurrentRawStream(dev.index)))
    if status_async:
        host = torch.empty(1, dtype=torch.int32, pin_memory=True)
        host.copy_(status, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        return idx.long(), (host, ev)
    fps_status_check(status.item())
    return idx.long()


def sample_scene_rows(batch_coords, feats, idx):
    """Keep the rows `idx` (int64 [B, m], global rows, scene by scene) of a batch: -> (coordinates [B m, .], features [B m, C],
    scene_offsets int32 [B + 1] = arange(B + 1) * m), the survivors in pick order."""
    B, m = idx.shape
    rows = idx.reshape(-1)
    offsets = torch.arange(B + 1, dtype=torch.int32, device=idx.device) * m
    return batch_coords[rows], feats[rows], offsets


def kaiming_normal_(tensor, a=0, mode="fan_in", nonlinearity="leaky_relu"):
    """ME.utils.kaiming_normal_ for convolution kernels laid out (K, Cin, Cout): fan_in = K * Cin, fan_out = K * Cout."""
    import math

    k = tensor.shape[0] if tensor.dim() == 3 else 1
    fan = k * (tensor.shape[-2] if mode == "fan_in" else tensor.shape[-1])
    std = torch.nn.init.calculate_gain(nonlinearity, a) / math.sqrt(fan)
    with torch.no_grad():
        return tensor.normal_(0, std)
