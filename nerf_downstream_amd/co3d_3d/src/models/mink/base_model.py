"""Input boundary of the Minkowski models (counterpart of the reference's
co3d_3d/src/models/mink/base_model.py:6-13 and models/interface.py:4-9)."""
import os
from abc import ABC, abstractmethod

from nerf_downstream_amd import minkowski as _HIP_ME


class InputInterface(ABC):
    @abstractmethod
    def process_input(self, batch):
        ...


class MinkowskiBaseModel(_HIP_ME.MinkowskiNetwork, InputInterface):
    """`process_input(batch)` -> TensorField, as in the reference.  On the HIP backend it also
    prepares, on a side HIP stream, every coordinate / kernel map the network asked for on the
    previous batch (hash build, stride maps, neighbour tables are pure functions of the
    coordinates), so calling it for batch i+1 while batch i is still in backward hides the map
    construction and its host synchronisations behind compute."""

    def __init__(self, dimension=3, ME=None):
        _HIP_ME.MinkowskiNetwork.__init__(self, dimension)
        self._ME = ME or _HIP_ME
        self._coord_plan = None
        self._recent_traces = []  # map-request traces of the last few fields (filled by their forward pass)
        self._side = None
        self._sampler_status = None  # (pinned status word of the last mink_fps_scenes call, event recorded after its copy)
        # (MINK_PREPARE_AHEAD=0: every batch's maps are built on the compute stream, on demand -- the A/B switch of the trainer CLI)
        self.prepare_ahead = os.environ.get("MINK_PREPARE_AHEAD", "1") != "0"

    def process_input(self, batch, defer=False, _fence=True):
        """`defer=True` (extension, HIP backend): only launch the coordinate pyramid of this batch
        on the side stream and return at once; `finish_input(field)` -- call it after the current
        batch's forward/backward have been queued -- reads the row counts back (already there by
        then, so the host never blocks) and builds the kernel maps."""
        ME = self._ME
        if "links" in batch:  # compact PeRFception batch: de-quantise + links -> coordinates on the device
            with self._prepare_stream_ctx(batch["links"], fence=batch.get("h2d_event", True)):
                coords, feats = ME.utils.decode_plenoxel_batch(batch)
            batch = dict(batch, coordinates=coords, features=feats)
        if "sample_points" in batch:  # the recipe's sampler (data/sampling.py): a fixed number of rows per scene, taken here
            with self._prepare_stream_ctx(batch["coordinates"], fence=batch.get("h2d_event", True)):
                batch = self._sample(batch, status_async=defer)
        if "ds_params" in batch:  # raw point clouds (ScannetDataset): down-sampled, then the drawn programs, all on the device
            if not getattr(ME, "SUPPORTS_PREPARE_AHEAD", False):
                raise RuntimeError("point clouds are prepared by the HIP backend (mink_voxel_downsample_scenes)")
            with self._prepare_stream_ctx(batch["coordinates"], fence=batch.get("h2d_event", True)):
                out = ME.utils.prepare_point_batch(batch, count_async=defer)
            batch = {k: v for k, v in batch.items() if not k.startswith("aug_") and k not in ("ds_params", "color_params")}
            batch["coordinates"], batch["features"], batch["row_labels"], batch["point_rows"] = out[:4]
            if defer:  # the row count is still on its way to the host
                return _PendingField(self, batch, out[4])
        if "scan" in batch:  # raw LiDAR scans (SemanticKITTIDataset): label table, down-sampling, the drawn program, xyzi features
            if not getattr(ME, "SUPPORTS_PREPARE_AHEAD", False):
                raise RuntimeError("LiDAR scans are prepared by the HIP backend (mink_lidar_decode_scans)")
            with self._prepare_stream_ctx(batch["scan"], fence=batch.get("h2d_event", True)):
                out = ME.utils.prepare_lidar_batch(batch, count_async=defer)
            batch = {k: v for k, v in batch.items() if not k.startswith("aug_") and k not in ("scan", "raw_labels", "lidar_params", "label_lut")}
            batch["coordinates"], batch["features"], batch["row_labels"], batch["point_rows"] = out[:4]
            if defer:  # the row count is still on its way to the host
                return _PendingField(self, batch, out[4])
        if "aug_params" in batch:  # augmentation programs drawn by the loader: applied to the whole batch here
            with self._prepare_stream_ctx(batch["coordinates"], fence=batch.get("h2d_event", True)):
                coords, feats, rows, pending = self._augment(batch, count_async=defer)
            batch = dict(batch, coordinates=coords, features=feats)
            if rows is not None:  # segmentation program: the source row of every survivor (labels follow it)
                batch["source_rows"] = rows
            if pending is not None:  # rows were dropped: the survivor count is still on its way to the host
                return _PendingField(self, batch, pending)
        coords, feats = batch["coordinates"], batch["features"]
        if not (self.prepare_ahead and getattr(ME, "SUPPORTS_PREPARE_AHEAD", False) and coords.is_cuda):
            return _with_rows(ME.TensorField(coordinates=coords, features=feats), batch)
        import torch

        for trace in self._recent_traces:  # the newest field may not have been through forward yet
            if trace:
                plan = ME.CoordinateManager.compile_plan(trace)
                if self._coord_plan is None or len(plan) > len(self._coord_plan):
                    self._coord_plan = plan
        skew = getattr(getattr(ME, "streams", None), "skew", None)
        # a batch that was just copied to the device carries the event recorded after its H2D copies
        # (train.py `_to_device`): the prepare stream waits for exactly that, not for the compute stream
        with self._prepare_stream_ctx(coords, fence=batch.get("h2d_event", False) if _fence else False):
            if skew is not None:
                skew(self._side)
            tf = ME.TensorField(coordinates=coords, features=feats, plan=self._coord_plan or [], defer=defer)
        self._recent_traces = [tf.coordinate_manager.trace] + self._recent_traces[:2]
        return _with_rows(tf, batch)

    def _sample(self, batch, status_async=False):
        """The batch cut down to `sample_points` rows per scene: the farthest-point picks from `fps_start` (mink_fps_scenes)
        or the host-drawn `sample_rows`, gathered in pick order; `scene_offsets` becomes the new one.  Both sizes are fixed, so
        nothing is waited for: with `status_async` the kernel's status word is looked at when the next batch comes in."""
        import torch

        ME, coords, m = self._ME, batch["coordinates"], int(batch["sample_points"])
        if self._sampler_status is not None:  # the previous batch's: long there
            self._check_sampler_status()
        if "fps_start" not in batch:
            idx = batch["sample_rows"].to(coords.device).long().reshape(-1, m)
        elif getattr(ME, "SUPPORTS_PREPARE_AHEAD", False):
            if not coords.is_cuda:
                raise RuntimeError("FarthestPointSample runs on the GPU: move the batch to cuda first")
            out = ME.utils.farthest_point_sample(coords[:, 1:4], batch["scene_offsets"], m, batch["fps_start"],
                                                 n_max=batch.get("sample_n_max"), status_async=status_async)
            idx = out[0] if status_async else out
            if status_async:
                self._sampler_status = out[1]
        else:  # the CPU backend of the trainer tests
            from nerf_downstream_amd.co3d_3d.src.data.sampling import fps_numpy

            idx = torch.from_numpy(fps_numpy(coords[:, 1:4].float().numpy(), batch["scene_offsets"].numpy(), m,
                                             batch["fps_start"].numpy()))
        from nerf_downstream_amd.minkowski.utils import sample_scene_rows

        drop = ("sample_points", "sample_rows", "fps_start", "sample_n_max", "links", "density", "sh_q")
        out = {k: v for k, v in batch.items() if k not in drop}
        out["coordinates"], out["features"], out["scene_offsets"] = sample_scene_rows(coords, batch["features"], idx)
        return out

    def _check_sampler_status(self):
        from nerf_downstream_amd.minkowski.utils import fps_status_check

        (host, event), self._sampler_status = self._sampler_status, None
        event.synchronize()
        fps_status_check(host)

    def _augment(self, batch, count_async=False):
        """-> (coordinates, features, source rows or None, pending count or None)"""
        from nerf_downstream_amd.co3d_3d.src.data import seg_transforms
        from nerf_downstream_amd.co3d_3d.src.data.transforms import raw_columns

        if not getattr(self._ME, "SUPPORTS_PREPARE_AHEAD", False):
            raise RuntimeError("augmentation programs are applied by the HIP backend (mink_augment_scenes)")
        if not batch["coordinates"].is_cuda:
            raise RuntimeError("augmentation runs on the GPU: move the batch to cuda first")
        args = (batch["coordinates"], batch["features"], batch["scene_offsets"], batch["aug_params"], batch["aug_streams"],
                batch["aug_seed"])
        if batch["aug_params"].shape[-1] == seg_transforms.SEG["PARAMS"]:  # segmentation program (MINK_SEGAUG_*)
            out = self._ME.utils.augment_seg_batch(*args, seg_transforms.raw_columns(batch["feature_names"]), count_async=count_async)
            return out if count_async else (*out, None)
        out = self._ME.utils.augment_batch(*args, raw_columns(batch["feature_names"]), count_async=count_async)
        return (out[0], out[1], None, out[2]) if count_async else (*out, None, None)

    def _prepare_stream_ctx(self, t, fence=True):
        """The prepare stream as a context, or a null context without prepare-ahead.  `fence`: True = wait for
        the current stream (where the batch's H2D copies were queued), an event = wait for it, False = none."""
        import contextlib

        import torch

        if not (self.prepare_ahead and t.is_cuda):
            return contextlib.nullcontext()
        if self._side is None:
            self._side = self._new_prepare_stream(t.device)
        if fence is True:
            self._side.wait_stream(torch.cuda.current_stream(t.device))
        elif fence:
            self._side.wait_event(fence)
        wait_gate = getattr(getattr(self._ME, "streams", None), "wait_prepare_gate", None)
        if wait_gate is not None:  # (MINK_PREPARE_GATE: one map build per step, beside its middle)
            wait_gate(self._side)
        return torch.cuda.stream(self._side)

    def _new_prepare_stream(self, device):
        new_stream = getattr(getattr(self._ME, "streams", None), "new_stream", None)
        import torch

        st = new_stream(device, "prepare") if new_stream is not None else torch.cuda.Stream(device=device)
        from nerf_downstream_amd.memory import reserve_on, reserved

        if reserved(device):  # (a process that reserved a segment for its compute stream -- bench.py, train.py -- gets one here too)
            reserve_on(st)
        return st

    @staticmethod
    def finish_input(field):
        if isinstance(field, _PendingField):
            field = field.materialise()
        finish = getattr(field, "finish", None)
        if finish is not None:
            finish()
        return field


def _with_rows(field, batch):
    """The field of an augmented segmentation batch carries the source row of every one of its rows (`source_rows`):
    per-point tensors of the batch -- labels, dists -- are gathered by it."""
    if "source_rows" in batch:
        field.source_rows = batch["source_rows"]
    if "row_labels" in batch:  # (point clouds: the voted class of every row, and its raw point)
        field.row_labels, field.point_rows = batch["row_labels"], batch["point_rows"]
    return field


class _PendingField:
    """A deferred batch whose augmentation dropped voxels: the transformed rows are on the device, their
    number arrives through pinned memory.  `finish_input` (called once the current batch's forward and
    backward are queued, so the count is there and the host does not wait) slices the buffers and
    builds the field -- pyramid and maps in one go -- on the prepare stream."""

    def __init__(self, model, batch, pending):
        self.model, self.batch, (self.count, self.event) = model, batch, pending

    def materialise(self):
        self.event.synchronize()
        if self.count.numel() > 4:  # LiDAR scans: the point cloud's four words, then the label words outside the table
            from nerf_downstream_amd.minkowski.utils import lidar_batch_status_check

            lidar_batch_status_check(self.count)
        elif self.count.numel() > 3:  # point cloud: (survivors, direct elastic grids, passes not applied, down-sampling status)
            from nerf_downstream_amd.minkowski.utils import points_status_check

            points_status_check(self.count)
        elif self.count.numel() > 1:  # segmentation program: (survivors, direct elastic grids, elastic passes not applied)
            from nerf_downstream_amd.minkowski.utils import seg_status_check

            seg_status_check(self.count)
        k = int(self.count[0])
        b = {key: v for key, v in self.batch.items() if not key.startswith("aug_") and key != "links"}
        b["coordinates"], b["features"] = b["coordinates"][:k], b["features"][:k]
        for key in ("source_rows", "row_labels", "point_rows"):
            if key in b:
                b[key] = b[key][:k]
        return self.model.process_input(b, defer=False, _fence=False)  # the rows were produced on the prepare stream

    def sparse(self):
        return MinkowskiBaseModel.finish_input(self).sparse()
