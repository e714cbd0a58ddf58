"""SparseTensor / TensorField of the HIP backend (subset of the ME classes used by the
reference: base_model.py:10-13, resnet.py:164,177, resnet_block.py:66, sparse_conv.py:387-425)."""
import torch

from .._lib import check, lib
from . import functional as Fn
from . import streams
from ._rt import _stream
from .eltwise import AddFunction
from .field import FieldGatherCatFunction, SegmentMeanFunction, index_csr, lazy_index_csr, segment_mean
from .head import slice_rows
from .interp import InterpolationFunction, SplatFunction
from .coords import CoordinateManager, CoordinateMapKey


class SparseTensor:
    """Feature matrix F [N,C] (ordinary autograd tensor in HBM) + an immutable coordinate map
    shared by reference through the coordinate manager."""

    def __init__(self, features, coordinate_map_key=None, coordinate_manager=None, coordinates=None, tensor_stride=1):
        if coordinate_map_key is None:
            assert coordinates is not None, "give either a coordinate_map_key or coordinates"
            assert coordinate_manager is None and _is_one(tensor_stride)
            coordinate_manager = CoordinateManager(D=coordinates.shape[1] - 1, device=coordinates.device)
            coordinate_map_key = coordinate_manager.insert_field(coordinates.int())
            if coordinate_manager.levels[1].n != coordinates.shape[0]:
                raise ValueError("duplicate coordinates: use ME.TensorField(...).sparse() to average them")
        self._F = features
        self.coordinate_map_key = coordinate_map_key
        self._manager = coordinate_manager

    @property
    def F(self):
        return self._F

    @property
    def C(self):
        return self._manager.get_coordinates(self.coordinate_map_key)

    @property
    def coordinate_manager(self):
        return self._manager

    @property
    def tensor_stride(self):
        return self.coordinate_map_key.get_tensor_stride()

    @property
    def D(self):
        return self._manager.D

    @property
    def shape(self):
        return self._F.shape

    @property
    def device(self):
        return self._F.device

    def __len__(self):
        return self._F.shape[0]

    def _check(self, other):
        if not (self._manager is other._manager and self.coordinate_map_key == other.coordinate_map_key):
            raise ValueError("SparseTensors must share the coordinate manager and the coordinate map key")

    def slice(self, field):
        """`out.slice(x)` (reference res16unet.py:435): the features of this tensor-stride-1 tensor read
        back at the rows of the TensorField it was quantised from (F[inverse mapping])."""
        if field.coordinate_manager is not self._manager:
            raise ValueError("slice: needs the tensor-stride-1 tensor and the field it came from (a tensor at another tensor "
                             "stride is read at a field of ITS OWN coordinate manager only)")
        m = self._manager
        if not _is_one(self.tensor_stride):
            # reference fcnn.py:158-161 (strides 2, 8, 32, 128): every field row reads the voxel of this stride containing it
            # (mink_field_map, kept on the manager).  The gather is left pending so that ME.cat of several such slices
            # writes the concatenated rows in one launch; `.F` of the result runs it for this slice alone.
            field._settle()
            return TensorField(features=None, coordinates=field.C, _manager=m, _origin=field,
                               _pending=(self._F, m.field_map(self.coordinate_map_key, field.C)))
        if m.levels[1].n == field.F.shape[0]:
            F = self._F  # no duplicates: the rows are the field's rows, in order (no copy)
        else:
            F = slice_rows(self._F, m.field_inverse, *_field_members(m))  # (gather; backward: fixed-order segment sum)
        return TensorField(features=F, coordinates=field.C, _manager=m, _origin=field)

    def features_at_coordinates(self, query):
        """Trilinear interpolation of this tensor's features at the float rows query[N, 4] = (b, x, y, z), at any tensor
        stride -> a tensor [N, C] [ME-recall of SparseTensor.features_at_coordinates; parity unpinned, ME is absent].  An
        absent corner contributes nothing (no renormalisation); the gradient goes to the features only."""
        imap, w = self._manager.interpolation_map_weight(self.coordinate_map_key, query)
        return InterpolationFunction.apply(self._F, imap, w, lazy_index_csr(imap, self._F.shape[0]))

    def interpolate(self, field):
        """`y.interpolate(x)` (reference models/mink/fcnn.py:194-208): this tensor's features, at any tensor stride, read at
        the coordinates of the TensorField `field` -> a TensorField with `field`'s coordinates and manager.  The field need
        not be the one this tensor was quantised from (a splat lives on a manager of its own)."""
        F = self.features_at_coordinates(field.C)
        return TensorField(features=F, coordinates=field.C, _manager=field.coordinate_manager, _origin=field)

    def __iadd__(self, other):  # `out += residual`, reference resnet_block.py:66
        self._check(other)
        self._F = AddFunction.apply(self._F, other._F)
        return self

    def __add__(self, other):
        self._check(other)
        return SparseTensor(AddFunction.apply(self._F, other._F), self.coordinate_map_key, self._manager)

    def __repr__(self):
        return f"SparseTensor(F={tuple(self._F.shape)}, tensor_stride={self.tensor_stride})"


def _field_members(m):
    """(order, seg), int32: the field rows of every voxel in input-row order, CSR -- what sparse() averages over and the
    backward of slice() sums over.  Built once per field and kept on the manager."""
    if m.field_members is None:
        n_unique = m.levels[1].n
        inv = m.field_inverse.long()
        order = torch.sort(inv, stable=True).indices.int()  # members of each voxel, input-row order
        seg = torch.zeros(n_unique + 1, dtype=torch.int32, device=inv.device)
        seg[1:] = torch.cumsum(torch.bincount(inv, minlength=n_unique), 0).int()
        m.field_members = (order, seg)
    return m.field_members


def _check_quantization_mode(who, qm):
    if qm is not None and getattr(qm, "name", str(qm)) != "UNWEIGHTED_AVERAGE":
        raise NotImplementedError(f"{who}(quantization_mode={qm}): only UNWEIGHTED_AVERAGE (the ME default the "
                                  "reference relies on) is implemented")


def _is_one(ts):
    return all(int(t) == 1 for t in (ts if isinstance(ts, (list, tuple)) else [ts]))


class TensorField:
    """ME.TensorField(coordinates=[N,1+D] float (batch,x,y,z), features=[N,C]).

    Owns a fresh coordinate manager; `.sparse()` floors the coordinates, inserts them into the
    hash map and averages the features of rows that collapse onto one voxel (A1, A2)."""

    def __init__(self, features=None, coordinates=None, plan=None, defer=False, **kwargs):
        """`plan` (extension): a compiled CoordinateManager request plan; all its maps are built
        right here, on the current (side) stream, and `.sparse()` makes the consumer stream wait.
        `defer=True` only launches the coordinate pyramid (no host synchronisation); `finish()`
        -- called explicitly once other work has been queued, or implicitly by `.sparse()` --
        reads the row counts back and builds the rest of the plan on the same stream."""
        self._origin = self._pending = None
        if kwargs.get("_manager") is not None:  # a derived field (a slice(), a module's output): shares the manager of the field it came from
            # `_origin`: the field that built the manager -- it alone holds the plan, the build stream and the readiness event,
            # so `.sparse()` of a derived field runs ITS finish() and hand-over.  `_pending` = (source features, (idx, csr_fn)):
            # a strided slice whose gather has not run yet (see SparseTensor.slice).
            assert coordinates is not None and (features is not None or kwargs.get("_pending") is not None)
            self._F, self._C, self._manager, self._plan, self._ready = features, coordinates, kwargs["_manager"], None, None
            origin = kwargs.get("_origin")
            if origin is not None and origin._manager is self._manager:
                self._origin = origin._origin if origin._origin is not None else origin
            self._pending = kwargs.get("_pending")
            return
        assert features is not None and coordinates is not None
        _check_quantization_mode("TensorField", kwargs.get("quantization_mode"))
        if not coordinates.is_cuda:
            raise RuntimeError("nerf_downstream_amd.minkowski runs on the GPU only: move the batch to cuda first")
        self._F, self._C = features, coordinates
        m = self._manager = CoordinateManager(D=coordinates.shape[1] - 1, device=coordinates.device)
        self._plan, self._ready = plan, None
        self._build_stream = streams.current_stream(coordinates.device)
        defer = bool(defer) and plan is not None
        self.coordinate_field_map_key = m.insert_field(coordinates, CoordinateManager.plan_stride_chain(plan), defer=defer)
        if not defer:
            self.finish()

    def finish(self):
        """Second half of a deferred construction (no-op otherwise)."""
        m = self._manager
        if self._plan is None:
            m.finish_field()
            return
        plan, self._plan = self._plan, None
        streams.skew(self._build_stream)
        streams.wait_prepare_gate(self._build_stream)
        with torch.cuda.stream(self._build_stream):
            m.finish_field()
            m.replay(plan)
            F = self._F
            if (Fn._STORAGE_B16 and F.is_cuda and F.dtype == torch.float32 and F.dim() == 2 and F.shape[1] <= 32
                    and F.stride(1) == 1 and m.levels[1].n == F.shape[0]):
                # bf16 storage of the full-resolution stage: the bf16 copy of the input rows (no duplicate voxels: the
                # sparse tensor's features ARE these rows) is made here, beside the previous step, not at the head of this one
                m.xb = (F.data_ptr(), Fn.rows_to_bf16(F))
            self._ready = self._build_stream.record_event()

    @property
    def F(self):
        if self._F is None:  # a strided slice read on its own: the one-source form of the fused gather
            x, fmap = self._pending
            self._F = FieldGatherCatFunction.apply((fmap,), x)
        return self._F

    @property
    def C(self):
        return self._C

    @property
    def coordinate_manager(self):
        return self._manager

    def _like(self, features):
        """A field with these features on this field's rows: same coordinates, same manager, same origin."""
        return TensorField(features=features, coordinates=self._C, _manager=self._manager, _origin=self)

    def _settle(self):
        """Everything the manager holds is usable on the current stream: the origin's deferred construction is finished and,
        when its maps were built ahead on the prepare stream, the current stream waits for them and takes them over -- once;
        later calls, from the origin or from any field derived from it, find nothing left to do."""
        root = self._origin if self._origin is not None else self
        m = root._manager
        root.finish()
        if root._ready is not None:  # maps were built ahead of time on another stream
            cur = streams.current_stream()
            cur.wait_event(root._ready)
            m.hand_over(cur)
            for t in (root._F, root._C):  # may have been produced on the build stream (GPU-side decode)
                t.record_stream(cur)
            for name in ("source_rows", "row_labels", "point_rows"):  # (segmentation batches: the labels of the rows)
                rows = getattr(root, name, None)
                if rows is not None:
                    rows.record_stream(cur)
            if m.xb is not None:
                m.xb[1].record_stream(cur)
            root._ready = None

    def sparse(self, quantization_mode=None):
        """`quantization_mode` (reference res16unet.py:707,781 pass UNWEIGHTED_AVERAGE): the mode the field averages with anyway;
        any other is refused as the constructor refuses it."""
        _check_quantization_mode("TensorField.sparse", quantization_mode)
        m = self._manager
        self._settle()
        n_unique = m.levels[1].n
        F = self.F
        if n_unique == F.shape[0]:
            Fs = F.float()  # no duplicates: unique rows are the input rows, in order
        else:
            order, seg = _field_members(m)
            if F.requires_grad and torch.is_grad_enabled():  # learned per-point features (reference fcnn.py:143-144,165)
                Fs = SegmentMeanFunction.apply(F, order, seg, n_unique)
            else:
                Fs = segment_mean(F, order, seg, n_unique)
        return SparseTensor(Fs, CoordinateMapKey(1), m)

    def splat(self):
        """`x.splat()` (reference models/mink/fcnn.py:186) [ME-recall of TensorField.splat; parity unpinned, ME is absent]:
        every row is spread over the eight corners of its floor cell with the trilinear weights, F_s[v] = the sum of
        w[p][c] * F[p] over the corners that fall on voxel v -- the transpose of interpolation, so the per-channel feature sum
        is kept.  The voxels are the corners listed (point 0, corners 0..7), (point 1, ...), numbered by first occurrence.

        The result lives on a coordinate manager OF ITS OWN: a manager holds one map per tensor stride, and this field's
        manager already holds its floor map at stride 1.  Strided levels, convolutions and pooling work on the splat's
        manager as on any other; `interpolate(field)` reads them back at this field."""
        self._settle()
        C = self._C.detach().float().contiguous()
        n = C.shape[0]
        if n == 0:
            raise ValueError("empty coordinate field")
        corners = torch.empty(8 * n, 4, dtype=torch.int32, device=C.device)
        w = torch.empty(n, 8, dtype=torch.float32, device=C.device)
        status = torch.zeros(1, dtype=torch.int32, device=C.device)
        check(lib().mink_splat_coords(C.data_ptr(), n, corners.data_ptr(), w.data_ptr(), status.data_ptr(), _stream()))
        if int(status.item()) & 1:  # MINK_STATUS_RANGE
            raise ValueError(
                "coordinate outside the supported range (0 <= batch <= 65534, -32768 <= x, y, z <= 32767 for every corner of "
                "the point's cell; NaN and infinite coordinates are refused)"
            )
        m = CoordinateManager(D=C.shape[1] - 1, device=C.device)
        key = m.insert_field(corners)
        n_rows = m.levels[1].n
        imap = m.field_inverse.reshape(n, 8)
        Fs = SplatFunction.apply(self.F, imap, w, index_csr(imap, n_rows), n_rows)
        return SparseTensor(Fs, key, m)
