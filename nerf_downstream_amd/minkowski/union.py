"""ME.MinkowskiUnion (csrc/union.hip): the sum of 2..8 sparse tensors over the UNION of their coordinate maps -- a voxel one
input holds contributes its row, a voxel several hold the sum of theirs.  The inputs may live on any mix of coordinate managers:
it is what joins a decoder tensor of a generative net with the encoder tensor of its tensor stride (the skip of a U-shaped
completion net), which `+` and `ME.cat` refuse by their same-manager check.

Row order of the union [ME-recall: ME's own order is unpinned, ME is absent; this is the definition here]: sample-major; inside
a sample the rows of input 0 in their order, then the rows of input 1 that no earlier input holds, in their order, and so on.

A coordinate manager holds one map per tensor stride, so the result lives on a DERIVED manager of its own
(CoordinateManager.from_coordinates, as with pruning and the generative transpose): a plan recorded for `prepare_ahead` does not
cover it."""
import ctypes

import torch
import torch.nn as nn

from .._lib import CONSTANTS, check, lib
from ._rt import _f32c, _row_stride, _scratch, _stream
from .coords import ORIGIN_TS, CoordinateManager, CoordinateMapKey
from .tensor import SparseTensor

MAX_INPUTS = CONSTANTS["MINK_UNION_MAX_INPUTS"]


def _pointers(tensors):
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _counts(tensors):
    return (ctypes.c_int64 * len(tensors))(*[t.shape[0] for t in tensors])


def union_map(tensors):
    """(coordinates int32 [N, 4], in2out: one int32 [n_i] per input, out2in int32 [k, N], batch offsets int32 [B + 1]) of the
    union of the coordinate maps of `tensors` (SparseTensors at one tensor stride and batch count, on any mix of managers):
    in2out[i][r] is the union row of row r of input i, out2in[i][u] the row of input i behind union row u or -1, exact inverses of
    each other.  out2in is a view of row pitch sum n_i.  mink_union_build; one host read: the count N."""
    L, k, dev = lib(), len(tensors), tensors[0].F.device
    coords, offs = [], []
    for t in tensors:
        m, key = t.coordinate_manager, t.coordinate_map_key
        assert m.has_level(key.ts)
        coords.append(m.get_coordinates(key))
        offs.append(m.batch_offsets(key))
    B = tensors[0].coordinate_manager.batch_size()
    S = sum(c.shape[0] for c in coords)
    idx = torch.empty((k + 1) * S + B + 2, dtype=torch.int32, device=dev)  # [in2out of every input | out2in | offsets | total]
    in2out = list(idx[:S].split([c.shape[0] for c in coords]))
    out2in, boff, total = idx[S : (k + 1) * S].view(k, S), idx[(k + 1) * S : (k + 1) * S + B + 1], idx[(k + 1) * S + B + 1 :]
    out_coords = torch.empty(S, 4, dtype=torch.int32, device=dev)
    n_host = _counts(coords)
    ws = _scratch(int(L.mink_union_workspace_bytes(k, n_host, B)), dev, "union")
    check(L.mink_union_build(k, _pointers(coords), _pointers(offs), n_host, B, out_coords.data_ptr(), _pointers(in2out), out2in.data_ptr(),
                             S, boff.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    N = int(total.item())
    return out_coords[:N], in2out, out2in[:, :N], boff


class UnionFunction(torch.autograd.Function):
    """y[u] = the sum of x_i[out2in[i][u]] over the inputs that hold union row u, in ascending input index, the first one copied
    (mink_union_sum: bitwise reproducible, no float atomics); backward dx_i[r] = dy[in2out[i][r]] (mink_prune_gather), for the
    inputs that require a gradient only."""

    @staticmethod
    def forward(ctx, out2in, in2out, *xs):
        xs = [_f32c(x) for x in xs]
        k, n_out, C = len(xs), out2in.shape[1], xs[0].shape[1]
        y = torch.empty(n_out, C, dtype=torch.float32, device=xs[0].device)
        ld = (ctypes.c_int32 * k)(*[_row_stride(x) for x in xs])
        check(lib().mink_union_sum(k, _pointers(xs), ld, _counts(xs), C, out2in.data_ptr(), out2in.stride(0), n_out,
                                   y.data_ptr(), C, _stream()))
        ctx.in2out, ctx.n_out = in2out, n_out
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        C, grads = gy.shape[1], []
        for i, rows in enumerate(ctx.in2out):
            if not ctx.needs_input_grad[2 + i]:
                grads.append(None)
                continue
            gx = torch.empty(rows.shape[0], C, dtype=torch.float32, device=gy.device)
            check(lib().mink_prune_gather(gy.data_ptr(), _row_stride(gy), ctx.n_out, C, rows.data_ptr(), rows.shape[0], gx.data_ptr(), C,
                                          _stream()))
            grads.append(gx)
        return (None, None, *grads)


class MinkowskiUnion(nn.Module):
    """ME.MinkowskiUnion: `forward(*inputs)` takes 2..8 SparseTensors of one tensor stride, channel count, device and batch
    count, on the same coordinate manager or on different ones, and returns their sum over the union of their coordinate maps
    at that tensor stride, on a derived manager.  One input given twice is legal: every row doubles."""

    def forward(self, *inputs):
        if not 2 <= len(inputs) <= MAX_INPUTS:
            raise ValueError(f"MinkowskiUnion: {len(inputs)} inputs (at least 2 and at most {MAX_INPUTS})")
        for i, t in enumerate(inputs):
            if not isinstance(t, SparseTensor):
                raise ValueError(f"MinkowskiUnion: input {i} is a {type(t).__name__}, not a SparseTensor")
        first = inputs[0]
        ts, C, dev = first.coordinate_map_key.ts, first.F.shape[1], first.F.device
        for i, t in enumerate(inputs):
            if t.coordinate_map_key.ts == ORIGIN_TS:
                raise ValueError(f"MinkowskiUnion: input {i} is at the origin map (one row per sample: add such tensors with `+`)")
            if t.coordinate_map_key.ts != ts:
                raise ValueError(f"MinkowskiUnion: input {i} is at tensor stride {t.coordinate_map_key.ts}, input 0 at {ts} (one tensor "
                                 "stride for all inputs)")
            if t.F.shape[1] != C:
                raise ValueError(f"MinkowskiUnion: input {i} has {t.F.shape[1]} channels, input 0 has {C} (one channel count for all inputs)")
            if t.F.device != dev:
                raise ValueError(f"MinkowskiUnion: input {i} is on {t.F.device}, input 0 on {dev} (one device for all inputs)")
        B = first.coordinate_manager.batch_size()
        for i, t in enumerate(inputs):
            if t.coordinate_manager.batch_size() != B:
                raise ValueError(f"MinkowskiUnion: input {i} has {t.coordinate_manager.batch_size()} samples, input 0 has {B} (one batch "
                                 "count for all inputs)")
        coords, in2out, out2in, boff = union_map(inputs)
        out = UnionFunction.apply(out2in, in2out, *[t.F for t in inputs])
        return SparseTensor(out, CoordinateMapKey(ts), CoordinateManager.from_coordinates(coords, ts, B, batch_offsets=boff))
