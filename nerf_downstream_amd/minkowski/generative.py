"""Layers that make and unmake voxels inside a network (csrc/generate.hip): ME.MinkowskiGenerativeConvolutionTranspose,
ME.MinkowskiPruning and `occupancy`, the three parts of ME's completion / reconstruction decoders (generative transpose ->
classifier -> pruning against an occupancy target).

A coordinate manager holds one map per tensor stride, so the result of either layer lives on a DERIVED manager of its own
(CoordinateManager.from_coordinates, as TensorField.splat() set the precedent): strided levels, convolutions, pooling and norms
work on it as on any other, while `ME.cat` / `+` with a tensor of the manager it came from is refused by the same-manager check."""
import math

import torch
import torch.nn as nn

from .._lib import check, lib
from . import functional as Fn
from ._rt import _f32c, _row_stride, _scratch, _stream
from .coords import CoordinateManager, CoordinateMapKey, _as_int
from .tensor import SparseTensor


def prune_compact(mask, coords, batch_size):
    """(kept int32 [k], old2new int32 [n], coordinates int32 [k, 4], batch offsets int32 [B + 1]) of the rows `mask` keeps
    (mink_prune_compact; one host read: the count k)."""
    L, n, dev = lib(), mask.shape[0], mask.device
    idx = torch.empty(2 * n + batch_size + 2, dtype=torch.int32, device=dev)  # [kept | old2new | offsets | total]
    kept, old2new, boff, total = idx[:n], idx[n : 2 * n], idx[2 * n : 2 * n + batch_size + 1], idx[2 * n + batch_size + 1 :]
    out_coords = torch.empty(n, 4, dtype=torch.int32, device=dev)
    ws = _scratch(int(L.mink_prune_workspace_bytes(n)), dev, "prune")
    check(L.mink_prune_compact(mask.data_ptr(), coords.data_ptr(), n, batch_size, kept.data_ptr(), old2new.data_ptr(),
                               out_coords.data_ptr(), boff.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    k = int(total.item())
    return kept[:k], old2new, out_coords[:k], boff


class PruneFunction(torch.autograd.Function):
    """y = x[kept] (mink_prune_gather); backward dX[i] = dY[old2new[i]] for a kept row and zeros for a pruned one, every row
    written once (mink_prune_gather_bwd)."""

    @staticmethod
    def forward(ctx, x, kept, old2new):
        x = _f32c(x)
        n_out, C = kept.shape[0], x.shape[1]
        y = torch.empty(n_out, C, dtype=torch.float32, device=x.device)
        check(lib().mink_prune_gather(x.data_ptr(), _row_stride(x), x.shape[0], C, kept.data_ptr(), n_out, y.data_ptr(), C, _stream()))
        ctx.old2new, ctx.n_out = old2new, n_out
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        n_in, C = ctx.old2new.shape[0], gy.shape[1]
        gx = torch.empty(n_in, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_prune_gather_bwd(gy.data_ptr(), _row_stride(gy), ctx.n_out, C, ctx.old2new.data_ptr(), n_in, gx.data_ptr(), C,
                                          _stream()))
        return gx, None, None


class MinkowskiPruning(nn.Module):
    """ME.MinkowskiPruning: `forward(x, mask)` keeps the rows of `x` where the bool `mask` [len(x)] is True, in their order, at
    the same tensor stride, on a derived manager that holds exactly those rows.  A sample may lose every voxel: the batch
    count stays and its `batch_offsets` range is empty (global pooling gives it a zero row).

    Deviation from ME: a mask that keeps NOTHING raises ValueError (ME returns an empty tensor; a manager here holds no empty
    map)."""

    def forward(self, input, mask):
        n = len(input)
        if not isinstance(mask, torch.Tensor) or mask.dtype != torch.bool:
            raise ValueError(f"MinkowskiPruning: the mask must be a bool tensor, not {getattr(mask, 'dtype', type(mask).__name__)}")
        if mask.dim() != 1 or mask.shape[0] != n:
            raise ValueError(f"MinkowskiPruning: a mask of shape {tuple(mask.shape)} for a tensor of {n} rows (one entry per row)")
        if mask.device != input.F.device:
            raise ValueError(f"MinkowskiPruning: the mask is on {mask.device}, the tensor on {input.F.device}")
        m, key = input.coordinate_manager, input.coordinate_map_key
        ts = key.get_tensor_stride()[0]
        assert m.has_level(ts)
        B = m.batch_size()
        kept, old2new, coords, boff = prune_compact(mask.contiguous(), m.get_coordinates(key), B)
        if kept.shape[0] == 0:
            raise ValueError("MinkowskiPruning: the mask keeps no row (a coordinate manager holds no empty map)")
        out = PruneFunction.apply(input.F, kept, old2new)
        return SparseTensor(out, CoordinateMapKey(ts), CoordinateManager.from_coordinates(coords, ts, B, batch_offsets=boff))


class _Fp32PointwiseFunction(Fn.PointwiseConvolutionFunction):
    """The pointwise path of the 1x1x1 convolutions with its weight gradient held to fp32 in every set_conv_math mode."""

    @staticmethod
    def backward(ctx, gy):
        old = Fn.set_conv_math("fp32")
        try:
            return Fn.PointwiseConvolutionFunction.backward(ctx, gy)
        finally:
            Fn.set_conv_math(old)


def generate_children(coords, ts):
    """int32 [8 n, 4]: the children of the rows coords[n, 4] at the even tensor stride `ts`, row 8 p + k = child k of parent p
    (mink_generate_children)."""
    n = coords.shape[0]
    children = torch.empty(8 * n, 4, dtype=torch.int32, device=coords.device)
    check(lib().mink_generate_children(coords.data_ptr(), n, ts, children.data_ptr(), _stream()))
    return children


class MinkowskiGenerativeConvolutionTranspose(nn.Module):
    """ME.MinkowskiGenerativeConvolutionTranspose for kernel_size == stride == 2: every input voxel p at tensor stride ts
    (even) spawns its 8 children p + kernel_offsets(2, ts / 2)[k] at ts / 2, whether or not anything was there before, and
    out[8 p + k] = x[p] @ kernel[k] (+ bias) -- the orientation of MinkowskiConvolutionTranspose (a coarse row at c feeds the
    fine row at c + offset k).  Rows are parent-major, so the whole operator is ONE product [n, Cin] x [Cin, 8 Cout] viewed
    as [8 n, Cout]: it takes the pointwise path of the 1x1x1 convolutions, in fp32 in every set_conv_math mode, and no
    neighbour table is built.  kernel: (8, Cin, Cout), init U(+-1/sqrt(Cout * 8)) like MinkowskiConvolutionTranspose."""

    def __init__(self, in_channels, out_channels, kernel_size=2, stride=2, dilation=1, bias=False, dimension=3):
        super().__init__()
        ks = list(kernel_size) if isinstance(kernel_size, (list, tuple)) else [kernel_size]
        st = list(stride) if isinstance(stride, (list, tuple)) else [stride]
        dl = list(dilation) if isinstance(dilation, (list, tuple)) else [dilation]
        if any(int(k) != 2 for k in ks) or any(int(s) != 2 for s in st) or any(int(d) != 1 for d in dl) or dimension != 3:
            raise ValueError(f"MinkowskiGenerativeConvolutionTranspose(kernel_size={kernel_size!r}, stride={stride!r}, "
                             f"dilation={dilation!r}, dimension={dimension!r}): only kernel_size == stride == 2, dilation == 1, "
                             "dimension == 3 is implemented")
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.dilation, self.dimension, self.kernel_volume = 2, 2, 1, 3, 8
        self.kernel = nn.Parameter(torch.empty(8, in_channels, out_channels))
        self.bias = nn.Parameter(torch.empty(1, out_channels)) if bias else None
        stdv = 1.0 / math.sqrt(out_channels * 8)
        with torch.no_grad():
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def forward(self, input):
        m, key = input.coordinate_manager, input.coordinate_map_key
        ts = _as_int(key.get_tensor_stride())
        if ts % 2:
            raise ValueError(f"MinkowskiGenerativeConvolutionTranspose: the input is at tensor stride {ts}; children live at half of "
                             "an even tensor stride")
        assert m.has_level(ts)
        x, n = _f32c(input.F), len(input)
        w = self.kernel.permute(1, 0, 2).reshape(self.in_channels, 8 * self.out_channels)  # [Cin, 8 Cout]: column block k = kernel[k]
        if n >= 4096 and self.kernel.requires_grad and torch.is_grad_enabled():  # (the row threshold of the 1x1x1 convolutions)
            out = _Fp32PointwiseFunction.apply(x, w, lambda m=m, k=key: m.identity_table(k))
        else:
            out = x.mm(w)
        out = out.view(8 * n, self.out_channels)
        if self.bias is not None:
            out = out + self.bias
        # children stay inside the 16-bit key range (see csrc/generate.hip): the build below cannot report a range error
        children = generate_children(m.get_coordinates(key), ts)
        return SparseTensor(out, CoordinateMapKey(ts // 2), CoordinateManager.from_coordinates(children, ts // 2, m.batch_size()))

    def extra_repr(self):
        return f"in={self.in_channels}, out={self.out_channels}, kernel_size=2, stride=2"


_ZERO_OFFSET = None


def occupancy(out, target):
    """bool [len(out)]: True where `out`'s coordinate is a voxel of `target`'s coordinate map at `out`'s tensor stride -- ME's
    `get_target` idiom (`cm.stride` then `kernel_map(..., kernel_size=1)`) for maps on different managers.  The level is made
    with `stride()` from `target`'s own when the manager does not hold it yet; the look-up is one probe per row of
    `target`'s hash map (mink_kernel_map with the single zero offset) and costs no host synchronisation of its own."""
    global _ZERO_OFFSET
    import ctypes

    ts, tts = _as_int(out.tensor_stride), _as_int(target.tensor_stride)
    tm = target.coordinate_manager
    if not tm.has_level(ts):
        if ts % tts:
            raise ValueError(f"occupancy: the target at tensor stride {tts} has no level at tensor stride {ts}")
        tm.stride(target.coordinate_map_key, ts // tts)
    tkeys, tvals, cap = tm.hash_map(ts)
    tm._sync_lazy()
    om = out.coordinate_manager
    assert om.has_level(ts)
    coords, n = om.get_coordinates(out.coordinate_map_key), len(out)
    if _ZERO_OFFSET is None:
        _ZERO_OFFSET = (ctypes.c_int32 * 3)(0, 0, 0)
    row = torch.empty(n, 1, dtype=torch.int32, device=coords.device)
    check(lib().mink_kernel_map(tkeys.data_ptr(), tvals.data_ptr(), cap, coords.data_ptr(), n, _ZERO_OFFSET, 1, row.data_ptr(), None,
                                _stream()))
    return row.view(n) >= 0
