"""Point stage of the point classifiers (csrc/field.hip): per-voxel means of point rows, the gather-and-concatenate back to
the points, batch offsets of a field, and the CSR grouping that the fixed-order backward passes read."""
import ctypes

import torch

from .._lib import check, lib
from ._rt import _f32c, _ptr, _row_stride, _stream


def index_csr(idx, n_rows):
    """The entries i of idx (flattened) grouped by their target idx[i]: (members int32 [idx.numel()], seg int32 [n_rows + 1]),
    members ascending inside a segment (a stable sort, as tensor.py::_field_members), the absent entries (idx < 0) behind the
    last segment.  For an interpolation map imap[n][8] a member is the pair q * 8 + c.  No host read-back."""
    flat = idx.reshape(-1).long()
    key = torch.where(flat >= 0, flat, torch.full_like(flat, n_rows))
    members = torch.sort(key, stable=True).indices.int()
    seg = torch.zeros(n_rows + 1, dtype=torch.int32, device=idx.device)
    seg[1:] = torch.cumsum(torch.bincount(key, minlength=n_rows + 1)[:n_rows], 0).int()
    return members, seg


def lazy_index_csr(idx, n_rows):
    """A `csr_fn` for InterpolationFunction / FieldGatherCatFunction: builds index_csr(idx, n_rows) on the first call and keeps it."""
    box = []

    def get():
        if not box:
            box.append(index_csr(idx, n_rows))
        return box[0]

    return get


def segment_mean(x, members, seg, n_out):
    x = _f32c(x)
    y = torch.empty(n_out, x.shape[1], dtype=torch.float32, device=x.device)
    check(
        lib().mink_segment_mean(x.data_ptr(), x.stride(0), x.shape[1], members.data_ptr(), seg.data_ptr(), n_out, y.data_ptr(), _stream())
    )
    return y


class SegmentMeanFunction(torch.autograd.Function):
    """TensorField.sparse() of learned per-point features (reference fcnn.py:143-144,165): y[u] = the mean of x[members[j]]
    over j in [seg[u], seg[u+1]) (mink_segment_mean, input-row order); backward dx[members[j]] = dy[u] / count[u]
    (mink_segment_mean_bwd: every input row written once, no atomics)."""

    @staticmethod
    def forward(ctx, x, members, seg, n_out):
        ctx.members, ctx.seg, ctx.n_in = members, seg, x.shape[0]  # (not saved tensors: views of the manager's arena, see InstanceNormFunction)
        return segment_mean(x, members, seg, n_out)

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        n_out, C = gy.shape
        gx = torch.empty(ctx.n_in, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_segment_mean_bwd(gy.data_ptr(), _row_stride(gy), C, ctx.members.data_ptr(), ctx.seg.data_ptr(),
                                          n_out, ctx.members.numel(), ctx.n_in, gx.data_ptr(), C, _stream()))
        return gx, None, None, None


class FieldGatherCatFunction(torch.autograd.Function):
    """y = cat_s x_s[idx_s] along the columns, apply(maps, x_0, ..., x_(S-1)), 1 <= S <= 8 (mink_field_gather_cat: one launch,
    every output row written once; idx < 0 -> zeros) -- `y.slice(x)` at a tensor stride beyond 1 (S == 1) and
    ME.cat(y1.slice(x), ..., y4.slice(x)) of reference fcnn.py:158-163.  `maps[s]` = (idx_s int32 [n], csr_fn_s); the backward
    of source s is mink_segment_sum over the column slice of dy with csr_fn_s() = index_csr(idx_s, rows of x_s), built on
    the first backward: fixed order, no atomics, bitwise the backward of the separate slices under torch.cat."""

    @staticmethod
    def forward(ctx, maps, *xs):
        assert 1 <= len(xs) <= 8 and len(maps) == len(xs), "field_gather_cat: 1..8 sources, one (idx, csr_fn) each"
        xs = [_f32c(x) for x in xs]
        n, S = maps[0][0].numel(), len(xs)
        for (idx, _), x in zip(maps, xs):
            assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == n and x.dim() == 2, \
                "field_gather_cat: idx int32 [n] on the device beside x [rows, C]"
        widths = [x.shape[1] for x in xs]
        y = torch.empty(n, sum(widths), dtype=torch.float32, device=xs[0].device)
        check(lib().mink_field_gather_cat(
            S, (ctypes.c_void_p * S)(*[_ptr(x) for x in xs]), (ctypes.c_int32 * S)(*[_row_stride(x) for x in xs]),
            (ctypes.c_int64 * S)(*[x.shape[0] for x in xs]), (ctypes.c_int32 * S)(*widths),
            (ctypes.c_void_p * S)(*[m[0].data_ptr() for m in maps]), n, y.data_ptr(), y.shape[1], _stream()))
        ctx.maps, ctx.widths, ctx.rows = maps, widths, [x.shape[0] for x in xs]
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        L, ld, off, out = lib(), gy.shape[1], 0, []
        for s, ((_, csr_fn), C, rows) in enumerate(zip(ctx.maps, ctx.widths, ctx.rows)):
            gx = None
            if ctx.needs_input_grad[1 + s]:
                members, seg = csr_fn()
                gx = torch.empty(rows, C, dtype=torch.float32, device=gy.device)
                check(L.mink_segment_sum(gy.data_ptr() + 4 * off, ld, C, members.data_ptr(), seg.data_ptr(), rows, gx.data_ptr(), _stream()))
            out.append(gx)
            off += C
        return (None, *out)


def field_batch_offsets(coords, B, sizes=None):
    """int32 [B + 1] row ranges of the batch indices 0..B-1 in the batch column of a field's float rows coords[n, 4]
    (mink_batch_offsets on the device); ValueError when the column is not non-decreasing (one read of the status word).
    `sizes`: a list that receives the B per-sample row counts, which arrive with that same read."""
    n = coords.shape[0]
    rows = torch.zeros(n, 4, dtype=torch.int32, device=coords.device)
    rows[:, 0] = coords[:, 0].detach().to(torch.int32)
    out = torch.zeros(B + 2, dtype=torch.int32, device=coords.device)  # [offsets | status]
    check(lib().mink_batch_offsets(rows.data_ptr(), n, B, out.data_ptr(), out[B + 1:].data_ptr(), _stream()))
    host = out.tolist()
    if host[B + 1] & 2:  # MINK_STATUS_UNSORTED
        raise ValueError("global pooling of a TensorField: batch indices must be non-decreasing (use ME.utils.sparse_collate); "
                         "the rows are not sorted for you")
    if sizes is not None:
        sizes[:] = [host[b + 1] - host[b] for b in range(B)]
    return out[: B + 1]
