"""Trilinear interpolation and splat of sparse tensors (csrc/interp.hip)."""
import torch

from .._lib import check, lib
from ._rt import _f32c, _ptr, _stream


def _interp_gather(x, imap, w):
    x = _f32c(x)
    n_q, C = imap.shape[0], x.shape[1]
    y = torch.empty(n_q, C, dtype=torch.float32, device=x.device)
    check(lib().mink_interp_gather(_ptr(x), C, x.shape[0], C, imap.data_ptr(), w.data_ptr(), n_q, y.data_ptr(), _stream()))
    return y


def _interp_segsum(dy, w, members, seg, n_rows):
    dy = _f32c(dy)
    C = dy.shape[1]
    dx = torch.empty(n_rows, C, dtype=torch.float32, device=dy.device)
    check(lib().mink_interp_segsum(_ptr(dy), C, dy.shape[0], C, w.data_ptr(), members.data_ptr(), seg.data_ptr(), n_rows,
                                   members.numel(), dx.data_ptr(), _stream()))
    return dx


def _check_maps(imap, w):
    assert imap.is_cuda and imap.dtype == torch.int32 and imap.dim() == 2 and imap.shape[1] == 8 and imap.is_contiguous(), \
        "imap: a contiguous int32 [n, 8] device tensor"
    assert w.is_cuda and w.dtype == torch.float32 and w.shape == imap.shape and w.is_contiguous(), "w: float32 [n, 8] beside imap"


class InterpolationFunction(torch.autograd.Function):
    """ME.MinkowskiInterpolation [ME-recall of interpolation_map_weight; parity unpinned, ME is absent]:
    y[q] = sum_c w[q][c] * x[imap[q][c]] (mink_interp_gather); the gradient goes to x only, none to the coordinates:
    dx[i] = the sum of w[q][c] * dy[q] over the pairs with imap[q][c] = i (mink_interp_segsum: fixed order, no atomics).
    Only the maps are kept; `csr_fn()` -> (members, seg) of `field.index_csr(imap, rows of x)` is called on the first backward."""

    @staticmethod
    def forward(ctx, x, imap, w, csr_fn):
        _check_maps(imap, w)
        ctx.w, ctx.csr_fn, ctx.n_in = w, csr_fn, x.shape[0]  # (not saved tensors: a splat's imap is a view of its manager's arena, see InstanceNormFunction)
        return _interp_gather(x, imap, w)

    @staticmethod
    def backward(ctx, gy):
        members, seg = ctx.csr_fn()
        return _interp_segsum(gy, ctx.w, members, seg, ctx.n_in), None, None, None


class SplatFunction(torch.autograd.Function):
    """TensorField.splat() [ME-recall of TensorField.splat; parity unpinned, ME is absent]: F_s[v] = the sum of
    w[p][c] * F[p] over the corners (p, c) that fall on voxel v -- the interpolation backward with all eight corners found
    (`csr` = field.index_csr(imap, n_rows)); its backward is the interpolation forward.  Only the maps are kept."""

    @staticmethod
    def forward(ctx, F, imap, w, csr, n_rows):
        _check_maps(imap, w)
        ctx.imap, ctx.w = imap, w
        return _interp_segsum(F, w, csr[0], csr[1], n_rows)

    @staticmethod
    def backward(ctx, gy):
        return _interp_gather(gy, ctx.imap, ctx.w), None, None, None, None
