"""Positional encoding of coordinate columns (csrc/posenc.hip)."""
import torch

from .._lib import check, lib
from ._rt import _f32c, _stream


def positional_encoding(x, freq, phase, L, lo=0, hi=0):
    """mink_posenc_fwd: y[:, q] = sin(freq[q] * x[:, q // (2L)] + phase[q]) for q < Q = 2 L C, then the columns x[:, lo:hi]."""
    x = _f32c(x)
    n, C = x.shape
    width = 2 * L * C + hi - lo
    assert freq.is_cuda and phase.is_cuda and freq.dtype == phase.dtype == torch.float32 and freq.is_contiguous() \
        and phase.is_contiguous() and freq.numel() == phase.numel() == 2 * L * C, "positional_encoding: freq and phase are fp32 [2 L C]"
    y = torch.empty(n, width, dtype=torch.float32, device=x.device)
    check(lib().mink_posenc_fwd(x.data_ptr(), n, C, C, freq.data_ptr(), phase.data_ptr(), L, lo, hi, y.data_ptr(), width, _stream()))
    return y


class PositionalEncodingFunction(torch.autograd.Function):
    """apply(x, freq, phase, L, lo, hi) -> [n, 2 L C + hi - lo] (reference modules/encoding.py:181-209, which forms the same
    values as a sparse matrix product, an add and a sin).  Backward mink_posenc_bwd: one lane per (row, channel), fixed order,
    no atomics.  freq and phase are constants of the layer and get no gradient."""

    @staticmethod
    def forward(ctx, x, freq, phase, L, lo, hi):
        x = _f32c(x)
        ctx.save_for_backward(x, freq, phase)
        ctx.cfg = (L, lo, hi)
        return positional_encoding(x, freq, phase, L, lo, hi)

    @staticmethod
    def backward(ctx, gy):
        x, freq, phase = ctx.saved_tensors
        (L, lo, hi), gy = ctx.cfg, _f32c(gy)
        n, C = x.shape
        gx = torch.empty_like(x)
        check(lib().mink_posenc_bwd(gy.data_ptr(), gy.shape[1], x.data_ptr(), n, C, C, freq.data_ptr(), phase.data_ptr(), L, lo, hi,
                                    gx.data_ptr(), C, _stream()))
        return gx, None, None, None, None, None
