"""Pointwise passes over feature rows: ReLU, the activations beyond it, and the add (csrc/elementwise.hip)."""
import torch

from .._lib import check, lib
from ._rt import _f32c, _ptr, _stream


def _eltwise(a, b, mode):
    y = torch.empty_like(a)
    check(lib().mink_eltwise(a.data_ptr(), _ptr(b), a.numel(), mode, y.data_ptr(), _stream()))
    return y


class ReLUFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        y = _eltwise(_f32c(x), None, 0)
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, gy):
        (y,) = ctx.saved_tensors
        return _eltwise(_f32c(gy), y, 1)


ACT_KINDS = {"leaky_relu": 1, "elu": 2, "celu": 3, "selu": 4, "gelu": 5, "prelu": 6}


class ActivationFunction(torch.autograd.Function):
    """Pointwise activations beyond ReLU (ME.MinkowskiLeakyReLU / ELU / CELU / SELU / GELU / PReLU; the reference's layer
    factory lists them at import, modules/common.py:36-43): out = f(x), backward gy * f'(x), one HIP pass each.  The
    PReLU weight gradient (a column sum of gy * min(x, 0)) is a torch reduction."""

    @staticmethod
    def forward(ctx, x, kind, alpha, slope):
        x = _f32c(x)
        y = torch.empty_like(x)
        C = 1 if slope is None or slope.numel() == 1 else x.shape[1]
        check(lib().mink_activation(x.data_ptr(), None, _ptr(slope), C, x.numel(), ACT_KINDS[kind], float(alpha), y.data_ptr(), _stream()))
        ctx.save_for_backward(x, slope)
        ctx.kind, ctx.alpha, ctx.C = kind, float(alpha), C
        return y

    @staticmethod
    def backward(ctx, gy):
        x, slope = ctx.saved_tensors
        gy = _f32c(gy)
        gx = torch.empty_like(x)
        check(lib().mink_activation(x.data_ptr(), gy.data_ptr(), _ptr(slope), ctx.C, x.numel(), ACT_KINDS[ctx.kind], ctx.alpha,
                                    gx.data_ptr(), _stream()))
        gslope = None
        if slope is not None and ctx.needs_input_grad[3]:
            t = gy * x.clamp(max=0)
            gslope = t.sum().reshape(1) if slope.numel() == 1 else t.sum(0)
        return gx, None, None, gslope


class AddFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        return _eltwise(_f32c(a), _f32c(b), 2)

    @staticmethod
    def backward(ctx, gy):
        return gy, gy
