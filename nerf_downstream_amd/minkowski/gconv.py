"""Grouped convolution over a neighbour table (csrc/gconv.hip)."""
import torch

from .._lib import check, lib
from ._rt import _f32c, _scratch, _stream


def gconv(x, w, nbr, groups, cg_in, cg_out, w_transposed=False, flip_k=False):
    """y[r, g cg_out + o] = sum_k sum_c x[nbr[r, k], g cg_in + c] w[k, g, c, o] (mink_gconv_fwd); `w` is the packed forward
    kernel [K, G, ci, co], read as [K, G, cg_out, cg_in] when w_transposed (the data gradient, cg_in / cg_out exchanged)."""
    n_out, K = nbr.shape
    assert x.shape[1] == groups * cg_in and w.numel() == K * groups * cg_in * cg_out, "gconv: x / w do not fit (K, G, cg_in, cg_out)"
    y = torch.empty(n_out, groups * cg_out, dtype=torch.float32, device=x.device)
    check(lib().mink_gconv_fwd(x.data_ptr(), x.shape[0], x.stride(0), w.data_ptr(), int(w_transposed), int(flip_k), nbr.data_ptr(),
                               n_out, K, groups, cg_in, cg_out, y.data_ptr(), y.stride(0), _stream()))
    return y


def gconv_wgrad(x, dy, nbr, groups, cg_in, cg_out):
    """dW[k, g, c, o] = sum_r x[nbr[r, k], g cg_in + c] dy[r, g cg_out + o] (mink_gconv_wgrad), row blocks added in a fixed order."""
    L = lib()
    n_out, K = nbr.shape
    dw = torch.empty(K, groups, cg_in, cg_out, dtype=torch.float32, device=x.device)
    ws = _scratch(L.mink_gconv_wgrad_workspace_bytes(n_out, K, groups, cg_in, cg_out), x.device, "gconv")
    check(L.mink_gconv_wgrad(x.data_ptr(), x.shape[0], x.stride(0), dy.data_ptr(), dy.stride(0), nbr.data_ptr(), n_out, K, groups,
                             cg_in, cg_out, dw.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    return dw


class GroupedConvolutionFunction(torch.autograd.Function):
    """apply(x, kernel [K, G, cg_in, cg_out], table_fn, same_map): a convolution over a neighbour table whose G groups do not
    mix (the 3x3 layers of ResNeXt).  `table_fn(transposed)` returns (nbr, nbr_t, ...) lazily and `same_map` has the meaning
    they have in functional.ConvolutionFunction.  fp32 whatever set_conv_math says; the backward is the data gradient, then the
    weight gradient, on the current stream, without atomics."""

    @staticmethod
    def forward(ctx, x, kernel, table_fn, same_map):
        x, w = _f32c(x), _f32c(kernel)
        K, G, ci, co = w.shape
        nbr = table_fn(False)[0]
        assert nbr.shape[1] == K, f"grouped convolution: a table of {nbr.shape[1]} offsets for a kernel of {K}"
        ctx.save_for_backward(x, w)
        ctx.table_fn, ctx.same_map, ctx.nbr = table_fn, same_map, nbr
        return gconv(x, w, nbr, G, ci, co)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        K, G, ci, co = w.shape
        gy = _f32c(gy)
        gx = gw = None
        if ctx.needs_input_grad[0]:
            if ctx.same_map:  # stride 1: nbr_t[i][k] == nbr[i][K-1-k]
                gx = gconv(gy, w, ctx.nbr, G, co, ci, w_transposed=True, flip_k=True)
            else:
                gx = gconv(gy, w, ctx.table_fn(True)[1], G, co, ci, w_transposed=True)
        if ctx.needs_input_grad[1]:
            gw = gconv_wgrad(x, gy, ctx.nbr, G, ci, co)
        return gx, gw, None, None
