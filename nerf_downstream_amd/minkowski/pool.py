"""Pooling over neighbour tables and over the samples of a batch (csrc/pool.hip)."""
import torch

from .._lib import check, lib
from ._rt import _check_offsets, _f32c, _row_stride, _scratch, _stream


class SumPoolFunction(torch.autograd.Function):
    """MinkowskiSumPooling(kernel==stride) (reference resnet.py:62-64; A9)."""

    @staticmethod
    def forward(ctx, x, nbr, in2out):
        x = _f32c(x)
        n_out, K = nbr.shape
        C = x.shape[1]
        y = torch.empty(n_out, C, dtype=torch.float32, device=x.device)
        check(lib().mink_pool_sum_fwd(x.data_ptr(), x.stride(0), C, nbr.data_ptr(), n_out, K, y.data_ptr(), _stream()))
        ctx.in2out, ctx.n_in = in2out, x.shape[0]
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        C = gy.shape[1]
        gx = torch.empty(ctx.n_in, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_pool_sum_bwd(gy.data_ptr(), C, ctx.in2out.data_ptr(), ctx.n_in, gx.data_ptr(), _stream()))
        return gx, None, None


class MaxPoolFunction(torch.autograd.Function):
    """Max pooling over a neighbour table (windows may overlap); `nbr_t` = the transposed table."""

    @staticmethod
    def forward(ctx, x, nbr, nbr_t):
        x = _f32c(x)
        n_out, K = nbr.shape
        C = x.shape[1]
        y = torch.empty(n_out, C, dtype=torch.float32, device=x.device)
        arg = torch.empty(n_out, C, dtype=torch.int32, device=x.device)
        check(lib().mink_pool_max_fwd(x.data_ptr(), C, nbr.data_ptr(), n_out, K, y.data_ptr(), arg.data_ptr(), _stream()))
        ctx.save_for_backward(arg, nbr_t)
        ctx.n_in = x.shape[0]
        return y

    @staticmethod
    def backward(ctx, gy):
        arg, nbr_t = ctx.saved_tensors
        gy = _f32c(gy)
        C = gy.shape[1]
        gx = torch.empty(ctx.n_in, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_pool_max_bwd(gy.data_ptr(), arg.data_ptr(), C, nbr_t.data_ptr(), ctx.n_in, nbr_t.shape[1], gx.data_ptr(), _stream()))
        return gx, None, None


class _LocalPoolFunction(torch.autograd.Function):
    """Sum (MODE 0) or average (MODE 1) pooling over a neighbour table whose windows may overlap (csrc/pool.hip); `nbr_t` =
    the transposed table the backward gathers through.  The average divides by the number of present inputs of the window."""

    MODE = 0

    @classmethod
    def _forward(cls, ctx, x, nbr, nbr_t):
        x = _f32c(x)
        n_out, K = nbr.shape
        C = x.shape[1]
        y = torch.empty(n_out, C, dtype=torch.float32, device=x.device)
        cnt = torch.empty(max(n_out, 1), dtype=torch.int32, device=x.device)
        check(lib().mink_pool_local_fwd(x.data_ptr(), _row_stride(x), C, nbr.data_ptr(), n_out, K, cls.MODE,
                                        y.data_ptr(), cnt.data_ptr(), _stream()))
        ctx.save_for_backward(cnt)
        ctx.nbr_t, ctx.n_in = nbr_t, x.shape[0]  # (not a saved tensor: the manager's tables share one arena, see InstanceNormFunction)
        ctx.mark_non_differentiable(cnt)
        return y, cnt

    @classmethod
    def _backward(cls, ctx, gy):
        (cnt,) = ctx.saved_tensors
        gy = _f32c(gy)
        C = gy.shape[1]
        gx = torch.empty(ctx.n_in, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_pool_local_bwd(gy.data_ptr(), C, ctx.nbr_t.data_ptr(), ctx.n_in, ctx.nbr_t.shape[1], cls.MODE,
                                        cnt.data_ptr(), gx.data_ptr(), _stream()))
        return gx, None, None


class AvgPoolFunction(_LocalPoolFunction):
    """ME.MinkowskiAvgPooling: (y, cnt) = AvgPoolFunction.apply(x, nbr, nbr_t); cnt[o] = present inputs of window o (int32)."""

    MODE = 1

    @staticmethod
    def forward(ctx, x, nbr, nbr_t):
        return AvgPoolFunction._forward(ctx, x, nbr, nbr_t)

    @staticmethod
    def backward(ctx, gy, _gcnt=None):
        return AvgPoolFunction._backward(ctx, gy)


class OverlapSumPoolFunction(_LocalPoolFunction):
    """ME.MinkowskiSumPooling with kernel_size != stride: the average's kernels without the division; also returns cnt."""

    MODE = 0

    @staticmethod
    def forward(ctx, x, nbr, nbr_t):
        return OverlapSumPoolFunction._forward(ctx, x, nbr, nbr_t)

    @staticmethod
    def backward(ctx, gy, _gcnt=None):
        return OverlapSumPoolFunction._backward(ctx, gy)


class SparseMaxPoolFunction(torch.autograd.Function):
    """ME.MinkowskiMaxPooling over a sparse neighbour table: (y, arg) with arg[o][c] = the input row of the maximum (the lowest
    kernel offset wins a tie); a window with no present entry gives 0 / -1.  (MaxPoolFunction above is the dense 2-D
    baseline's: C % 4 == 0 and -inf for an empty window.)"""

    @staticmethod
    def forward(ctx, x, nbr, nbr_t):
        x = _f32c(x)
        n_out, K = nbr.shape
        C = x.shape[1]
        y = torch.empty(n_out, C, dtype=torch.float32, device=x.device)
        arg = torch.empty(n_out, C, dtype=torch.int32, device=x.device)
        check(lib().mink_pool_local_max_fwd(x.data_ptr(), _row_stride(x), C, nbr.data_ptr(), n_out, K,
                                            y.data_ptr(), arg.data_ptr(), _stream()))
        ctx.save_for_backward(arg)
        ctx.nbr_t, ctx.n_in = nbr_t, x.shape[0]
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, gy, _garg=None):
        (arg,) = ctx.saved_tensors
        gy = _f32c(gy)
        C = gy.shape[1]
        gx = torch.empty(ctx.n_in, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_pool_local_max_bwd(gy.data_ptr(), arg.data_ptr(), C, ctx.nbr_t.data_ptr(), ctx.n_in, ctx.nbr_t.shape[1],
                                            gx.data_ptr(), _stream()))
        return gx, None, None


class GlobalMaxPoolFunction(torch.autograd.Function):
    """ME.MinkowskiGlobalMaxPooling: (y, arg) = apply(x, boff); y[b][c] = max over the rows of sample b, arg[b][c] = the lowest
    row of x attaining it (0 / -1 for an empty sample).  `boff`: the manager's int32 [B+1] device offsets, never read by the
    host; two launches forward, one backward whatever B is (csrc/pool.hip)."""

    @staticmethod
    def forward(ctx, x, boff):
        L = lib()
        x = _f32c(x)
        B = _check_offsets(boff)
        n, C = x.shape
        y = torch.empty(B, C, dtype=torch.float32, device=x.device)
        arg = torch.empty(B, C, dtype=torch.int32, device=x.device)
        ws = _scratch(L.mink_global_pool_workspace_bytes(n, C, B), x.device, "gpool")
        check(L.mink_global_max_fwd(x.data_ptr(), n, _row_stride(x), C, boff.data_ptr(), B, y.data_ptr(),
                                    arg.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        ctx.save_for_backward(arg)
        ctx.boff, ctx.n = boff, n
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, gy, _garg=None):
        (arg,) = ctx.saved_tensors
        gy = _f32c(gy)
        B, C = gy.shape
        gx = torch.empty(ctx.n, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_global_max_bwd(gy.data_ptr(), arg.data_ptr(), ctx.n, C, ctx.boff.data_ptr(), B, gx.data_ptr(), _stream()))
        return gx, None


class GlobalSumPoolFunction(torch.autograd.Function):
    """ME.MinkowskiGlobalSumPooling: y[b] = sum of the rows of sample b (accumulated in double, rounded once); dx[i] = dy[b]."""

    @staticmethod
    def forward(ctx, x, boff):
        L = lib()
        x = _f32c(x)
        B = _check_offsets(boff)
        n, C = x.shape
        y = torch.empty(B, C, dtype=torch.float32, device=x.device)
        ws = _scratch(L.mink_global_pool_workspace_bytes(n, C, B), x.device, "gpool")
        check(L.mink_global_sum_fwd(x.data_ptr(), n, _row_stride(x), C, boff.data_ptr(), B, y.data_ptr(),
                                    ws.data_ptr(), ws.numel(), _stream()))
        ctx.boff, ctx.n = boff, n
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        B, C = gy.shape
        gx = torch.empty(ctx.n, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_global_sum_bwd(gy.data_ptr(), ctx.n, C, ctx.boff.data_ptr(), B, gx.data_ptr(), _stream()))
        return gx, None


class GlobalAvgPoolFunction(torch.autograd.Function):
    """MinkowskiGlobalAvgPooling (reference resnet.py:15-22,175; A10)."""

    @staticmethod
    def forward(ctx, x, boff):
        x = _f32c(x)
        B, C = boff.numel() - 1, x.shape[1]
        y = torch.empty(B, C, dtype=torch.float32, device=x.device)
        check(lib().mink_global_avg_fwd(x.data_ptr(), C, boff.data_ptr(), B, y.data_ptr(), _stream()))
        ctx.boff, ctx.n = boff, x.shape[0]
        return y

    @staticmethod
    def backward(ctx, gy):
        gy = _f32c(gy)
        B, C = gy.shape
        gx = torch.empty(ctx.n, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_global_avg_bwd(gy.data_ptr(), C, ctx.boff.data_ptr(), B, ctx.n, gx.data_ptr(), _stream()))
        return gx, None
