"""Dynamic graph layers on the rows of a field (csrc/graph.hip): the per-sample k-nearest-neighbour graph in feature space
(`knn`; `knn_cross` with queries and candidates in two matrices, and distances) and the edge convolution of DGCNN (reference co3d_3d/src/models/mink/dgcnn.py:8-38,81-85) fused with its batch norm,
LeakyReLU(0.2) and the maximum over the k edges.

With W = [W1 | W2] the reference's 1x1 convolution of [x_j - x_i ; x_i] is e[i][j] = P[idx[i][j]] + Q[i] with P = X W1^T and
Q = X (W2 - W1)^T: two dense GEMMs with k times fewer FLOPs, and kernels that read P through the neighbour table.  No
n x n matrix and no edge-sized (n x k x C) tensor is ever formed, forward or backward."""
import torch

from .._lib import check, lib
from . import functional as Fn
from ._rt import _check_offsets, _f32c, _row_stride, _scratch, _stream
from .field import lazy_index_csr
from .norm import _bn_statistics

MAX_K, MAX_C = 64, 256  # MINK_KNN_MAX_K / MINK_KNN_MAX_C


def knn(x, batch_offsets, k):
    """idx int32 [n, k]: the global rows of the k rows of the same sample (batch_offsets int32 [B + 1] on the device) nearest
    to every row of x [n, C] in squared Euclidean distance, the row itself included; ascending distance, ties to the lower
    row.  Not differentiable.  Slots of a sample with fewer than k rows are -1 (see check_sample_sizes)."""
    B = _check_offsets(batch_offsets)
    x = x.detach()
    assert x.is_cuda and x.dim() == 2, "knn: x [n, C] on the device"
    if x.dtype != torch.float32 or x.stride(1) != 1:
        x = x.float().contiguous()
    n, C = x.shape
    idx = torch.empty(n, int(k), dtype=torch.int32, device=x.device)
    check(lib().mink_knn(x.data_ptr(), n, _row_stride(x), C, batch_offsets.data_ptr(), B, int(k), idx.data_ptr(), _stream()))
    return idx


def _rows_view(x, what):
    """A float32 [n, C] device matrix with unit column stride (a strided row view is kept: its stride(0) is the leading
    dimension the kernel takes); anything else is copied."""
    x = x.detach()
    assert x.is_cuda and x.dim() == 2, f"{what} [n, C] on the device"
    if x.dtype != torch.float32 or x.stride(1) != 1 or (x.shape[0] > 1 and x.stride(0) < x.shape[1]):
        x = x.float().contiguous()
    return x


def knn_cross(q, c, k=1, q_offsets=None, c_offsets=None, return_distance=False):
    """idx int32 [nq, k]: for every row of q [nq, C] the global rows of the k rows of c [nc, C], inside the same sample, nearest
    in squared Euclidean distance (csrc/graph.hip mink_knn_cross); ascending ranking score ||c_j||^2 - 2 q_i.c_j, ties to the
    lower row, -1 in the slots beyond the sample's candidates.  With `return_distance` also dist float32 [nq, k]: the squared
    distance of every chosen pair recomputed by direct differences (+inf at -1); its slots follow the ranking order, so
    neighbouring entries may be out of exact order by less than the ranking error.  Not differentiable.
    `q_offsets` / `c_offsets`: int32 [B + 1] device row ranges of the samples on either side; both None = one sample (the
    [0, n] offsets are built on the device, nothing is read back).  q and c may be strided row views (the xyz columns of an
    [n, 4] coordinate matrix, a row slice): stride(0) is passed as the leading dimension, nothing is copied."""
    q, c = _rows_view(q, "knn_cross: q"), _rows_view(c, "knn_cross: c")
    assert q.device == c.device and q.shape[1] == c.shape[1], "knn_cross: q [nq, C] and c [nc, C] on one device"
    (nq, C), nc = q.shape, c.shape[0]
    if (q_offsets is None) != (c_offsets is None):
        raise ValueError("knn_cross: give both q_offsets and c_offsets, or neither (one sample)")
    if q_offsets is None:
        both = torch.zeros(4, dtype=torch.int32, device=q.device)
        both[1], both[3] = nq, nc  # (host scalars written by fills: no read-back)
        q_offsets, c_offsets = both[:2], both[2:]
    B = _check_offsets(q_offsets)
    assert _check_offsets(c_offsets) == B, "knn_cross: q_offsets and c_offsets describe the same B samples"
    idx = torch.empty(nq, int(k), dtype=torch.int32, device=q.device)
    dist = torch.empty(nq, int(k), dtype=torch.float32, device=q.device) if return_distance else None
    check(lib().mink_knn_cross(q.data_ptr(), nq, _row_stride(q), c.data_ptr(), nc, _row_stride(c), C,
                               q_offsets.data_ptr(), c_offsets.data_ptr(), B, int(k), idx.data_ptr(),
                               dist.data_ptr() if return_distance else None, _stream()))
    return (idx, dist) if return_distance else idx


def check_sample_sizes(sizes, k):
    """ValueError for a sample with 0 < rows < k (the reference's `topk` fails there); an empty sample is allowed."""
    for b, nb in enumerate(sizes):
        if 0 < nb < k:
            raise ValueError(f"k-nearest-neighbour graph with k = {k}: sample {b} holds only {nb} points")


def _xwt(x, w):
    """x [n, Kd] @ w [N, Kd]^T: the fp32 matrix-core GEMM where its shape rules fit (Kd a multiple of 4), torch otherwise."""
    if x.shape[1] % 4 == 0 and x.shape[1] >= 4 and x.data_ptr() % 16 == 0 and w.data_ptr() % 16 == 0:
        return Fn.dense_xwt(x, w)
    return torch.matmul(x, w.t())


class EdgeConvFunction(torch.autograd.Function):
    """(y [n, Cout], arg uint8 [n, Cout]) = apply(x, W, gamma, beta, running_mean, running_var, idx, training, momentum, eps):
    y[i] = max_j lrelu_0.2(bn(W [x_idx[i][j] - x_i ; x_i])) with batch statistics over the n k edges (training; the running
    statistics are updated with that count and the unbiased variance) or the running statistics (eval); arg = the lowest slot
    attaining the maximum.  W: [Cout, 2 Cin] (or the conv weight [Cout, 2 Cin, 1, 1]).  Kept for the backward: P, Q, arg and the
    statistics.  The incoming-edge lists the backward sums over are built on the first backward."""

    @staticmethod
    def forward(ctx, x, W, gamma, beta, running_mean, running_var, idx, training, momentum, eps):
        L = lib()
        x = _f32c(x)
        n, cin = x.shape
        cout = W.shape[0]
        assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 2 and idx.shape[0] == n, \
            "edge_conv: idx int32 [n, k] on the device"
        assert W.numel() == cout * 2 * cin and n >= 1, "edge_conv: W [Cout, 2 Cin] beside x [n >= 1, Cin]"
        k = idx.shape[1]
        Wm = W.detach().reshape(cout, 2 * cin).float()
        W1 = Wm[:, :cin].contiguous()
        Wd = (Wm[:, cin:] - Wm[:, :cin]).contiguous()
        P, Q = _xwt(x, W1), _xwt(x, Wd)
        gamma, beta = _f32c(gamma.detach()), _f32c(beta.detach())
        if training:
            partial = torch.empty(L.mink_edge_stats_rows(n), 2, cout, dtype=torch.float64, device=x.device)
            check(L.mink_edge_stats(P.data_ptr(), Q.data_ptr(), idx.data_ptr(), n, k, cout, partial.data_ptr(), partial.numel() * 8,
                                    _stream()))
            mean, invstd = _bn_statistics(L, P, n * k, cout, eps, momentum, running_mean, running_var, partial)
        else:
            mean = running_mean.float().contiguous()
            invstd = torch.rsqrt(running_var.float() + eps)
        y = torch.empty(n, cout, dtype=torch.float32, device=x.device)
        arg = torch.empty(n, cout, dtype=torch.uint8, device=x.device)
        check(L.mink_edge_fwd(P.data_ptr(), Q.data_ptr(), idx.data_ptr(), n, k, cout, mean.data_ptr(), invstd.data_ptr(),
                              gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), arg.data_ptr(), _stream()))
        ctx.save_for_backward(x, W1, Wd, P, Q, arg, mean, invstd, gamma, beta, idx)
        ctx.training, ctx.w_shape = bool(training), W.shape
        ctx.csr_fn = lazy_index_csr(idx, n)
        ctx.mark_non_differentiable(arg)
        return y, arg

    @staticmethod
    def backward(ctx, gy, _garg=None):
        L = lib()
        x, W1, Wd, P, Q, arg, mean, invstd, gamma, beta, idx = ctx.saved_tensors
        gy = _f32c(gy)
        n, cout = gy.shape
        k = idx.shape[1]
        members, seg = ctx.csr_fn()
        dP, dQ = torch.empty_like(P), torch.empty_like(Q)
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
        ws = _scratch(L.mink_edge_bwd_workspace_bytes(n, cout), gy.device, "edge")
        check(L.mink_edge_bwd(gy.data_ptr(), P.data_ptr(), Q.data_ptr(), idx.data_ptr(), arg.data_ptr(), n, k, cout, mean.data_ptr(),
                              invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), int(ctx.training), members.data_ptr(),
                              seg.data_ptr(), dP.data_ptr(), dQ.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(),
                              ws.numel(), _stream()))
        gx = gw = None
        if ctx.needs_input_grad[0]:
            gx = torch.addmm(dP.mm(W1), dQ, Wd)
        if ctx.needs_input_grad[1]:
            gq = dQ.t().mm(x)  # = dW2
            gw = torch.cat([dP.t().mm(x) - gq, gq], 1).reshape(ctx.w_shape)
        return gx, gw, dgamma, dbeta, None, None, None, None, None, None


def edge_conv(x, weight, bn, idx):
    """The edge-convolution block of one DGCNN layer on the feature matrix x [n, Cin]: `weight` [Cout, 2 Cin(, 1, 1)] and `bn`,
    an nn.BatchNorm*d holding gamma, beta and the running statistics (its step counter is advanced as torch does)."""
    training = bn.training or not bn.track_running_stats
    if training and bn.track_running_stats:
        bn.num_batches_tracked += 1
    momentum = bn.momentum if bn.momentum is not None else 1.0 / max(float(bn.num_batches_tracked), 1.0)
    y, _ = EdgeConvFunction.apply(x, weight, bn.weight, bn.bias, bn.running_mean, bn.running_var, idx, training, momentum, bn.eps)
    return y
