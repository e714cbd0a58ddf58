"""PAConv on the rows of a field (csrc/paconv.hip): the score-weighted neighbour aggregation of the reference's
co3d_3d/src/models/paconv (feat_trans_dgcnn / feat_trans_pointnet followed by the assign_score_withk CUDA extension) and its
ScoreNet.

The reference transforms every point by the whole weight bank first (two [B, N, M, O] tensors) and then gathers and contracts
them with the scores, one thread per output element with atomicAdd.  Here the neighbour sum runs in input space,
    A[i, m] = sum_j s[i, j, m] x[idx[i, j]],   S[i, m] = sum_j s[i, j, m],   y[i] = sum_m (A[i, m] Wn_m - S[i, m] x[i] Wc_m),
and the bank meets [A | S x] in one dense GEMM: the gather reads M O / Cin times fewer bytes, no [n, M, O] and no [n, k, ., O]
tensor exists forward or backward, and every sum has a fixed order (two runs give the same bits).  With the bank
`matrice` [Cin', M O] viewed as [Cin', M, O]:
    "dgcnn"    Cin' = 2 Cin, K1 = matrice[:Cin], K2 = matrice[Cin:]:  Wn_m = K1_m + K2_m, Wc_m = K1_m   (sum s (P[j] - C[i]))
    "pointnet" Cin' = Cin:                                            Wn_m = 2 K_m,       Wc_m = K_m    (sum s (2 P[j] - P[i]))"""
import torch
import torch.nn as nn

from .._lib import check, lib
from ._rt import _f32c, _stream
from .field import lazy_index_csr
from .graph import MAX_K, _xwt
from .norm import BatchNormFunction

MAX_M = 16  # MINK_PACONV_MAX_M
MODES = ("dgcnn", "pointnet")


def _bank(matrice, M, cin, mode):
    """[Wn ; -Wc] as [2 M Cin, O], rows ordered (m, c) like the columns of [A | S x]."""
    K = matrice.detach().float().reshape(-1, M, matrice.shape[1] // M)
    if mode == "dgcnn":
        Wn, Wc = K[:cin] + K[cin:], K[:cin]
    else:
        Wn, Wc = 2.0 * K, K
    rows = lambda W: W.permute(1, 0, 2).reshape(M * cin, -1)  # noqa: E731
    return torch.cat([rows(Wn), -rows(Wc)], 0).contiguous()


class PAConvFunction(torch.autograd.Function):
    """y [n, O] = apply(x [n, Cin], matrice [Cin', M O], scores [n, k, M], idx int32 [n, k], mode, csr_fn); differentiable in x,
    matrice and scores.  Kept for the backward: x, the scores, [A | S x] and S.  `csr_fn` returns the incoming-edge lists of
    idx (lazy_index_csr(idx, n): built on the first backward; layers that share idx may share it)."""

    @staticmethod
    def forward(ctx, x, matrice, scores, idx, mode, csr_fn):
        L = lib()
        x, s = _f32c(x), _f32c(scores)
        n, cin = x.shape
        assert idx.is_cuda and idx.dtype == torch.int32 and idx.is_contiguous() and idx.dim() == 2 and idx.shape[0] == n, \
            "paconv: idx int32 [n, k] on the device"
        k = idx.shape[1]
        assert s.dim() == 3 and s.shape[:2] == (n, k), "paconv: scores [n, k, M] beside idx [n, k]"
        M = s.shape[2]
        assert matrice.dim() == 2 and matrice.shape[0] == (2 * cin if mode == "dgcnn" else cin) and matrice.shape[1] % M == 0, \
            f"paconv: matrice [{'2 Cin' if mode == 'dgcnn' else 'Cin'}, M O] beside x [n, Cin] and scores [n, k, M]"
        W = _bank(matrice, M, cin, mode)
        Z = torch.empty(n, 2, M, cin, dtype=torch.float32, device=x.device)  # [A | S x]
        S = torch.empty(n, M, dtype=torch.float32, device=x.device)
        check(L.mink_paconv_gather(x.data_ptr(), s.data_ptr(), idx.data_ptr(), n, k, M, cin, Z.data_ptr(), Z.data_ptr() + 4 * M * cin,
                                   2 * M * cin, S.data_ptr(), _stream()))
        y = _xwt(Z.view(n, -1), W.t().contiguous()) if n else x.new_zeros(0, W.shape[1])
        ctx.save_for_backward(x, s, idx, Z, S, W)
        ctx.mode, ctx.bank_shape = mode, matrice.shape
        ctx.csr_fn = csr_fn if csr_fn is not None else lazy_index_csr(idx, n)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = lib()
        x, s, idx, Z, S, W = ctx.saved_tensors
        g = _f32c(gy)
        n, cin = x.shape
        k, M, O = idx.shape[1], s.shape[2], W.shape[1]
        ldz = 2 * M * cin
        gx = gm = gs = None
        if n and (ctx.needs_input_grad[0] or ctx.needs_input_grad[2]):
            dZ = _xwt(g, W)  # [dA | dCX] = g [Wn ; -Wc]^T
            dA, dCX = dZ.data_ptr(), dZ.data_ptr() + 4 * M * cin
            if ctx.needs_input_grad[2]:
                gs = torch.empty_like(s)
                check(L.mink_paconv_score_bwd(dA, dCX, ldz, x.data_ptr(), idx.data_ptr(), n, k, M, cin, gs.data_ptr(), _stream()))
            if ctx.needs_input_grad[0]:
                members, seg = ctx.csr_fn()
                gx = torch.empty_like(x)
                check(L.mink_paconv_scatter_bwd(dA, dCX, ldz, s.data_ptr(), S.data_ptr(), members.data_ptr(), seg.data_ptr(), n, k, M, cin,
                                                gx.data_ptr(), _stream()))
        if ctx.needs_input_grad[1]:
            dW = Z.view(n, -1).t().mm(g).view(2, M, cin, O)  # (dWn, -dWc)
            dWn, dWc = dW[0], -dW[1]
            dK = torch.cat([dWn + dWc, dWn], 1) if ctx.mode == "dgcnn" else 2.0 * dWn + dWc
            gm = dK.permute(1, 0, 2).reshape(ctx.bank_shape)
        return gx, gm, gs, None, None, None


def paconv(x, matrice, scores, idx, mode="dgcnn", aggregate="sum", csr_fn=None):
    """One PAConv layer on the feature matrix x [n, Cin]: what the reference computes by `feat_trans_dgcnn` +
    `assign_score_withk` (mode "dgcnn") or `feat_trans_pointnet` + `assign_score_withk_halfkernel` (mode "pointnet") -> [n, O].
    `matrice` keeps the reference's [Cin', M O] layout, `scores` [n, k, M] is its (B, N, K, M) with n = B N, `idx` int32 [n, k]
    holds global rows as graph.knn returns them (a slot outside [0, n) contributes nothing).  Only aggregate = "sum" exists."""
    if aggregate != "sum":
        raise ValueError(f"paconv: aggregate = {aggregate!r} is not implemented (the reference's models use 'sum' only)")
    if mode not in MODES:
        raise ValueError(f"paconv: mode = {mode!r}, expected one of {MODES}")
    if not 1 <= scores.shape[-1] <= MAX_M or not 1 <= idx.shape[-1] <= MAX_K:
        raise ValueError(f"paconv: M = {scores.shape[-1]} of 1..{MAX_M}, k = {idx.shape[-1]} of 1..{MAX_K}")
    return PAConvFunction.apply(x, matrice, scores, idx, mode, csr_fn)


def batch_norm_rows(x, bn, relu):
    """`bn` (an nn.BatchNorm*d: gamma, beta, running statistics, step counter) over the rows of x [rows, C], fused with ReLU."""
    training = bn.training or not bn.track_running_stats
    if training and bn.track_running_stats:
        bn.num_batches_tracked += 1
    momentum = bn.momentum if bn.momentum is not None else 1.0 / max(float(bn.num_batches_tracked), 1.0)
    return BatchNormFunction.apply(x, bn.weight, bn.bias, bn.running_mean, bn.running_var, training, momentum, bn.eps, None, bool(relu))


def scorenet_input(xyz, idx):
    """[n k, 6] = (x_j - x_i, x_j) for the slots of idx [n, k] over the points xyz [n, 3] (reference get_scorenet_input)."""
    n, k = idx.shape
    nb = xyz[idx.long().clamp_(0, max(n - 1, 0))]
    return torch.cat([nb - xyz[:, None, :], nb], 2).reshape(n * k, -1)


class ScoreNet(nn.Module):
    """The reference's ScoreNet (util/PAConv_util.py:73-137) on row matrices: the parameters are its nn.Conv2d / nn.BatchNorm2d
    modules under its names (`mlp_convs_hidden.{i}`, `mlp_bns_hidden.{i}`, `mlp_convs_nohidden`; the last `mlp_bns_hidden`
    entry exists but is unused when last_bn is False), the 1x1 convolutions run as matmuls over the n k rows and the batch
    norms over those rows.  forward(rows [n k, in_channel], k) -> scores [n, k, M]."""

    def __init__(self, in_channel, out_channel, hidden_unit=(16,), last_bn=False):
        super().__init__()
        self.hidden_unit = list(hidden_unit) if hidden_unit else []
        self.last_bn = last_bn
        self.mlp_convs_hidden = nn.ModuleList()
        self.mlp_bns_hidden = nn.ModuleList()
        if not self.hidden_unit:
            self.mlp_convs_nohidden = nn.Conv2d(in_channel, out_channel, 1, bias=not last_bn)
            if last_bn:
                self.mlp_bns_nohidden = nn.BatchNorm2d(out_channel)
        else:
            widths = [in_channel] + self.hidden_unit
            for a, b in zip(widths[:-1], widths[1:]):
                self.mlp_convs_hidden.append(nn.Conv2d(a, b, 1, bias=False))
                self.mlp_bns_hidden.append(nn.BatchNorm2d(b))
            self.mlp_convs_hidden.append(nn.Conv2d(widths[-1], out_channel, 1, bias=not last_bn))
            self.mlp_bns_hidden.append(nn.BatchNorm2d(out_channel))

    @staticmethod
    def _conv(conv, rows):
        w = conv.weight.view(conv.weight.shape[0], -1)
        return rows.mm(w.t()) if conv.bias is None else torch.addmm(conv.bias, rows, w.t())

    def forward(self, rows, k, calc_scores="softmax", bias=0):
        if not self.hidden_unit:
            out = self._conv(self.mlp_convs_nohidden, rows)
            if self.last_bn:
                out = batch_norm_rows(out, self.mlp_bns_nohidden, False)
        else:
            out = rows
            for conv, bn in zip(self.mlp_convs_hidden[:-1], self.mlp_bns_hidden[:-1]):
                out = batch_norm_rows(self._conv(conv, out), bn, True)
            out = self._conv(self.mlp_convs_hidden[-1], out)
            if self.last_bn:
                out = batch_norm_rows(out, self.mlp_bns_hidden[-1], False)
        if calc_scores == "softmax":
            out = torch.softmax(out, 1) + bias
        elif calc_scores == "sigmoid":
            out = torch.sigmoid(out) + bias
        else:
            raise ValueError(f"ScoreNet: calc_scores = {calc_scores!r} is not implemented")
        return out.reshape(-1, k, out.shape[1])
