"""The tails of the networks: classifier head and its loss (csrc/dense.hip), and the segmentation tail -- masked cross
entropy with its statistics, and the slice back to the points (csrc/seghead.hip)."""
import torch

from .._lib import check, lib
from . import streams
from ._rt import _f32c, _ptr, _scratch, _stream


# ----------------------------------------------------------------------- classifier head
class GlobalAvgLinearFunction(torch.autograd.Function):
    """logits = MinkowskiGlobalAvgPooling(x) @ kernel + bias in one launch each way (mink_head_forward/backward):
    the tail of the reference network, `self.final(self.glob_avg(out))` (models/mink/resnet.py:175-177)."""

    @staticmethod
    def forward(ctx, x, boff, kernel, bias):
        x = _f32c(x)
        B, C, ncls = boff.numel() - 1, x.shape[1], kernel.shape[1]
        pooled = torch.empty(B, C, dtype=torch.float32, device=x.device)
        logits = torch.empty(B, ncls, dtype=torch.float32, device=x.device)
        w = kernel.contiguous()
        check(lib().mink_head_forward(x.data_ptr(), boff.data_ptr(), B, C, w.data_ptr(), _ptr(bias), ncls, pooled.data_ptr(),
                                      logits.data_ptr(), _stream()))
        ctx.save_for_backward(pooled, w, boff)
        ctx.n, ctx.has_bias, ctx.bias_shape = x.shape[0], bias is not None, None if bias is None else bias.shape
        ctx.params = (kernel, bias) if (w is kernel and (bias is None or bias.is_contiguous())) else None
        return logits

    @staticmethod
    def backward(ctx, gl):
        pooled, w, boff = ctx.saved_tensors
        gl = _f32c(gl)
        B, C = pooled.shape
        ncls = w.shape[1]
        gx = torch.empty(ctx.n, C, dtype=torch.float32, device=gl.device) if ctx.needs_input_grad[0] else None
        # a data-parallel reducer's flat buffer as the gradient sink: the kernel writes dW / db in place (no accumulate launches)
        views = None
        sink = streams.grad_sink()
        if sink is not None and ctx.params is not None:
            views = streams.sink_views(*[p for p in ctx.params if p is not None])
        if views is not None:
            gw, gb = views[0], (views[1] if ctx.has_bias else None)
        else:
            gw = torch.empty_like(w)
            gb = torch.empty(ctx.bias_shape, dtype=torch.float32, device=gl.device) if ctx.has_bias else None
        check(lib().mink_head_backward(gl.data_ptr(), pooled.data_ptr(), w.data_ptr(), boff.data_ptr(), B, C, ncls, gw.data_ptr(),
                                       _ptr(gb), _ptr(gx), _stream()))
        if views is not None:
            for p in ctx.params:
                if p is not None:
                    sink.ready(p)
            return gx, None, None, None
        return gx, None, gw, gb


def global_avg_linear(x, batch_offsets, kernel, bias=None):
    return GlobalAvgLinearFunction.apply(x, batch_offsets, kernel, bias)


class SoftmaxCrossEntropyFunction(torch.autograd.Function):
    """F.cross_entropy(logits, labels) with its defaults (mean over the batch) as one launch each way."""

    @staticmethod
    def forward(ctx, logits, labels):
        logits = _f32c(logits)
        labels = labels.contiguous()
        assert labels.dtype == torch.int64 and labels.shape == (logits.shape[0],), "labels: int64 [B]"
        B, ncls = logits.shape
        prob = torch.empty_like(logits)
        loss = torch.empty((), dtype=torch.float32, device=logits.device)
        check(lib().mink_softmax_ce_forward(logits.data_ptr(), labels.data_ptr(), B, ncls, prob.data_ptr(), loss.data_ptr(), _stream()))
        ctx.save_for_backward(prob, labels)
        return loss

    @staticmethod
    def backward(ctx, g):
        prob, labels = ctx.saved_tensors
        g = _f32c(g)
        dl = torch.empty_like(prob)
        check(lib().mink_softmax_ce_backward(prob.data_ptr(), labels.data_ptr(), g.data_ptr(), prob.shape[0], prob.shape[1],
                                             dl.data_ptr(), _stream()))
        return dl, None


def cross_entropy(logits, labels):
    """Mean softmax cross-entropy; HIP kernels for device logits, torch otherwise (CPU oracle runs of the same trainer)."""
    if logits.is_cuda and logits.dim() == 2 and labels.dim() == 1:
        return SoftmaxCrossEntropyFunction.apply(logits, labels)
    return torch.nn.functional.cross_entropy(logits, labels)


# ------------------------------------------------------------------- segmentation tail
SEG_STATS_WORDS = 5  # mink_hip.h: double num, double den, int64 n_valid, n_ignored, n_bad


def seg_stats(stats):
    """The `stats` tensor of seg_cross_entropy read back (ONE device-to-host copy) -> dict(num, den, n_valid, n_ignored, n_bad)."""
    s = stats.cpu()
    num, den = s[:2].view(torch.float64).tolist()
    n_valid, n_ignored, n_bad = s[2:5].tolist()
    return {"num": num, "den": den, "n_valid": n_valid, "n_ignored": n_ignored, "n_bad": n_bad}


class SegCrossEntropyFunction(torch.autograd.Function):
    """F.cross_entropy(logits, labels, weight=, ignore_index=) over per-point logits [N, C] as one pass each way
    (mink_seg_ce_forward / backward).  Forward keeps 4 bytes per row (the log-sum-exp), not N x C probabilities, and
    hands back, from the same pass, the prediction, the confusion matrix and the label counts as non-differentiable
    extras: -> (loss, pred int32 [N] | None, hist int64 [C, C] | None, stats int64 [5], see seg_stats)."""

    @staticmethod
    def forward(ctx, logits, labels, weight, ignore_index, want_pred, want_hist):
        z = logits if (logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 2 and logits.stride(1) == 1
                       and logits.stride(0) >= logits.shape[1]) else _f32c(logits)
        n, C = z.shape
        if labels.dtype not in (torch.int64, torch.int32):
            labels = labels.long()
        labels = labels.contiguous()
        assert labels.shape == (n,), "labels: integer [N]"
        w = None if weight is None else _f32c(weight)
        assert w is None or w.shape == (C,), "weight: [C]"
        dev = z.device
        lse = torch.empty(n, dtype=torch.float32, device=dev)
        pred = torch.empty(n, dtype=torch.int32, device=dev) if want_pred else None
        hist = torch.empty(C, C, dtype=torch.int64, device=dev) if want_hist else None
        stats = torch.empty(SEG_STATS_WORDS, dtype=torch.int64, device=dev)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        L = lib()
        need = L.mink_seg_ce_workspace_bytes(n, C)
        if need < 0:
            raise ValueError(f"seg_cross_entropy: {C} classes (2 .. 128 are supported)")
        ws = _scratch(need, dev, "seg_ce")
        check(L.mink_seg_ce_forward(z.data_ptr(), z.stride(0) if n else C, labels.data_ptr(), int(labels.dtype == torch.int64), _ptr(w),
                                    int(ignore_index), n, C, lse.data_ptr(), _ptr(pred), _ptr(hist), stats.data_ptr(),
                                    loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        ctx.save_for_backward(z, labels, lse, stats, *([w] if w is not None else []))
        ctx.ignore_index = int(ignore_index)
        extras = [t for t in (pred, hist, stats) if t is not None]
        ctx.mark_non_differentiable(*extras)
        return loss, pred, hist, stats

    @staticmethod
    def backward(ctx, g, *_):
        z, labels, lse, stats, *w = ctx.saved_tensors
        w = w[0] if w else None
        g = _f32c(g)
        n, C = z.shape
        dz = torch.empty(n, C, dtype=torch.float32, device=z.device)
        check(lib().mink_seg_ce_backward(z.data_ptr(), z.stride(0) if n else C, labels.data_ptr(), int(labels.dtype == torch.int64),
                                         _ptr(w), ctx.ignore_index, lse.data_ptr(), stats.data_ptr(), g.data_ptr(), n, C,
                                         dz.data_ptr(), _stream()))
        return dz, None, None, None, None, None


def seg_cross_entropy(logits, labels, weight=None, ignore_index=-100, want_pred=False, want_hist=False):
    """Weighted / ignore-label mean cross entropy over per-point logits [N, C] -> (loss, pred, hist, stats).

    `pred` (argmax, lowest index on ties; None unless want_pred), `hist[label, pred]` over the valid rows (None unless
    want_hist) and `stats` (seg_stats(): the weighted sums and the counts of valid / ignored / bad labels) come out of
    the same pass.  A label that is neither `ignore_index` nor in [0, C) is COUNTED (n_bad) and left out, where torch's
    kernel aborts the process.  HIP kernels for device logits; torch otherwise (CPU oracle runs of the same trainer):
    there the loss is exactly F.cross_entropy's, and bad labels are masked before they reach it."""
    if logits.is_cuda and logits.dim() == 2 and labels.dim() == 1:
        return SegCrossEntropyFunction.apply(logits, labels, weight, ignore_index, want_pred, want_hist)
    import torch.nn.functional as F

    C = logits.shape[1]
    y = labels.long()
    ignored = y == ignore_index
    valid = (y >= 0) & (y < C) & ~ignored
    bad = ~valid & ~ignored
    safe = torch.where(bad, torch.full_like(y, ignore_index), y) if bool(bad.any()) else y
    loss = F.cross_entropy(logits, safe, weight=weight, ignore_index=ignore_index)
    with torch.no_grad():
        p = logits.argmax(1)
        pred = p.int() if want_pred else None
        hist = torch.bincount(C * y[valid] + p[valid], minlength=C * C).reshape(C, C) if want_hist else None
        wy = (weight.double()[y[valid]] if weight is not None else torch.ones(int(valid.sum()), dtype=torch.float64))
        den = wy.sum().reshape(1)
        stats = torch.cat([(loss.detach().double().reshape(1) * den).view(torch.int64), den.view(torch.int64),
                           torch.stack([valid.sum(), ignored.sum(), bad.sum()])])
    return loss, pred, hist, stats


class SliceFunction(torch.autograd.Function):
    """SparseTensor.slice(): y = x[inverse] (mink_rows_gather); backward = the sum of every voxel's member rows in input-row
    order (mink_segment_sum over the CSR pair TensorField.sparse() built): fixed order, no atomics."""

    @staticmethod
    def forward(ctx, x, inverse, members, seg):
        x = _f32c(x)
        n, C = inverse.numel(), x.shape[1]
        y = torch.empty(n, C, dtype=torch.float32, device=x.device)
        check(lib().mink_rows_gather(x.data_ptr(), x.stride(0), x.shape[0], C, inverse.data_ptr(), n, y.data_ptr(), _stream()))
        ctx.save_for_backward(members, seg)
        ctx.n_src = x.shape[0]
        return y

    @staticmethod
    def backward(ctx, gy):
        members, seg = ctx.saved_tensors
        gy = _f32c(gy)
        C = gy.shape[1]
        gx = torch.empty(ctx.n_src, C, dtype=torch.float32, device=gy.device)
        check(lib().mink_segment_sum(gy.data_ptr(), gy.stride(0), C, members.data_ptr(), seg.data_ptr(), ctx.n_src, gx.data_ptr(), _stream()))
        return gx, None, None, None


def slice_rows(x, inverse, members, seg):
    """x[inverse] with the native backward; inverse / members int32 [n], seg int32 [rows of x + 1]."""
    return SliceFunction.apply(x, inverse, members, seg)
