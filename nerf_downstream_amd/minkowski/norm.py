"""Batch, instance, layer, power and cross-rank batch normalisation of feature rows, each optionally fused with the residual
add and ReLU that follow it (csrc/batchnorm.hip, csrc/norm.hip, csrc/powernorm.hip)."""
import torch

from .._lib import CONSTANTS, check, lib
from . import streams
from ._rt import _check_offsets, _f32c, _ptr, _scratch, _stream

PN_MAX_C = CONSTANTS["MINK_PN_MAX_C"]  # the widest layer the PowerNorm kernels take


# -------------------------------------------------------------------------- batch norm
def _bn_statistics(L, x, n, C, eps, momentum, running_mean, running_var, partial):
    """mean / invstd of the batch (+ running-stat update): from the producer's column partials
    when it supplied them, else by a reduction pass over x."""
    dev = x.device
    mean = torch.empty(C, dtype=torch.float32, device=dev)
    invstd = torch.empty(C, dtype=torch.float32, device=dev)
    mom = momentum if running_mean is not None else 0.0
    if partial is not None:
        check(
            L.mink_bn_stats_from_partials(
                partial.data_ptr(), partial.shape[0], n, C, eps, mom, mean.data_ptr(), invstd.data_ptr(),
                _ptr(running_mean), _ptr(running_var), _stream(),
            )
        )
    else:
        ws = _scratch(L.mink_bn_workspace_bytes(n, C), dev, "bn")
        check(
            L.mink_bn_stats(
                x.data_ptr(), n, C, eps, mom, mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean), _ptr(running_var),
                ws.data_ptr(), ws.numel(), _stream(),
            )
        )
    return mean, invstd


class BatchNormFunction(torch.autograd.Function):
    """BatchNorm1d over the rows of F, optionally fused with the residual add and ReLU that
    follow it in the reference block (modules/resnet_block.py:53-69; A8)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, residual, relu, partial=None):
        L = lib()
        x = _f32c(x)
        n, C = x.shape
        dev = x.device
        if residual is not None:
            residual = _f32c(residual)
        y = torch.empty_like(x)
        if training:
            mean = torch.empty(C, dtype=torch.float32, device=dev)
            invstd = torch.empty(C, dtype=torch.float32, device=dev)
            if partial is None:
                ws = _scratch(L.mink_bn_workspace_bytes(n, C), dev, "bn")
                check(
                    L.mink_bn_fwd(
                        x.data_ptr(), n, C, eps, momentum if running_mean is not None else 0.0, gamma.data_ptr(), beta.data_ptr(),
                        _ptr(residual), int(relu), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean),
                        _ptr(running_var), ws.data_ptr(), ws.numel(), _stream(),
                    )
                )
            else:
                # statistics partials from the producing convolution: finalize + apply, one launch when the partial rows are few
                check(
                    L.mink_bn_apply_from_partials(
                        x.data_ptr(), n, C, partial.data_ptr(), partial.shape[0], eps, momentum if running_mean is not None else 0.0,
                        gamma.data_ptr(), beta.data_ptr(), _ptr(residual), int(relu), y.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                        _ptr(running_mean), _ptr(running_var), _stream(),
                    )
                )
        else:
            mean = running_mean.float()
            invstd = torch.rsqrt(running_var.float() + eps)
            check(
                L.mink_bn_apply(
                    x.data_ptr(), n, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                    _ptr(residual), int(relu), y.data_ptr(), _stream(),
                )
            )
        ctx.save_for_backward(x, y if relu else None, mean, invstd, gamma)
        ctx.training, ctx.relu, ctx.has_res = training, relu, residual is not None
        ctx.beta = beta  # only as the key of its gradient slot under data parallelism
        return y

    @staticmethod
    def backward(ctx, gy):
        L = lib()
        x, y, mean, invstd, gamma = ctx.saved_tensors
        gy = _f32c(gy)
        n, C = x.shape
        dev = x.device
        if not ctx.training:  # eval-mode BN is an affine map; rarely differentiated
            g = torch.where(y > 0, gy, torch.zeros_like(gy)) if ctx.relu else gy  # (0 where masked, whatever gy holds)
            xhat = (x - mean) * invstd
            return (g * (gamma * invstd), (g * xhat).sum(0), g.sum(0), None, None, None, None, None,
                    g if ctx.has_res else None, None, None)
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if ctx.has_res else None
        views = streams.sink_views(gamma, ctx.beta) if ctx.needs_input_grad[1] and ctx.needs_input_grad[2] else None
        if views is not None:
            dgamma, dbeta = views
        else:
            dgamma = torch.empty(C, dtype=torch.float32, device=dev)
            dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        ws = _scratch(L.mink_bn_workspace_bytes(n, C), dev, "bn")
        check(
            L.mink_bn_bwd(
                gy.data_ptr(), x.data_ptr(), _ptr(y), n, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(),
                int(ctx.relu), gx.data_ptr(), _ptr(gres), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
            )
        )
        if views is not None:  # written in place into the reducer's buffer: nothing for autograd to accumulate
            sink = streams.grad_sink()
            sink.ready(gamma), sink.ready(ctx.beta)
            return gx, None, None, None, None, None, None, None, gres, None, None
        return gx, dgamma, dbeta, None, None, None, None, None, gres, None, None


class InstanceNormFunction(torch.autograd.Function):
    """Per-sample, per-channel normalisation of F (ME.MinkowskiInstanceNorm) with the residual add and ReLU of
    BatchNormFunction: sample b owns rows [offsets[b], offsets[b+1]) -- `offsets` is the manager's int32 [B+1] device
    tensor and is never read by the host.  Three launches forward, four backward, whatever B is (csrc/norm.hip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, offsets, eps, residual, relu):
        L = lib()
        x = _f32c(x)
        n, C = x.shape
        dev = x.device
        B = _check_offsets(offsets)
        gamma, beta = _f32c(gamma).reshape(-1), _f32c(beta).reshape(-1)
        if residual is not None:
            residual = _f32c(residual)
        y = torch.empty_like(x)
        mean = torch.empty(B, C, dtype=torch.float32, device=dev)
        invstd = torch.empty(B, C, dtype=torch.float32, device=dev)
        ws = _scratch(L.mink_in_workspace_bytes(n, C, B), dev, "in")
        check(
            L.mink_in_fwd(
                x.data_ptr(), n, C, offsets.data_ptr(), B, eps, gamma.data_ptr(), beta.data_ptr(), _ptr(residual), int(relu),
                y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
            )
        )
        ctx.save_for_backward(x, y if relu else None, mean, invstd, gamma)
        # (not a saved tensor: the manager carves its index tensors out of one arena, so a later carve-out next to the offsets
        #  bumps the version counter they share without touching them)
        ctx.offsets = offsets
        ctx.relu, ctx.has_res = relu, residual is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        L = lib()
        x, y, mean, invstd, gamma = ctx.saved_tensors
        offsets = ctx.offsets
        gy = _f32c(gy)
        n, C = x.shape
        dev = x.device
        B = offsets.numel() - 1
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if ctx.has_res else None
        dgamma = torch.empty(C, dtype=torch.float32, device=dev)
        dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        ws = _scratch(L.mink_in_workspace_bytes(n, C, B), dev, "in")
        check(
            L.mink_in_bwd(
                gy.data_ptr(), x.data_ptr(), _ptr(y), n, C, offsets.data_ptr(), B, mean.data_ptr(), invstd.data_ptr(),
                gamma.data_ptr(), int(ctx.relu), gx.data_ptr(), _ptr(gres), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(),
                ws.numel(), _stream(),
            )
        )
        return gx, dgamma, dbeta, None, None, gres, None


class LayerNormFunction(torch.autograd.Function):
    """torch.nn.LayerNorm(C) over the channels of every row of F (ME.MinkowskiLayerNorm), 1 <= C <= 512, with the residual
    add and ReLU of BatchNormFunction: one launch forward, two backward (csrc/norm.hip)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps, residual, relu):
        L = lib()
        x = _f32c(x)
        n, C = x.shape
        dev = x.device
        gamma, beta = _f32c(gamma).reshape(-1), _f32c(beta).reshape(-1)
        if residual is not None:
            residual = _f32c(residual)
        y = torch.empty_like(x)
        mean = torch.empty(n, dtype=torch.float32, device=dev)
        invstd = torch.empty(n, dtype=torch.float32, device=dev)
        check(
            L.mink_ln_fwd(
                x.data_ptr(), n, C, eps, gamma.data_ptr(), beta.data_ptr(), _ptr(residual), int(relu), y.data_ptr(),
                mean.data_ptr(), invstd.data_ptr(), _stream(),
            )
        )
        ctx.save_for_backward(x, y if relu else None, mean, invstd, gamma)
        ctx.relu, ctx.has_res = relu, residual is not None
        return y

    @staticmethod
    def backward(ctx, gy):
        L = lib()
        x, y, mean, invstd, gamma = ctx.saved_tensors
        gy = _f32c(gy)
        n, C = x.shape
        dev = x.device
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if ctx.has_res else None
        dgamma = torch.empty(C, dtype=torch.float32, device=dev)
        dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        ws = _scratch(L.mink_ln_workspace_bytes(n, C), dev, "ln")
        check(
            L.mink_ln_bwd(
                gy.data_ptr(), x.data_ptr(), _ptr(y), n, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), int(ctx.relu),
                gx.data_ptr(), _ptr(gres), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
            )
        )
        return gx, dgamma, dbeta, None, gres, None


class SyncBatchNormFunction(torch.autograd.Function):
    """BatchNorm with statistics over all ranks (ME.MinkowskiSyncBatchNorm, reference
    train.py:106-107): per-channel (sum x, sum x^2, rows) are all-reduced between the reduction and
    the apply pass; backward all-reduces (sum g, sum g*xhat).  Parameter gradients stay local
    sums -- the data-parallel gradient all-reduce averages them like every other gradient."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, momentum, eps, residual, relu, group):
        import torch.distributed as dist

        L = lib()
        x = _f32c(x)
        n, C = x.shape
        dev = x.device
        if residual is not None:
            residual = _f32c(residual)
        buf = torch.empty(2 * C + 1, dtype=torch.float64, device=dev)
        buf[2 * C] = float(n)
        ws = _scratch(L.mink_bn_workspace_bytes(n, C), dev, "bn")
        check(L.mink_bn_reduce(0, x.data_ptr(), None, None, n, C, None, None, buf.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
        dist.all_reduce(buf, group=group)
        mean = torch.empty(C, dtype=torch.float32, device=dev)
        invstd = torch.empty(C, dtype=torch.float32, device=dev)
        check(
            L.mink_bn_stats_from_sums(
                buf.data_ptr(), buf[2 * C :].data_ptr(), C, eps, momentum if running_mean is not None else 0.0,
                mean.data_ptr(), invstd.data_ptr(), _ptr(running_mean), _ptr(running_var), _stream(),
            )
        )
        y = torch.empty_like(x)
        check(
            L.mink_bn_apply(
                x.data_ptr(), n, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                _ptr(residual), int(relu), y.data_ptr(), _stream(),
            )
        )
        ctx.save_for_backward(x, y if relu else None, mean, invstd, gamma, buf[2 * C :].clone())
        ctx.relu, ctx.has_res, ctx.group = relu, residual is not None, group
        return y

    @staticmethod
    def backward(ctx, gy):
        import torch.distributed as dist

        L = lib()
        x, y, mean, invstd, gamma, n_total = ctx.saved_tensors
        gy = _f32c(gy)
        n, C = x.shape
        dev = x.device
        sums = torch.empty(2 * C, dtype=torch.float64, device=dev)
        ws = _scratch(L.mink_bn_workspace_bytes(n, C), dev, "bn")
        check(
            L.mink_bn_reduce(1, gy.data_ptr(), x.data_ptr(), _ptr(y), n, C, mean.data_ptr(), invstd.data_ptr(),
                             sums.data_ptr(), ws.data_ptr(), ws.numel(), _stream())
        )
        dbeta, dgamma = sums[:C].float(), sums[C:].float()  # local sums: averaged later with the other grads
        dist.all_reduce(sums, group=ctx.group)
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if ctx.has_res else None
        tmp = torch.empty(2 * C, dtype=torch.float32, device=dev)
        check(
            L.mink_bn_bwd_from_sums(
                gy.data_ptr(), x.data_ptr(), _ptr(y), n, C, sums.data_ptr(), n_total.data_ptr(), mean.data_ptr(),
                invstd.data_ptr(), gamma.data_ptr(), int(ctx.relu), gx.data_ptr(), _ptr(gres), tmp.data_ptr(), _stream(),
            )
        )
        return gx, dgamma, dbeta, None, None, None, None, gres, None, None


class BNReLUSumPoolFunction(torch.autograd.Function):
    """relu(BN(x)) summed over the 2^3 children of every coarse voxel, in one pass over x
    (reference resnet.py:58-64: bn1 -> relu -> pool).  The normalised fine-level tensor -- the
    largest activation of the network -- is never written; backward recomputes the ReLU mask."""

    @staticmethod
    def forward(ctx, x, gamma, beta, running_mean, running_var, training, momentum, eps, nbr, in2out, partial=None):
        L = lib()
        x = _f32c(x)
        n, C = x.shape
        dev = x.device
        if training:
            mean, invstd = _bn_statistics(L, x, n, C, eps, momentum, running_mean, running_var, partial)
        else:
            mean = running_mean.float()
            invstd = torch.rsqrt(running_var.float() + eps)
        n_out, K = nbr.shape
        y = torch.empty(n_out, C, dtype=torch.float32, device=dev)
        check(
            L.mink_bn_relu_pool_fwd(
                x.data_ptr(), C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), nbr.data_ptr(),
                n_out, K, y.data_ptr(), _stream(),
            )
        )
        ctx.save_for_backward(x, mean, invstd, gamma, beta)
        ctx.in2out, ctx.training = in2out, training
        return y

    @staticmethod
    def backward(ctx, gy):
        if not ctx.training:
            raise NotImplementedError("fused bn+relu+pool backward needs batch statistics (training mode)")
        L = lib()
        x, mean, invstd, gamma, beta = ctx.saved_tensors
        gy = _f32c(gy)
        n, C = x.shape
        gx = torch.empty_like(x)
        dgamma = torch.empty(C, dtype=torch.float32, device=x.device)
        dbeta = torch.empty(C, dtype=torch.float32, device=x.device)
        ws = _scratch(L.mink_bn_workspace_bytes(n, C), x.device, "bn")
        check(
            L.mink_bn_relu_pool_bwd(
                gy.data_ptr(), x.data_ptr(), n, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                ctx.in2out.data_ptr(), gx.data_ptr(), dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
            )
        )
        return gx, dgamma, dbeta, None, None, None, None, None, None, None, None


class PowerNormFunction(torch.autograd.Function):
    """PowerNorm over the rows of F (the reference's MaskPowerNorm behind MinkowskiPowerNorm, csrc/powernorm.hip) with the
    residual add and ReLU of BatchNormFunction.  `running_phi`, `ema_gz` (fp32, C elements) and `iters` (int64 [1]) are the
    module's device buffers: the kernels bump the counter, pick the warm-up branch and update the buffers themselves, so
    neither forward nor backward reads anything back.  The backward is PowerNorm's approximate derivative (it updates
    `ema_gz`), followed by the exact derivative of the group scaling.  Kept for backward beside x (and y under a fused
    ReLU): the row scale [n, groups] and two [C] vectors."""

    @staticmethod
    def forward(ctx, x, weight, bias, running_phi, ema_gz, iters, training, eps, alpha_fwd, alpha_bkw, warmup_iters, groups,
                residual, relu):
        L = lib()
        x = _f32c(x)
        n, C = x.shape
        dev = x.device
        groups = int(groups)
        if groups < 1 or C % groups:
            raise ValueError(f"PowerNorm: {C} channels are not divisible into {groups} groups")
        if C > PN_MAX_C:
            raise ValueError(f"PowerNorm: {C} channels, the kernels take at most {PN_MAX_C}")
        if training and n == 0:
            raise ValueError("PowerNorm in training mode needs at least one row: an empty batch has no second moment "
                             "(running_phi would become NaN)")
        weight, bias = _f32c(weight).reshape(-1), _f32c(bias).reshape(-1)
        if residual is not None:
            residual = _f32c(residual)
        y = torch.empty_like(x)
        ctx.training, ctx.relu, ctx.has_res = bool(training), bool(relu), residual is not None
        ctx.eps, ctx.alpha_bkw, ctx.groups = float(eps), float(alpha_bkw), groups
        ctx.ema_gz = ema_gz  # (a buffer the backward updates in place, not a saved tensor: its version moves with every step)
        if n == 0:
            ctx.save_for_backward(x, None, None, None, None, weight)
            return y
        rscale = torch.empty(n, groups, dtype=torch.float32, device=dev)
        scale = torch.empty(C, dtype=torch.float32, device=dev)
        if training:
            _check_pn_buffers(running_phi, ema_gz, iters, C, dev)
            var = torch.empty(C, dtype=torch.float32, device=dev)
            ws = _scratch(L.mink_pn_workspace_bytes(n, C, groups), dev, "pn")
            check(
                L.mink_pn_fwd(
                    x.data_ptr(), C, n, C, groups, eps, alpha_fwd, int(warmup_iters), weight.data_ptr(), bias.data_ptr(),
                    _ptr(residual), int(relu), y.data_ptr(), rscale.data_ptr(), var.data_ptr(), scale.data_ptr(),
                    running_phi.data_ptr(), iters.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
                )
            )
        else:
            _check_pn_buffers(running_phi, None, None, C, dev)
            var = None
            check(
                L.mink_pn_apply(
                    x.data_ptr(), C, n, C, groups, eps, running_phi.data_ptr(), weight.data_ptr(), bias.data_ptr(), _ptr(residual),
                    int(relu), y.data_ptr(), rscale.data_ptr(), scale.data_ptr(), _stream(),
                )
            )
        ctx.save_for_backward(x, y if relu else None, rscale, var, scale, weight)
        return y

    @staticmethod
    def backward(ctx, gy):
        L = lib()
        x, y, rscale, var, scale, weight = ctx.saved_tensors
        gy = _f32c(gy)
        n, C = x.shape
        dev = x.device
        none = (None,) * 9
        if n == 0:
            z = torch.zeros(C, dtype=torch.float32, device=dev)
            return (torch.empty_like(x), z, z.clone(), *none, torch.empty_like(x) if ctx.has_res else None, None)
        gx = torch.empty_like(x)
        gres = torch.empty_like(x) if ctx.has_res else None
        dweight = torch.empty(C, dtype=torch.float32, device=dev)
        dbias = torch.empty(C, dtype=torch.float32, device=dev)
        ws = _scratch(L.mink_pn_workspace_bytes(n, C, ctx.groups), dev, "pn")
        check(
            L.mink_pn_bwd(
                gy.data_ptr(), x.data_ptr(), C, _ptr(y), n, C, ctx.groups, ctx.eps, ctx.alpha_bkw, int(ctx.training),
                rscale.data_ptr(), _ptr(var), scale.data_ptr(), weight.data_ptr(), int(ctx.relu),
                ctx.ema_gz.data_ptr() if ctx.training else None, gx.data_ptr(), _ptr(gres), dweight.data_ptr(), dbias.data_ptr(),
                ws.data_ptr(), ws.numel(), _stream(),
            )
        )
        return (gx, dweight, dbias, *none, gres, None)


def _check_pn_buffers(running_phi, ema_gz, iters, C, dev):
    """The PowerNorm state the kernels write through raw pointers: fp32 / int64, contiguous, on the features' device."""
    for name, t, dtype, numel in (("running_phi", running_phi, torch.float32, C), ("ema_gz", ema_gz, torch.float32, C),
                                  ("iters", iters, torch.int64, 1)):
        if t is None:
            continue
        if t.dtype != dtype or t.numel() != numel or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"PowerNorm: buffer {name} must be a contiguous {dtype} tensor of {numel} elements on {dev}, "
                             f"got {t.dtype} {tuple(t.shape)} on {t.device}")
