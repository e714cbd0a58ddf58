"""Autograd functions of the HIP backend: every forward/backward is a call into libmink_hip.so
(C ABI, include/mink_hip.h) on torch-owned device buffers and the current HIP stream.

Semantics follow SURVEY.md Appendix A (A6 convolution, A8 batch norm, A9 sum pooling,
A10 global average pooling); the reference call sites are cited on the modules.

This module holds the convolution path, its options and the benchmark's diagnostics: the names that tests, scripts and
the benchmark patch on it (`_FORCE_KSPLIT`, `gather_gemm`, `_PHASE_LOG`, `log_phase`) are read by the code right here.
Every other operator family lives in a module named after its .hip file (norm, eltwise, pool, head, interp, field, posenc,
attn, gconv), the stream orchestration in streams.py, the call helpers in _rt.py; the import block at the bottom
re-exports their public names, so `functional.<name>` keeps working for all of them.
"""
import ctypes
import re
import time

import torch

from .._lib import TimingEntry, check, lib
from . import streams
from ._rt import _f32c, _ptr, _scratch, _stream
from .norm import _bn_statistics
from .streams import current_stream, skew, stream_wait

# ------------------------------------------------------------------- matrix-core math
_MATH = {"fp32": 0, "f32": 0, "bf16": 1, "bf16x3": 3}


def set_conv_math(mode="fp32"):
    """Arithmetic of the convolution forward / input-gradient GEMMs: "fp32" (exact, default),
    "bf16" (bf16 MFMA operands, fp32 accumulate -- BASELINE config "bf16 mixed precision") or
    "bf16x3" (split-bf16, three products per step).  Tensors in HBM stay fp32; the weight
    gradient always runs in exact fp32, and so does every pass of a 5^3 / 7^3 convolution (K > 27, csrc/conv_bigk.hip) in
    every mode.  Returns the previous mode name."""
    if mode not in _MATH:
        raise ValueError(f"conv math {mode!r}: choose from {sorted(set(_MATH))}")
    old = lib().mink_conv_set_math(_MATH[mode])
    _PLAN_CACHE.clear()  # the split plan depends on which kernel the mode selects
    return {0: "fp32", 1: "bf16", 3: "bf16x3"}[old]


_STORAGE_B16 = False


def set_conv_storage(mode="fp32"):
    """HBM storage of the FULL-RESOLUTION stage of a Mink-ResNet trunk (input features and the stem convolution's
    output, three quarters of the activation bytes of a step): "fp32" (default) or "bf16".  "bf16" takes effect under
    `set_conv_math("bf16")` on the native trunk (minkowski/trunk.py); every tensor from the pooled level down, the
    parameters, their gradients and the batch-norm statistics stay fp32.  Returns the previous mode name."""
    global _STORAGE_B16
    if mode not in ("fp32", "bf16"):
        raise ValueError(f"conv storage {mode!r}: choose 'fp32' or 'bf16'")
    old, _STORAGE_B16 = _STORAGE_B16, mode == "bf16"
    return "bf16" if old else "fp32"


def rows_to_bf16(x):
    """bf16 copy [n, 32] (zero-padded) of fp32 rows with at most 32 channels (mink_rows_to_bf16) on the current stream."""
    xb = torch.empty(x.shape[0], 32, dtype=torch.bfloat16, device=x.device)
    check(lib().mink_rows_to_bf16(x.data_ptr(), x.shape[0], x.shape[1], x.stride(0), xb.data_ptr(), _stream()))
    return xb


def conv_math():
    """The current mode name of set_conv_math (read without changing it)."""
    return {0: "fp32", 1: "bf16", 3: "bf16x3"}[lib().mink_conv_get_math()]


# ---------------------------------------------------------------------- kernel timing
# bench.py measures the dominant kernel live with HIP events recorded on the launch stream.  The events are recorded
# inside the native library around each convolution call (mink_conv_timing), so the module-by-module path and the
# native trunk are instrumented alike.  HIP event records are not free on this stack (each one is a barrier packet),
# so the timed region instruments ONE kernel tag only; the warm-up instruments all.
_TIMING_MODE = 0     # 0 off, 1 every convolution launch, 2 only `_TIMING_ONLY`
_TIMING_ONLY = None
_TIMING_TABLES = {}  # warm-up (mode 1): data_ptr -> neighbour table, kept until the entries are fetched (pair counts)
_TIMING_PAIRS = {}   # tag -> {n_out: valid entries of its table}
_KINDS = ("fwd", "dgrad", "wgrad")


def _parse_tag(tag):
    kind, n_out, K, cin, cout = re.fullmatch(r"(\w+)\[(\d+)x(\d+):(\d+)->(\d+)\]", tag).groups()
    return _KINDS.index(kind), int(n_out), int(K), int(cin), int(cout)


def enable_kernel_timing(on=True, only=None, any_kind=False):
    """`only`: a tag "kind[n_out x K:cin->cout]" -- every launch of that kind / K / cin / cout is timed (`any_kind`: of that
    K / cin / cout, whatever the kind -- forward, data gradient and weight gradient of one layer)."""
    global _TIMING_MODE, _TIMING_ONLY
    L = lib()
    n = L.mink_conv_timing_fetch(None, 0)
    if n:  # drop entries nobody asked for
        L.mink_conv_timing_fetch((TimingEntry * n)(), n)
    _TIMING_TABLES.clear()
    if not on:
        _TIMING_MODE, _TIMING_ONLY = 0, None
        L.mink_conv_timing(0, 0, 0, 0, 0)
    elif only is None:
        _TIMING_MODE, _TIMING_ONLY = 1, None
        L.mink_conv_timing(1, 0, 0, 0, 0)
    else:
        kind, _, K, cin, cout = _parse_tag(only)
        _TIMING_MODE, _TIMING_ONLY = 2, only
        L.mink_conv_timing(2, -1 if any_kind else kind, K, cin, cout)


def note_table(*tables):
    """Warm-up instrumentation: keep the neighbour tables of timed launches alive so their pair counts can be read."""
    if _TIMING_MODE == 1:
        for t in tables:
            if t is not None:
                _TIMING_TABLES[t.data_ptr()] = t


def kernel_timings():
    """{tag: {"ms": [per-launch milliseconds], "meta": {kind, n_in, n_out, K, cin, cout, pairs (per launch)}}} of the
    launches timed since the last call (synchronises on their events)."""
    L = lib()
    n = L.mink_conv_timing_fetch(None, 0)
    out = {}
    if n == 0:
        return out
    buf = (TimingEntry * n)()
    n = L.mink_conv_timing_fetch(buf, n)
    for e in buf[:n]:
        tag = f"{_KINDS[e.kind]}[{e.n_out}x{e.K}:{e.cin}->{e.cout}]"
        pairs = _TIMING_PAIRS.setdefault(tag, {})
        t = _TIMING_TABLES.get(e.nbr)
        if t is not None and e.n_out not in pairs:
            # (the row count of the gathered operand is not an argument of a forward / data-gradient call: every row of
            # it is referenced by the table of the layers timed here, so it is the largest index + 1)
            pairs[e.n_out] = (int((t >= 0).sum().item()), e.n_in if e.n_in >= 0 else int(t.max().item()) + 1)
        pr, n_in = pairs.get(e.n_out, (None, e.n_in))
        ent = out.setdefault(tag, {"ms": [], "meta": {"kind": _KINDS[e.kind], "n_in": n_in, "n_out": e.n_out, "K": e.K,
                                                      "cin": e.cin, "cout": e.cout, "pairs": pr}})
        if e.ms >= 0:
            ent["ms"].append(e.ms)
    _TIMING_TABLES.clear()
    return out


_PHASE_LOG = None  # diagnostic (bench.py --timeline): [(name, timing event, host clock)] of every mark


def log_phase(name, stream):
    if _PHASE_LOG is not None:
        t = torch.cuda.Event(enable_timing=True)
        t.record(stream)
        _PHASE_LOG.append((name, t, time.perf_counter()))


# -------------------------------------------------------------------------- batch norm options
def set_bn_small(on=True):
    """Few-row layers of the native trunk: the one-launch batch norm + split-K sum (mink_bn_small_fwd / _bwd; csrc/
    batchnorm.hip).  Off: the trunk sequences exactly the kernels of the module-by-module path (the bitwise tests)."""
    return bool(lib().mink_bn_set_small(1 if on else 0))


def set_bn_fold(max_rows=0):
    """Batch-norm finalize inside the apply pass (mink_bn_apply_from_partials, mink_bn_bwd) when the producer left at most
    `max_rows` partial rows (0: never; at most 128).  Returns the previous limit."""
    return int(lib().mink_bn_set_fold(int(max_rows)))


# ------------------------------------------------------------------------- convolution
_FORCE_KSPLIT = 0  # benchmarking hook (scripts/kbench.py ksweep)

def gather_gemm(x, w, nbr, cout, w_transposed=False, flip_k=False, bias=None, row_perm=None, stats=False):
    """y[o] = sum_k x[nbr[o,k]] @ W[k] (+bias) on the fp32 matrix cores.  `stats=True` (forward
    only) also returns the column (sum, sum of squares) partials [rows,2,cout] (float64) of y for
    the batch norm that follows, or None when the launch shape cannot produce them."""
    L = lib()
    n_out, K = nbr.shape
    cin = x.shape[1]
    y = torch.empty(n_out, cout, dtype=torch.float32, device=x.device)
    if K > 27:  # the 5^3 / 7^3 cubes (csrc/conv_bigk.hip): one launch, fp32 in every math mode, no statistics partial
        if row_perm is not None:
            raise ValueError(f"gather_gemm: a row permutation with kernel volume {K} is not implemented (27 offsets at most)")
        note_table(nbr)
        check(
            L.mink_conv_bigk_gather_gemm(
                x.data_ptr(), x.shape[0], x.stride(0), cin, w.data_ptr(), int(w_transposed), int(flip_k), nbr.data_ptr(), n_out, K,
                y.data_ptr(), cout, cout, _ptr(bias), _stream(),
            )
        )
        return (y, None) if stats else y
    n_rows = n_out if row_perm is None else row_perm.numel()
    ksplit = _FORCE_KSPLIT or _plan_ksplit(L, n_rows, K, cin, cout, int(row_perm is not None))
    ws = _scratch(4 * ksplit * n_out * cout, x.device, "splitk") if ksplit > 1 else None
    partial = None
    note_table(nbr)
    if stats and not w_transposed and row_perm is None and n_out > 0:
        partial = torch.empty(512, 2, cout, dtype=torch.float64, device=x.device)
        sws = _scratch(L.mink_conv_stats_workspace_bytes(n_out, cout), x.device, "convstats")
        rows = ctypes.c_int32(0)
        check(
            L.mink_conv_gather_gemm_stats(
                x.data_ptr(), x.shape[0], x.stride(0), cin, w.data_ptr(), nbr.data_ptr(), n_out, K, y.data_ptr(), cout, cout,
                _ptr(bias), ksplit, _ptr(ws), 0 if ws is None else ws.numel(), partial.data_ptr(), ctypes.addressof(rows), sws.data_ptr(),
                sws.numel(), _stream(),
            )
        )
        partial = partial[: rows.value] if rows.value > 0 else None
    else:
        check(
            L.mink_conv_gather_gemm(
                x.data_ptr(), x.shape[0], x.stride(0), cin, w.data_ptr(), int(w_transposed), int(flip_k), nbr.data_ptr(), n_out, K,
                _ptr(row_perm), 0 if row_perm is None else row_perm.numel(),
                y.data_ptr(), cout, cout, _ptr(bias), ksplit, _ptr(ws), 0 if ws is None else ws.numel(), _stream(),
            )
        )
    return (y, partial) if stats else y


def dense_xwt(x, w):
    """x [n, Kd] @ w[N, Kd]^T on the fp32 matrix cores (mink_dense_xwt)."""
    x, w = _f32c(x), _f32c(w)
    y = torch.empty(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    check(lib().mink_dense_xwt(x.data_ptr(), w.data_ptr(), x.shape[0], x.shape[1], w.shape[0], y.data_ptr(), _stream()))
    return y


def conv_wgrad(x, dy, nbr, kernel_shape, out=None, on=None):
    """dW[k] = X[nbr[:, k]]^T dY.  `out`: write into this contiguous fp32 tensor (a slice of a
    data-parallel reducer's flat gradient buffer) instead of a fresh one.  `on`: launch on this torch
    stream instead of the current one (the caller orders it and records the buffers it reads; a fresh
    result tensor is recorded here) -- cheaper than switching the current stream around the call."""
    L = lib()
    n_out, K = nbr.shape
    cin, cout = x.shape[1], dy.shape[1]
    if out is not None:
        dw = out
    else:
        dw = torch.empty(kernel_shape, dtype=torch.float32, device=x.device)
        if on is not None:
            dw.record_stream(on)
    ws = _scratch(_wgrad_ws_bytes(L, n_out, K, cin, cout), x.device, "wgrad", on)
    raw = _stream() if on is None else on.cuda_stream
    note_table(nbr)
    check(
        (L.mink_conv_bigk_wgrad if K > 27 else L.mink_conv_wgrad)(
            x.data_ptr(), x.shape[0], x.stride(0), cin, dy.data_ptr(), dy.stride(0), cout, nbr.data_ptr(), n_out, K,
            dw.data_ptr(), ws.data_ptr(), ws.numel(), raw,
        )
    )
    return dw


_PLAN_CACHE = {}


def _cached_plan(key, query):
    """`int(query(*key[1:]))`, asked of the library once per key; the table is dropped whole when it overflows."""
    v = _PLAN_CACHE.get(key)
    if v is None:
        if len(_PLAN_CACHE) > 4096:
            _PLAN_CACHE.clear()
        v = _PLAN_CACHE[key] = int(query(*key[1:]))
    return v


def _wgrad_ws_bytes(L, n_out, K, cin, cout):
    return _cached_plan(("wws", n_out, K, cin, cout), L.mink_conv_bigk_wgrad_workspace_bytes if K > 27 else L.mink_conv_wgrad_workspace_bytes)


def _plan_ksplit(L, n_rows, K, cin, cout, classes):
    return _cached_plan(("ks", n_rows, K, cin, cout, classes), L.mink_conv_plan)


class ConvolutionFunction(torch.autograd.Function):
    """MinkowskiConvolution forward/backward (reference modules/common.py:116-125; A6).

    `table_fn(transposed)` returns (nbr, nbr_t) lazily so the transposed table is only built
    when an input gradient is really needed (the stem conv needs wgrad only).
    """

    @staticmethod
    def forward(ctx, x, kernel, table_fn, same_map, stats_holder=None):
        """`stats_holder`: a list that receives the column-statistics partials of the output (or
        None) -- the batch norm that follows then skips its own reduction pass."""
        x = _f32c(x)
        w = _f32c(kernel)
        cin = x.shape[1]
        ctx.cin = cin
        if cin % 4 and not ctx.needs_input_grad[0] and w.shape[0] <= 27:  # (the K > 27 kernels have no alignment needs)
            # e.g. the reference default features=["sh"] (27 channels): one zero column puts the
            # rows on 16-byte boundaries so the vectorised / flattened-K kernels apply
            pad = 4 - cin % 4
            x = torch.nn.functional.pad(x, (0, pad))
            w = torch.nn.functional.pad(w, (0, 0, 0, pad))
        tables = table_fn(False)
        nbr = tables[0]
        ctx.save_for_backward(x, w)
        ctx.table_fn, ctx.same_map, ctx.nbr = table_fn, same_map, nbr
        if stats_holder is None:  # a transposed convolution brings the parity-class row order of its output
            return gather_gemm(x, w, nbr, w.shape[-1], row_perm=tables[2] if len(tables) > 2 else None)
        y, partial = gather_gemm(x, w, nbr, w.shape[-1], stats=True)
        stats_holder.append(partial)
        return y

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        gy = _f32c(gy)
        gx = gw = None
        want_gx, want_gw = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        # dgrad and wgrad only share their inputs: run wgrad on a second HIP stream so the two
        # (latency-bound for the deep, small layers) overlap; the compute stream re-joins before
        # anything can consume the weight gradient.
        side = streams.side_stream(gy.device) if (want_gx and want_gw and streams.wgrad_overlap()) else None
        if side is not None:
            main = current_stream()
            stream_wait(side, main)  # gy / x are ready on the side stream
            skew(side)
        if want_gx:
            # dgrad = the same gather-GEMM over the transposed map with W[k]^T (read in place)
            if ctx.same_map:  # stride 1: nbr_t[i][k] == nbr[i][K-1-k]
                gx = gather_gemm(gy, w, ctx.nbr, w.shape[-2], w_transposed=True, flip_k=True)
            elif w.shape[0] == 1 and w.shape[-1] % 4 == 0 and w.shape[-2] % 4 == 0:
                # kernel volume 1, strided (the shortcut of a residual block): the product is a plain GEMM over the
                # OUTPUT rows, scattered to the input rows it reaches through the forward table -- the same two
                # kernels the native trunk sequences (no transposed table, no class permutation)
                gx = torch.zeros(x.shape[0], w.shape[-2], dtype=torch.float32, device=gy.device)
                gsc = dense_xwt(gy, w[0])
                check(lib().mink_rows_scatter_add(gsc.data_ptr(), ctx.nbr.data_ptr(), gsc.shape[0], gsc.shape[1], gx.data_ptr(), _stream()))
            else:
                _, nbr_t, perm = ctx.table_fn(True)
                gx = gather_gemm(gy, w, nbr_t, w.shape[-2], w_transposed=True, row_perm=perm)
        if want_gw:
            sink = streams.grad_sink()
            out = sink.view_for(w) if (sink is not None and w.shape[1] == ctx.cin) else None
            if side is not None:
                gw = conv_wgrad(x, gy, ctx.nbr, w.shape, out=out, on=side)  # (a fresh gw is recorded on the side stream there)
                for t in (x, gy, ctx.nbr):  # every buffer the side stream reads
                    t.record_stream(side)
                if out is not None:  # written in place into the reducer's buffer: nothing for autograd to do
                    streams.defer_join()
                    sink.ready(w)
                    if w.shape[-1] * w.shape[-2] <= streams._FLUSH_MAX_WEIGHTS:  # long kernels are queued: the host has time to launch collectives
                        sink.flush()
                    return gx, None, None, None, None
                # Nothing reads gw before backward ends when autograd merely installs it as
                # w.grad: then the join is deferred to the end-of-backward callback and the
                # wgrad kernels overlap the rest of the backward chain.  An existing .grad
                # (accumulation, DP flat buffers), a gradient hook or the channel-padding slice
                # below consume it right away: join now.
                # (No reference to gw may be kept here: AccumulateGrad only installs the tensor
                # itself when nobody else holds it -- otherwise it CLONES it, at once, on the
                # compute stream.  Double backward clones as well.)
                home = streams.home_stream(gw.device.index)
                if home is not None and home != main:
                    gw.record_stream(home)  # a branch's gradient is consumed by the network's own stream later
                if w.is_leaf and w.grad is None and not getattr(w, "_post_accumulate_grad_hooks", None) and \
                        not w._backward_hooks and gw.shape[1] == ctx.cin and not torch.is_grad_enabled():
                    streams.defer_join()
                else:
                    stream_wait(main, side)
            else:
                gw = conv_wgrad(x, gy, ctx.nbr, w.shape, out=out)
                if out is not None:
                    sink.ready(w)
                    return gx, None, None, None, None
            if gw.shape[1] != ctx.cin:  # drop the gradient of the zero-padded input channels
                gw = gw[:, : ctx.cin].contiguous()
        return gx, gw, None, None, None


class PointwiseConvolutionFunction(torch.autograd.Function):
    """1x1x1 stride-1 convolution = F @ W (`use_mm`, witness sparse_conv.py:323-335).  Forward and input
    gradient are plain library GEMMs with a long M; the weight gradient X^T dY is [cin, cout] small with the
    row count as its reduction dimension -- the library runs that on a few dozen workgroups (14 ms for
    825 k x 128 -> 96), so it goes through the streaming weight-gradient kernel with an identity table."""

    @staticmethod
    def forward(ctx, x, w, ident_fn):
        ctx.save_for_backward(x, w)
        ctx.ident_fn = ident_fn
        return x.mm(w)

    @staticmethod
    def backward(ctx, gy):
        x, w = ctx.saved_tensors
        # (W^T materialised: for the transposed-operand form the library picks a 12-wide macro tile -- 10 ms
        # instead of 0.7 ms for 825 k x 96 -> 128)
        gx = gy.mm(w.t().contiguous()) if ctx.needs_input_grad[0] else None
        gw = None
        if ctx.needs_input_grad[1]:
            gw = conv_wgrad(_f32c(x), _f32c(gy), ctx.ident_fn(), (1,) + tuple(w.shape)).view_as(w)
        return gx, gw, None


class ConvBNReLUSumPoolFunction(torch.autograd.Function):
    """pool(relu(bn(conv(x)))) of the network stem (reference resnet.py:58-64) as ONE autograd node,
    for an input that needs no gradient: forward = convolution (+ column statistics in its epilogue)
    and the fused bn+relu+sum-pool pass; backward = (dgamma, dbeta) reduction and the streaming
    weight-gradient kernel recomputing the gradient w.r.t. the conv output inside its operand load
    -- neither bn(conv(x)) nor its gradient (825 k x 64 floats each at B=16) is ever written."""

    @staticmethod
    def forward(ctx, x, kernel, gamma, beta, running_mean, running_var, momentum, eps, nbr, nbr_pool, in2out):
        L = lib()
        x, w = _f32c(x), _f32c(kernel)
        cin = x.shape[1]
        ctx.cin = cin
        if cin % 4:
            pad = 4 - cin % 4
            x = torch.nn.functional.pad(x, (0, pad))
            w = torch.nn.functional.pad(w, (0, 0, 0, pad))
        C = w.shape[-1]
        y, partial = gather_gemm(x, w, nbr, C, stats=True)
        n = y.shape[0]
        mean, invstd = _bn_statistics(L, y, n, C, eps, momentum, running_mean, running_var, partial)
        n_pool, K = nbr_pool.shape
        out = torch.empty(n_pool, C, dtype=torch.float32, device=x.device)
        check(
            L.mink_bn_relu_pool_fwd(
                y.data_ptr(), C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(), nbr_pool.data_ptr(),
                n_pool, K, out.data_ptr(), _stream(),
            )
        )
        ctx.save_for_backward(x, w, y, mean, invstd, gamma, beta)
        ctx.nbr, ctx.in2out = nbr, in2out
        ctx.kernel = kernel  # only as the key of its gradient slot under data parallelism
        return out

    @staticmethod
    def backward(ctx, gy):
        L = lib()
        x, w, y, mean, invstd, gamma, beta = ctx.saved_tensors
        gy = _f32c(gy)
        n, C = y.shape
        dev = y.device
        need = ctx.needs_input_grad
        pv = streams.sink_views(gamma, beta) if need[2] and need[3] else None  # data parallelism: write straight into the reducer's buffer
        kv = streams.sink_views(ctx.kernel) if need[1] and w.shape[1] == ctx.cin else None
        if pv is not None:
            dgamma, dbeta = pv
        else:
            dgamma = torch.empty(C, dtype=torch.float32, device=dev)
            dbeta = torch.empty(C, dtype=torch.float32, device=dev)
        gw = kv[0] if kv is not None else None
        ws = _scratch(L.mink_bn_workspace_bytes(n, C), dev, "bn")
        check(
            L.mink_bn_relu_pool_bwd(
                gy.data_ptr(), y.data_ptr(), n, C, mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                ctx.in2out.data_ptr(), None, dgamma.data_ptr(), dbeta.data_ptr(), ws.data_ptr(), ws.numel(), _stream(),
            )
        )
        nbr = ctx.nbr
        K = nbr.shape[1]
        if gw is None:
            gw = torch.empty(w.shape, dtype=torch.float32, device=dev)
        wws = _scratch(L.mink_conv_wgrad_workspace_bytes(n, K, x.shape[1], C), dev, "wgrad")
        note_table(nbr)
        check(
            L.mink_conv_wgrad_bn_relu_pool(
                x.data_ptr(), x.shape[0], x.stride(0), x.shape[1], y.data_ptr(), C, gy.data_ptr(), gy.shape[0],
                ctx.in2out.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gamma.data_ptr(), beta.data_ptr(),
                dgamma.data_ptr(), dbeta.data_ptr(), nbr.data_ptr(), n, K, gw.data_ptr(), wws.data_ptr(), wws.numel(), _stream(),
            )
        )
        sink = streams.grad_sink()
        if sink is not None and hasattr(sink, "flush"):
            sink.flush()  # the stem's weight gradient (0.9 ms) is queued: everything completed so far goes out beside it
        if pv is not None:
            sink.ready(gamma), sink.ready(beta)
            dgamma = dbeta = None
        if kv is not None:
            sink.ready(ctx.kernel)
            gw = None
        elif gw.shape[1] != ctx.cin:
            gw = gw[:, : ctx.cin].contiguous()
        return None, gw, dgamma, dbeta, None, None, None, None, None, None, None

    @staticmethod
    def supported(x, kernel, nbr):
        cin = x.shape[1] + (-x.shape[1]) % 4
        return bool(lib().mink_conv_wgrad_bn_relu_pool_supported(x.shape[0], cin, cin, nbr.shape[0], nbr.shape[1], kernel.shape[-1]))


# ------------------------------------------------------------------------- re-exports
# Every public name that moved to a module of its own, so that `functional.<name>` stays valid.  Functions only: the
# mutable state of streams.py is read there (`streams.X`), never copied here.
from ._rt import _bytes, _check_offsets, _row_stride  # noqa: E402,F401
from .attn import AttentionB16Function, AttentionFunction, attention, attention_b16  # noqa: E402,F401
from .eltwise import ACT_KINDS, ActivationFunction, AddFunction, ReLUFunction, _eltwise  # noqa: E402,F401
from .field import FieldGatherCatFunction, SegmentMeanFunction, field_batch_offsets, index_csr, lazy_index_csr, segment_mean  # noqa: E402,F401
from .gconv import GroupedConvolutionFunction, gconv, gconv_wgrad  # noqa: E402,F401
from .head import (  # noqa: E402,F401
    SEG_STATS_WORDS,
    GlobalAvgLinearFunction,
    SegCrossEntropyFunction,
    SliceFunction,
    SoftmaxCrossEntropyFunction,
    cross_entropy,
    global_avg_linear,
    seg_cross_entropy,
    seg_stats,
    slice_rows,
)
from .interp import InterpolationFunction, SplatFunction  # noqa: E402,F401
from .norm import BatchNormFunction, BNReLUSumPoolFunction, InstanceNormFunction, LayerNormFunction, PowerNormFunction, SyncBatchNormFunction  # noqa: E402,F401
from .pool import (  # noqa: E402,F401
    AvgPoolFunction,
    GlobalAvgPoolFunction,
    GlobalMaxPoolFunction,
    GlobalSumPoolFunction,
    MaxPoolFunction,
    OverlapSumPoolFunction,
    SparseMaxPoolFunction,
    SumPoolFunction,
)
from .posenc import PositionalEncodingFunction, positional_encoding  # noqa: E402,F401
from .streams import (  # noqa: E402,F401
    branch_fork_enabled,
    branch_stream,
    compute_streams,
    join_side_streams,
    new_stream,
    note_prepare_gate,
    set_branch_fork,
    set_grad_sink,
    set_trunk_branch_on_side,
    set_wgrad_overlap,
    side_stream_if_any,
    trunk_branch_mode,
    wait_prepare_gate,
)
# (under their earlier names: the gate's parser, and its event table -- a dict that is filled and cleared, never rebound, so
# this is the one object of streams.py and not a copy of it)
from .streams import _PREPARE_GATE_EVENT  # noqa: E402,F401
from .streams import parse_gate as _parse_gate  # noqa: E402,F401

pair_csr, lazy_csr = index_csr, lazy_index_csr  # the names these had when interpolation and the point stage each kept a copy
