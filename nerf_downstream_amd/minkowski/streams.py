"""Process-wide stream orchestration of a training step: the weight-gradient side stream, the shortcut-branch stream, the
home streams they fork from, cached stream objects and wait events, the prepare gate, the skew hook, the end-of-backward
join with its callbacks, and the data-parallel gradient sink.

Every mutable global below has this module as its one home: read it as `streams.X` (or through its accessor) at the time
of use, never by `from .streams import X`, which would freeze the value seen at import.  Imports torch, the standard
library and the native library only, so every operator module may import it.
"""
import ctypes
import os
import re

import torch

from .._lib import check, lib

# ------------------------------------------------------------------- stream creation and lookup
_SIDE_STREAMS = {}
_BRANCH_STREAMS = {}
_HOME_STREAMS = {}  # device index -> the stream the network itself runs on (noted where a branch forks off)
_CU_STREAMS = []  # (raw handle) of the CU-subset streams created here: they live as long as the process
_CU_DEFAULTS = {}


def new_stream(device, role):
    """A HIP stream for one of the auxiliary roles ("prepare": the next batch's coordinate maps, "wgrad": the weight
    gradients, "branch": the shortcut branch).  MINK_CUS_<ROLE>="first:count" (or "count") confines it to that range
    of compute units (mink_stream_create_cu_subset): what runs on it then cannot take execution slots from the
    kernels of the compute stream on the other CUs."""
    spec = os.environ.get("MINK_CUS_" + role.upper(), _CU_DEFAULTS.get(role, ""))
    if not spec or spec == "0":
        return torch.cuda.Stream(device=device)
    first, _, count = spec.rpartition(":")
    total = torch.cuda.get_device_properties(device).multi_processor_count
    first, count = int(first or 0), int(count)
    h = ctypes.c_void_p()
    with torch.cuda.device(device):
        check(lib().mink_stream_create_cu_subset(first, count, total, ctypes.byref(h)))
    _CU_STREAMS.append(h.value)
    return torch.cuda.ExternalStream(h.value, device=device)


def side_stream(device):
    """The weight-gradient stream of `device`, created on first use."""
    s = _SIDE_STREAMS.get(device.index)
    if s is None:
        s = _SIDE_STREAMS[device.index] = new_stream(device, "wgrad")
    return s


def side_stream_if_any(device):
    return _SIDE_STREAMS.get(device.index)


def compute_streams(device):
    """The auxiliary compute streams this module has created on `device` (weight-gradient stream,
    shortcut-branch stream): whoever consumes gradients from another stream joins these."""
    return [d[device.index] for d in (_SIDE_STREAMS, _BRANCH_STREAMS) if device.index in d]


def branch_stream(device, home=None):
    """A second compute stream for an independent branch of the network (the shortcut
    convolution of a residual block runs beside the main branch: both are small kernels that do
    not fill the chip on their own).  `home`: the stream the caller forks from."""
    s = _BRANCH_STREAMS.get(device.index)
    if s is None:
        s = _BRANCH_STREAMS[device.index] = new_stream(device, "branch")
        quiet = getattr(torch.autograd.graph, "set_warn_on_accumulate_grad_stream_mismatch", None)
        if quiet is not None:  # parameters of the branch get their gradient from this stream on purpose
            quiet(False)
    if home is not None:
        _HOME_STREAMS[device.index] = home
    return s


def home_stream(index):
    """The stream a branch on device `index` last forked from, or None."""
    return _HOME_STREAMS.get(index)


_STREAM_OBJS = {}


def current_stream(device=None):
    """torch.cuda.current_stream(device) without building a Stream object per call (8 us each, ~15 per step on the hot path: 0.12 ms
    of a host-bound step): the raw handle of the current stream is one C call, the object comes out of a cache.
    `device`: None, an index, a torch.device or a string such as "cuda:0".

    The cache `_STREAM_OBJS` is keyed by (device index, raw handle), so it may only ever hold streams whose handle lives
    as long as the process: torch's pool and default streams (new_stream's CU-subset streams are never destroyed either).
    A handle that HIP destroyed and handed out again would find the object of the dead stream here."""
    idx = device.index if (device is not None and getattr(device, "index", None) is not None) else (
        device if isinstance(device, int) else torch.cuda.current_device())
    try:
        raw = torch._C._cuda_getCurrentRawStream(idx)
    except (TypeError, RuntimeError):  # "cuda:0": the `index` of a str is the bound method str.index, which torch's C call rejects
        if not isinstance(device, str):
            raise
        return current_stream(torch.device(device))
    s = _STREAM_OBJS.get((idx, raw))
    if s is None:
        s = _STREAM_OBJS[(idx, raw)] = torch.cuda.current_stream(idx)
    return s


_WAIT_EVENTS = {}


def stream_wait(waiter, awaited):
    """`waiter.wait_stream(awaited)` without creating a HIP event per call (9 us each on this stack, ~20 per
    step): one cached event per awaited stream.  Re-recording it later does not disturb a wait already
    queued -- a stream wait captures the record that precedes it."""
    ev = _WAIT_EVENTS.get(awaited)
    if ev is None:
        ev = _WAIT_EVENTS[awaited] = torch.cuda.Event()
    ev.record(awaited)
    waiter.wait_event(ev)


# ------------------------------------------------------------------- branch settings
_BRANCH_FORK = True
_TRUNK_BRANCH_ON_SIDE = False  # data parallelism: the native trunk runs its shortcut branch on the weight-gradient stream


def set_branch_fork(on=True):
    """Allow / forbid residual blocks to run their shortcut branch on the second compute stream."""
    global _BRANCH_FORK
    old, _BRANCH_FORK = _BRANCH_FORK, bool(on)
    return old


def branch_fork_enabled():
    return _BRANCH_FORK


def set_trunk_branch_on_side(on=True):
    """The native trunk's shortcut branch on the weight-gradient stream instead of a stream of its own (data parallelism:
    the process group's streams already take hardware queues; the module-by-module path then does not fork at all)."""
    global _TRUNK_BRANCH_ON_SIDE
    old, _TRUNK_BRANCH_ON_SIDE = _TRUNK_BRANCH_ON_SIDE, bool(on)
    return old


def trunk_branch_mode():
    """Where the native trunk runs the shortcut branch of its residual blocks: "own" (a stream of its own), "side" (the
    weight-gradient stream: data parallelism with fp32 matrix math, where that stream has room -- under bf16 math its
    fp32 weight gradients are the long pole and the branch behind them stalls the chain: 2.64 -> 2.69 ms) or None."""
    if _BRANCH_FORK:
        return "own"
    if _TRUNK_BRANCH_ON_SIDE and lib().mink_conv_get_math() != 1:  # (1: bf16, see functional.set_conv_math)
        return "side"
    return None


# ------------------------------------------------------------------- test and gating hooks
_SKEW = int(os.environ.get("MINK_STREAM_SKEW", "0"))  # race hunting: delay every auxiliary stream by this many GPU cycles


def skew(stream):
    """Test hook: stall `stream` for MINK_STREAM_SKEW cycles before its next piece of work, so a
    missing cross-stream dependency shows up as a wrong result instead of passing by luck."""
    if _SKEW:
        with torch.cuda.stream(stream):
            torch.cuda._sleep(_SKEW)


def parse_gate(v):
    """"f<i>" / "b<i>": before block i of the native trunk's forward / backward pass; "b-1": before the stem's backward; "0": off."""
    if not v or v == "0":
        return None
    if not re.fullmatch(r"[fb]-?\d+", v):
        raise ValueError(f"MINK_PREPARE_GATE={v!r}: expected 'f<i>' or 'b<i>' (block index; 'b-1' = before the stem's backward) or '0'")
    return (1 if v[0] == "b" else 0, int(v[1:]))


# MINK_PREPARE_GATE (off by default): the prepare stream may start a batch's pyramid / plan only once the compute stream has
# reached this point of its latest native-trunk pass -- one map build per step, beside the middle of the step, instead of a
# prepare stream that follows the host however far ahead it is.  Steady step times and fewer prepared batches in memory (peak
# reserved 38.8 -> 26.7 GB), no throughput gain (3,000 steps: 3.43-3.44 ms against 3.41-3.43); a short timed window
# loses its map-free tail and host-bound shapes lose ~1 % (profiles/r05_transient.txt).
_PREPARE_GATE = parse_gate(os.environ.get("MINK_PREPARE_GATE", "0"))  # (backward?, stage): see trunk._stage_hook
_PREPARE_GATE_EVENT = {}  # device index -> event of the latest gate point


def note_prepare_gate(stream):
    _PREPARE_GATE_EVENT[stream.device.index] = stream.record_event()


def wait_prepare_gate(stream):
    ev = _PREPARE_GATE_EVENT.get(stream.device.index) if (_PREPARE_GATE_EVENT and stream is not None) else None
    if ev is not None:
        stream.wait_event(ev)


# ------------------------------------------------------------------- join handling
_DEFERRED = {"pending": False, "task": -1}  # task: the autograd graph task the end-of-backward join is queued for
_AFTER_JOIN = []  # callables run once the compute stream is ordered after the side stream (release of kept-alive buffers)


def after_join(fn):
    """Run `fn()` every time the compute stream has been ordered after the side stream."""
    _AFTER_JOIN.append(fn)


def join_side_streams():
    """Make the current stream wait for weight gradients still in flight on the side stream (no-op when none are)."""
    if _DEFERRED["pending"]:
        _DEFERRED["pending"] = False
        for index, side in _SIDE_STREAMS.items():
            stream_wait(current_stream(index), side)
    for fn in _AFTER_JOIN:
        fn()


def _join_side_streams():
    """End-of-backward callback: the compute stream waits for the weight gradients still running
    on the side stream, so everything after backward() (optimizer, clipping, ...) is ordered."""
    _DEFERRED["task"] = -1
    join_side_streams()


def defer_join():
    """Queue the end-of-backward join once per backward pass.  Keyed by the autograd graph task: a backward that
    raised drops its queued callbacks, and a flag that merely said "already queued" would then stay set for the
    rest of the process -- every later optimizer step would read weight gradients the side stream is still writing."""
    _DEFERRED["pending"] = True
    task = torch._C._current_graph_task_id()
    if _DEFERRED["task"] != task or task < 0:
        _DEFERRED["task"] = task
        torch.autograd.Variable._execution_engine.queue_callback(_join_side_streams)


# ------------------------------------------------------------------- data-parallel hooks
_OVERLAP_WGRAD = True  # weight gradients on a side stream, joined at the end of backward (B=16 ResNet14: 5.11 -> 4.84 ms/step)


def set_wgrad_overlap(on=True):
    global _OVERLAP_WGRAD
    old, _OVERLAP_WGRAD = _OVERLAP_WGRAD, bool(on)
    return old


def wgrad_overlap():
    return _OVERLAP_WGRAD


_GRAD_SINK = None  # a data-parallel reducer that owns the gradient memory (see set_grad_sink)
# Where a deferred bucket collective may be launched: behind the backward of a convolution with at most this many
# weights per offset -- the wide-and-shallow layers, whose kernels keep the GPU busy for >100 us.  A static property
# of the layer on purpose: every rank then issues its collectives at the same points of the backward pass (a
# row-count rule would depend on each rank's batch and could interleave them differently with SyncBatchNorm's).
_FLUSH_MAX_WEIGHTS = 128 * 128


def set_grad_sink(sink):
    """`sink.view_for(param)` -> the tensor the weight gradient of `param` is to be WRITTEN into (or
    None: hand the gradient to autograd as usual); `sink.ready(param)` is called once that write
    has been queued, `sink.release(param)` if it will not be after all, `sink.flush()` where the host has
    time to spare (a large layer's kernels have just been queued).  This lets a bucketed all-reduce keep the weight-gradient side stream: without
    it every gradient would have to be accumulated into the reducer's buffer on the compute stream,
    i.e. joined layer by layer."""
    global _GRAD_SINK
    old, _GRAD_SINK = _GRAD_SINK, sink
    return old


def grad_sink():
    return _GRAD_SINK


def sink_views(*params):
    """Data parallelism: the slices of the reducer's flat buffer to write these parameters' gradients into --
    all of them or none (then autograd accumulates as usual).  Saves one accumulate launch per parameter."""
    sink = _GRAD_SINK
    if sink is None:
        return None
    bulk = getattr(sink, "views_for", None)
    if bulk is not None:
        return bulk(params)
    views = []
    for p in params:
        v = sink.view_for(p)
        if v is None:
            for q in params[: len(views)]:  # hand back what was claimed
                sink.release(q)
            return None
        views.append(v)
    return views
