"""Call helpers of the operator wrappers: the raw handle of the current HIP stream, fp32-contiguous inputs, optional
pointers, recycled scratch buffers and the checks several operator families share.  Imports torch only."""
import torch


def _stream():
    return torch._C._cuda_getCurrentRawStream(torch.cuda.current_device())


def _f32c(t):
    assert t.is_cuda, "the HIP backend has no CPU path"
    return t.contiguous() if t.dtype == torch.float32 else t.float().contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _bytes(nbytes, device):
    return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)


def _row_stride(x):
    """Leading dimension of the rows of x [n, C]: torch reports an arbitrary stride(0) for a single row."""
    return x.stride(0) if x.shape[0] > 1 else x.shape[1]


# Scratch buffers of the main (compute) stream are recycled: kernels on one stream run in
# order, so the next user may overwrite a workspace as soon as it is enqueued behind the last.
_SCRATCH = {}


def _scratch(nbytes, device, slot, on=None):
    """`on`: the torch stream the buffer will be used on when that is not the current one."""
    stream = _stream() if on is None else on.cuda_stream
    key = (device.index, stream, slot)
    buf = _SCRATCH.get(key)
    nbytes = max(int(nbytes), 256)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes * 1.25), dtype=torch.uint8, device=device)
        if on is not None:  # allocated under the current stream, used on `on`: a later free must wait for that stream
            buf.record_stream(on)
        _SCRATCH[key] = buf
    return buf


def _check_offsets(boff):
    assert boff.is_cuda and boff.dtype == torch.int32 and boff.is_contiguous() and boff.numel() >= 2, \
        "batch offsets: a contiguous int32 [B+1] device tensor"
    return boff.numel() - 1
