"""Multi-head self-attention on packed token rows (csrc/attn.hip, fp32; csrc/attn16.hip, bf16 rows)."""
import torch

from .._lib import check, lib
from ._rt import _f32c, _row_stride, _scratch, _stream


def _attn_shape(qkv, batch, tokens, heads):
    n, width = qkv.shape
    assert n == batch * tokens and width % (3 * heads) == 0, \
        f"attention: qkv is [{n}, {width}], not [batch * tokens = {batch * tokens}, 3 * heads * D] with heads = {heads}"
    return width // (3 * heads)


class AttentionFunction(torch.autograd.Function):
    """apply(qkv, batch, tokens, heads, scale) -> [batch * tokens, heads * D]: the multi-head self-attention of a ViT block
    on token rows (timm's Attention.forward between `qkv` and `proj`).  qkv [batch * tokens, 3 * heads * D] is what
    nn.Linear(dim, 3 * dim) writes, the result is what `proj` reads: no permute copy on either side.  D == 64, fp32 on the
    fp32 matrix cores whatever set_conv_math says.  Saves qkv, out and lse [batch, heads, tokens]; the backward is one
    call that recomputes the probabilities, without atomics (two runs give the same bits)."""

    @staticmethod
    def forward(ctx, qkv, batch, tokens, heads, scale):
        L = lib()
        qkv = _f32c(qkv)
        D = _attn_shape(qkv, batch, tokens, heads)
        out = torch.empty(batch * tokens, heads * D, dtype=torch.float32, device=qkv.device)
        lse = torch.empty(batch, heads, tokens, dtype=torch.float32, device=qkv.device)
        check(L.mink_attn_fwd(qkv.data_ptr(), qkv.shape[1], batch, tokens, heads, D, float(scale), out.data_ptr(), heads * D,
                              lse.data_ptr(), _stream()))
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (batch, tokens, heads, D, float(scale))
        return out

    @staticmethod
    def backward(ctx, gout):
        L = lib()
        qkv, out, lse = ctx.saved_tensors
        batch, tokens, heads, D, scale = ctx.cfg
        gout = _f32c(gout)
        gqkv = torch.empty_like(qkv)
        ws = _scratch(L.mink_attn_bwd_workspace_bytes(batch, tokens, heads, D), qkv.device, "attn")
        check(L.mink_attn_bwd(qkv.data_ptr(), qkv.shape[1], out.data_ptr(), heads * D, lse.data_ptr(), gout.data_ptr(), heads * D,
                              batch, tokens, heads, D, scale, gqkv.data_ptr(), qkv.shape[1], ws.data_ptr(), ws.numel(), _stream()))
        return gqkv, None, None, None, None


def attention(qkv, batch, tokens, heads, scale=None):
    """softmax(scale q k^T) v per (sample, head) on packed rows; scale defaults to D ** -0.5."""
    if scale is None:
        scale = _attn_shape(qkv, batch, tokens, heads) ** -0.5
    return AttentionFunction.apply(qkv, batch, tokens, heads, scale)


def _b16_rows(t, what):
    """bf16 rows on the GPU, contiguous or with a row pitch (unit column stride) -> (t, pitch in elements)"""
    if t.dtype != torch.bfloat16:
        raise TypeError(f"attention_b16: {what} is {t.dtype}, not torch.bfloat16; fp32 rows go through attention()")
    assert t.is_cuda, "the HIP backend has no CPU path"
    if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1) or (t.shape[0] > 1 and t.stride(0) < t.shape[1]):
        t = t.contiguous()
    return t, max(_row_stride(t), t.shape[1])


class AttentionB16Function(torch.autograd.Function):
    """apply(qkv, batch, tokens, heads, scale) -> bf16 [batch * tokens, heads * D]: AttentionFunction on bf16 rows with the
    products on the bf16 matrix cores (csrc/attn16.hip; include/mink_hip.h states where it rounds to bf16).  qkv is bf16
    [batch * tokens, 3 * heads * D], contiguous or with a row pitch.  Saves qkv, out (bf16) and lse (fp32); the gradient of
    qkv is bf16.  No atomics: two runs give the same bits."""

    @staticmethod
    def forward(ctx, qkv, batch, tokens, heads, scale):
        L = lib()
        qkv, ldq = _b16_rows(qkv, "qkv")
        D = _attn_shape(qkv, batch, tokens, heads)
        out = torch.empty(batch * tokens, heads * D, dtype=torch.bfloat16, device=qkv.device)
        lse = torch.empty(batch, heads, tokens, dtype=torch.float32, device=qkv.device)
        check(L.mink_attn_fwd_b16(qkv.data_ptr(), ldq, batch, tokens, heads, D, float(scale), out.data_ptr(), heads * D,
                                  lse.data_ptr(), _stream()))
        ctx.save_for_backward(qkv, out, lse)
        ctx.cfg = (batch, tokens, heads, D, float(scale), ldq)
        return out

    @staticmethod
    def backward(ctx, gout):
        L = lib()
        qkv, out, lse = ctx.saved_tensors
        batch, tokens, heads, D, scale, ldq = ctx.cfg
        gout, lddo = _b16_rows(gout if gout.dtype == torch.bfloat16 else gout.bfloat16(), "the gradient of out")
        gqkv = torch.empty(batch * tokens, 3 * heads * D, dtype=torch.bfloat16, device=qkv.device)
        ws = _scratch(L.mink_attn_bwd_b16_workspace_bytes(batch, tokens, heads, D), qkv.device, "attn16")
        check(L.mink_attn_bwd_b16(qkv.data_ptr(), ldq, out.data_ptr(), heads * D, lse.data_ptr(), gout.data_ptr(), lddo,
                                  batch, tokens, heads, D, scale, gqkv.data_ptr(), 3 * heads * D, ws.data_ptr(), ws.numel(), _stream()))
        return gqkv, None, None, None, None


def attention_b16(qkv, batch, tokens, heads, scale=None):
    """attention() on bf16 rows: bf16 in, bf16 out, products on the bf16 matrix cores; scale defaults to D ** -0.5."""
    if qkv.dtype != torch.bfloat16:
        raise TypeError(f"attention_b16: qkv is {qkv.dtype}, not torch.bfloat16; fp32 rows go through attention()")
    if scale is None:
        scale = _attn_shape(qkv, batch, tokens, heads) ** -0.5
    return AttentionB16Function.apply(qkv, batch, tokens, heads, scale)
