"""Vision Transformer of the 2-D comparison (the networks the reference builds with timm.create_model("vit_*_patch16_224",
num_classes=51) in co3d_2d/src/model/models.py:37-54), written from scratch on token rows [B * N, dim]: timm is not a
dependency.

    patch embedding   the 16 x 16 patches of an image as rows [B * P, 3 * 256], one GEMM with the Conv2d-shaped weight
    tokens            class token in front, position embedding added, N = P + 1
    depth x block     x = x + proj(attention(qkv(LN(x))));  x = x + fc2(GELU(fc1(LN(x))))      (pre-norm, LayerNorm eps 1e-6)
    tail              LN, `head` on the class token

The attention between `qkv` and `proj` is minkowski.attn.AttentionFunction (csrc/attn.hip): it reads the packed rows
the qkv linear writes and writes the rows the proj linear reads, fp32 on the fp32 matrix cores, head size 64.  The exact-erf
GELU is ActivationFunction (mink_activation), the linears are dense GEMMs through torch as in MinkowskiLinear.  Layer norm is
LayerNormFunction (mink_ln_*) where the width fits that kernel's 512-channel limit -- vit_small, 384 -- and
torch.nn.functional.layer_norm above it (vit_base 768, vit_large 1024): the limit is part of the norm kernels' contract
(tests/test_gpu_norm.py) and is not widened here.  Every dropout and the drop path are 0, as timm's defaults are, so train
and eval mode compute the same function.

State-dict keys and shapes are timm's (`cls_token` [1, 1, dim], `pos_embed` [1, N, dim], `patch_embed.proj.weight`
[dim, 3, 16, 16], `blocks.{i}.norm1 / attn.qkv / attn.proj / norm2 / mlp.fc1 / mlp.fc2`, `norm`, `head`), so a timm or a
reference checkpoint loads unchanged.  The initialisation is timm's as recalled, NOT checked against timm (it is not
available here): truncated normal of std 0.02 for the linear weights, the class token and the position embedding, zero
biases, LayerNorm 1 / 0, torch's default for the patch convolution.

`math="bf16"` (VisionTransformer, `ViTBased.math`; the counterpart of the reference's precision=16) runs the four linears of
every block -- qkv, proj, fc1, fc2 -- as F.linear on explicit bf16 casts of the input, the fp32 master weight and the bias, and
the attention between qkv and proj as AttentionB16Function (csrc/attn16.hip) on the bf16 rows qkv wrote.  Their backward runs
in bf16 and the parameter gradients arrive fp32 through the casts.  The residual stream, the LayerNorms, the GELU (the same
ActivationFunction, on an fp32 copy), the patch embedding, class token, position embedding, final norm and `head` stay fp32;
the casts at those borders are torch's.  Nothing is autocast.  Parameters, state-dict keys and dtypes are those of
math="fp32": a checkpoint moves freely between the two modes."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from nerf_downstream_amd.minkowski.attn import AttentionB16Function, AttentionFunction
from nerf_downstream_amd.minkowski.eltwise import ActivationFunction
from nerf_downstream_amd.minkowski.norm import LayerNormFunction

PATCH = 16
HEAD_DIM = 64  # of all three networks, and the one size csrc/attn.hip is built for
LN_KERNEL_MAX = 512  # widest row of mink_ln_*
MATHS = ("fp32", "bf16")

# name -> (dim, depth, heads); mlp ratio 4
SIZES = {"vit_small_patch16_224": (384, 12, 6), "vit_base_patch16_224": (768, 12, 12), "vit_large_patch16_224": (1024, 24, 16)}


def layer_norm(x, ln):
    if x.shape[1] <= LN_KERNEL_MAX:
        return LayerNormFunction.apply(x, ln.weight, ln.bias, ln.eps, None, False)
    return F.layer_norm(x, ln.normalized_shape, ln.weight, ln.bias, ln.eps)


def linear_b16(x, lin):
    """lin(x) on the bf16 matrix cores: explicit casts of the input, the fp32 master weight and the bias; bf16 out"""
    return F.linear(x.bfloat16(), lin.weight.bfloat16(), lin.bias.bfloat16())


class PatchEmbed(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.proj = nn.Conv2d(3, dim, PATCH, PATCH)  # holds the parameters; the product below is a GEMM on patch rows

    def forward(self, images):
        B, C, Hh, Ww = images.shape
        gh, gw = Hh // PATCH, Ww // PATCH
        rows = images.reshape(B, C, gh, PATCH, gw, PATCH).permute(0, 2, 4, 1, 3, 5).reshape(B * gh * gw, C * PATCH * PATCH)
        return F.linear(rows, self.proj.weight.reshape(self.proj.out_channels, -1), self.proj.bias)


class Attention(nn.Module):
    def __init__(self, dim, heads, math="fp32"):
        super().__init__()
        self.math = math
        assert dim == heads * HEAD_DIM, f"head size {dim // heads}: the attention kernel is built for {HEAD_DIM}"
        self.num_heads, self.scale = heads, HEAD_DIM ** -0.5
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)

    def forward(self, x, batch, tokens):
        if self.math == "bf16":
            out = AttentionB16Function.apply(linear_b16(x, self.qkv), batch, tokens, self.num_heads, self.scale)
            return linear_b16(out, self.proj).float()
        return self.proj(AttentionFunction.apply(self.qkv(x), batch, tokens, self.num_heads, self.scale))


class Mlp(nn.Module):
    def __init__(self, dim, hidden, math="fp32"):
        super().__init__()
        self.math = math
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)

    def forward(self, x):
        if self.math == "bf16":  # (the GELU kernel is fp32: it runs on an fp32 copy of what fc1 wrote)
            return linear_b16(ActivationFunction.apply(linear_b16(x, self.fc1).float(), "gelu", 0.0, None), self.fc2).float()
        return self.fc2(ActivationFunction.apply(self.fc1(x), "gelu", 0.0, None))


class Block(nn.Module):
    def __init__(self, dim, heads, mlp_ratio=4, math="fp32"):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = Attention(dim, heads, math)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = Mlp(dim, int(dim * mlp_ratio), math)

    def forward(self, x, batch, tokens):
        x = x + self.attn(layer_norm(x, self.norm1), batch, tokens)
        return x + self.mlp(layer_norm(x, self.norm2))


class VisionTransformer(nn.Module):
    def __init__(self, img_size=224, dim=384, depth=12, heads=6, num_classes=51, mlp_ratio=4, math="fp32"):
        super().__init__()
        if math not in MATHS:
            raise ValueError(f"math={math!r}: one of {MATHS}")
        self.math = math
        if img_size < PATCH or img_size % PATCH:
            raise ValueError(f"img_size={img_size} is not a positive multiple of the patch size {PATCH}")
        self.img_size, self.embed_dim = img_size, dim
        self.num_tokens = (img_size // PATCH) ** 2 + 1
        self.patch_embed = PatchEmbed(dim)
        self.cls_token = nn.Parameter(torch.zeros(1, 1, dim))
        self.pos_embed = nn.Parameter(torch.zeros(1, self.num_tokens, dim))
        self.blocks = nn.ModuleList([Block(dim, heads, mlp_ratio, math) for _ in range(depth)])
        self.norm = nn.LayerNorm(dim, eps=1e-6)
        self.head = nn.Linear(dim, num_classes)
        nn.init.trunc_normal_(self.cls_token, std=0.02)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        for m in self.modules():
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def forward(self, images):
        B = images.shape[0]
        if images.shape[1:] != (3, self.img_size, self.img_size):
            raise ValueError(f"images of shape {tuple(images.shape)}: this network was built for [B, 3, {self.img_size}, {self.img_size}]")
        N, dim = self.num_tokens, self.embed_dim
        x = self.patch_embed(images.float()).reshape(B, N - 1, dim)
        x = (torch.cat([self.cls_token.expand(B, 1, dim), x], dim=1) + self.pos_embed).reshape(B * N, dim)
        for blk in self.blocks:
            x = blk(x, B, N)
        cls = x.reshape(B, N, dim)[:, 0]
        return self.head(layer_norm(cls.contiguous(), self.norm))
