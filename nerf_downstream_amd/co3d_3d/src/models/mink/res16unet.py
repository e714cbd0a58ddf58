"""Res16UNet segmentation family (counterpart of the reference's co3d_3d/src/models/mink/res16unet.py:25-575;
SURVEY 8f-3).  U-shaped sparse network: a two-convolution stem at tensor stride 1, four down-sampling
stages (convolution k=2 s=2 + residual blocks), four up-sampling stages (transposed convolution k=2 s=2
onto the encoder's coordinate map, concatenation with the encoder activation of that stride, residual
blocks), a 1x1x1 classifier, and the per-point read-back `out.slice(x).F`.

Module names follow the reference so state dicts map one to one: conv0p1s1, conv1p1s2, block1, conv2p2s2,
block2, conv3p4s2, block3, conv4p8s2, block4, convtr4p16s2, block5, convtr5p8s2, block6, convtr6p4s2,
block7, convtr7p2s2, block8, final -- each conv*/convtr* an nn.Sequential whose entries 0 / 1 (/ 3 / 4 in
the stem) are the convolution and its norm.

Reference quirk kept visible: the size-named subclasses read `self.PLANES`, which only the *A / *B / *C / *D
variants define (res16unet.py:438-453 vs :528-575); here the base class carries the constructor default
(32, 48, 64, 96, 96, 96, 64, 64) as a class attribute so Res16UNet14/18/34 are constructible; and the
classifier takes PLANES[7] * BLOCK.expansion inputs (the reference passes PLANES[7], res16unet.py:343-351,
which only fits the BasicBlock variants).

The `*Ins` variants (reference res16unet.py:584-601) add `offset_block` on block8's output and return (offsets, logits);
EncodedRes16UNet / EncodedRes16UNet2 (:604-795) wrap the U between two per-point MLPs behind a positional encoding."""
import torch
import torch.nn as nn

from nerf_downstream_amd import gin_lite as gin

from .base_model import MinkowskiBaseModel
from .modules.common import conv, conv_tr, get_nonlinearity, get_norm, takes_conv_stats
from .modules.resnet_block import BasicBlock, Bottleneck


class _Unit(nn.Sequential):
    """[conv, norm, nonlinearity] * n as the reference lays them out in an nn.Sequential; with a backend
    that fuses norm + ReLU (and takes the norm's statistics from the convolution's epilogue) each triple is
    two launches instead of four."""

    fused = False

    def forward(self, x):
        if not self.fused:
            return super().forward(x)
        mods = list(self)
        for j in range(0, len(mods), 3):
            x = mods[j + 1](mods[j](x, bn_stats=self.training and takes_conv_stats(mods[j + 1])), relu=True)
        return x


@gin.configurable
class Res16UNet(MinkowskiBaseModel):
    INSSEG = False
    BLOCK = BasicBlock
    PLANES = (32, 48, 64, 96, 96, 96, 64, 64)
    LAYERS = (2, 2, 2, 2, 2, 2, 2, 2)
    NORM_TYPE = "BN"

    def __init__(self, in_channel, out_channel, PLANES=None, LAYERS=None, BLOCK=None, NORM_TYPE=None,
                 nonlinearity="MinkowskiReLU", bn_momentum=0.1, D=3, ME=None, sparse_mode=(0,) * 9):
        """`sparse_mode` (reference res16unet.py:42,67): nine SparseConvMode values -- entry 0 for the stem, the down- and
        up-sampling convolutions and `final`, entries 1..8 for block1..block8 (their shortcut convolutions included)."""
        super().__init__(D, ME=ME)
        ME = self._ME
        sm = [int(getattr(v, "value", v)) for v in sparse_mode]
        if len(sm) != 9:
            raise ValueError(f"sparse_mode takes nine entries (stem / sampling / final, block1..block8), got {len(sm)}")
        self.sparse_mode = tuple(sm)
        self.D, self.bn_momentum, self.nonlinearity = D, bn_momentum, nonlinearity
        self.PLANES, self.LAYERS = tuple(PLANES or self.PLANES), tuple(LAYERS or self.LAYERS)
        self.BLOCK, self.NORM_TYPE = BLOCK or self.BLOCK, NORM_TYPE or self.NORM_TYPE
        self._fused = bool(getattr(ME, "SUPPORTS_FUSED_NORM", False))
        P, exp = self.PLANES, self.BLOCK.expansion

        def unit(*convs):
            mods = []
            for c in convs:
                mods += [c, get_norm(self.NORM_TYPE, c.out_channels, D, bn_momentum=bn_momentum, ME=ME),
                         get_nonlinearity(nonlinearity, ME)()]
            u = _Unit(*mods)
            u.fused = self._fused
            return u

        def down(c):
            return unit(conv(c, c, kernel_size=2, stride=2, D=D, conv_mode=sm[0], ME=ME))

        def up(cin, cout):
            return unit(conv_tr(cin, cout, kernel_size=2, upsample_stride=2, D=D, conv_mode=sm[0], ME=ME))

        self.conv0p1s1 = unit(conv(in_channel, P[0], kernel_size=3, D=D, conv_mode=sm[0], ME=ME),
                              conv(P[0], P[0], kernel_size=3, D=D, conv_mode=sm[0], ME=ME))
        self.conv1p1s2 = down(P[0])
        self.inplanes = P[0]
        self.block1 = self._make_layer(P[0], self.LAYERS[0], sm[1])
        self.conv2p2s2 = down(self.inplanes)
        self.block2 = self._make_layer(P[1], self.LAYERS[1], sm[2])
        self.conv3p4s2 = down(self.inplanes)
        self.block3 = self._make_layer(P[2], self.LAYERS[2], sm[3])
        self.conv4p8s2 = down(self.inplanes)
        self.block4 = self._make_layer(P[3], self.LAYERS[3], sm[4])
        self.convtr4p16s2 = up(self.inplanes, P[4])
        self.inplanes = P[4] + P[2] * exp
        self.block5 = self._make_layer(P[4], self.LAYERS[4], sm[5])
        self.convtr5p8s2 = up(self.inplanes, P[5])
        self.inplanes = P[5] + P[1] * exp
        self.block6 = self._make_layer(P[5], self.LAYERS[5], sm[6])
        self.convtr6p4s2 = up(self.inplanes, P[6])
        self.inplanes = P[6] + P[0] * exp
        self.block7 = self._make_layer(P[6], self.LAYERS[6], sm[7])
        self.convtr7p2s2 = up(self.inplanes, P[7])
        self.inplanes = P[7] + P[0]
        self.block8 = self._make_layer(P[7], self.LAYERS[7], sm[8])
        self.final = conv(P[7] * exp, out_channel, kernel_size=1, stride=1, bias=True, D=D, conv_mode=sm[0], ME=ME)
        if self.INSSEG:  # the offset head of the *Ins variants (reference res16unet.py:308-321), on the width after block8
            w = self.inplanes
            self.offset_block = nn.Sequential(
                conv(w, w, kernel_size=1, stride=1, bias=True, D=D, ME=ME),
                get_norm(self.NORM_TYPE, w, D, bn_momentum=bn_momentum, ME=ME),
                get_nonlinearity(nonlinearity, ME)(),
                conv(w, 3, kernel_size=1, stride=1, bias=True, D=D, ME=ME),
            )
        for m in self.modules():  # reference weight_initialization (res16unet.py:384-389), extended to the affine
            # parameters of NORM_TYPE "LN" (nn.LayerNorm) and "IN" (weight / bias of shape (1, C))
            if isinstance(m, (nn.BatchNorm1d, nn.LayerNorm, ME.MinkowskiInstanceNorm)):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, conv_mode=0):
        ME, out_planes = self._ME, planes * self.BLOCK.expansion
        shortcut = None
        if self.inplanes != out_planes:
            shortcut = nn.Sequential(
                conv(self.inplanes, out_planes, kernel_size=1, stride=1, D=self.D, conv_mode=conv_mode, ME=ME),
                get_norm(self.NORM_TYPE, out_planes, D=self.D, bn_momentum=self.bn_momentum, ME=ME),
            )
        mk = dict(norm_type=self.NORM_TYPE, nonlinearity_type=self.nonlinearity, bn_momentum=self.bn_momentum, D=self.D,
                  conv_mode=conv_mode, ME=ME)
        seq = [self.BLOCK(self.inplanes, planes, stride=1, downsample=shortcut, **mk)]
        self.inplanes = out_planes
        seq += [self.BLOCK(self.inplanes, planes, stride=1, **mk) for _ in range(1, blocks)]
        return nn.Sequential(*seq)

    def _unet(self, x):
        """The U from the tensor-stride-1 SparseTensor `x` to the output of block8, without the classifier."""
        cat = self._ME.cat
        out_p1 = self.conv0p1s1(x)
        out_b1p2 = self.block1(self.conv1p1s2(out_p1))
        out_b2p4 = self.block2(self.conv2p2s2(out_b1p2))
        out_b3p8 = self.block3(self.conv3p4s2(out_b2p4))
        out = self.block4(self.conv4p8s2(out_b3p8))            # tensor stride 16
        out = self.block5(cat(self.convtr4p16s2(out), out_b3p8))  # 8
        out = self.block6(cat(self.convtr5p8s2(out), out_b2p4))   # 4
        out = self.block7(cat(self.convtr6p4s2(out), out_b1p2))   # 2
        return self.block8(cat(self.convtr7p2s2(out), out_p1))    # 1

    def forward(self, x):
        out = self._unet(x.sparse())
        if self.INSSEG:  # (offsets [N, 3], logits [N, out_channel]), both read back through the field's one inverse map
            return self.offset_block(out).slice(x).F, self.final(out).slice(x).F
        return self.final(out).slice(x).F


class Res16UNet14(Res16UNet):
    LAYERS = (1, 1, 1, 1, 1, 1, 1, 1)


class Res16UNet18(Res16UNet):
    LAYERS = (2, 2, 2, 2, 2, 2, 2, 2)


class Res16UNet34(Res16UNet):
    LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)


class Res16UNet50(Res16UNet):
    BLOCK = Bottleneck
    LAYERS = (2, 3, 4, 6, 2, 2, 2, 2)


class Res16UNet101(Res16UNet):
    BLOCK = Bottleneck
    LAYERS = (2, 3, 4, 23, 2, 2, 2, 2)


class Res16UNet14A(Res16UNet14):
    PLANES = (32, 64, 128, 256, 128, 128, 96, 96)


class Res16UNet14A2(Res16UNet14A):
    LAYERS = (1, 1, 1, 1, 2, 2, 2, 2)


class Res16UNet14B(Res16UNet14):
    PLANES = (32, 64, 128, 256, 128, 128, 128, 128)


class Res16UNet14B2(Res16UNet14B):
    LAYERS = (1, 1, 1, 1, 2, 2, 2, 2)


class Res16UNet14B3(Res16UNet14B):
    LAYERS = (2, 2, 2, 2, 1, 1, 1, 1)


class Res16UNet14C(Res16UNet14):
    PLANES = (32, 64, 128, 256, 192, 192, 128, 128)


class Res16UNet14D(Res16UNet14):
    PLANES = (32, 64, 128, 256, 384, 384, 384, 384)


class Res16UNet18A(Res16UNet18):
    PLANES = (32, 64, 128, 256, 128, 128, 96, 96)


class Res16UNet18B(Res16UNet18):
    PLANES = (32, 64, 128, 256, 128, 128, 128, 128)


class Res16UNet18C(Res16UNet18):
    PLANES = (32, 64, 128, 256, 256, 128, 96, 96)


class Res16UNet18D(Res16UNet18):
    PLANES = (32, 64, 128, 256, 384, 384, 384, 384)


class Res16UNet34A(Res16UNet34):
    PLANES = (32, 64, 128, 256, 256, 128, 64, 64)


class Res16UNet34B(Res16UNet34):
    PLANES = (32, 64, 128, 256, 256, 128, 64, 32)


class Res16UNet34C(Res16UNet34):
    PLANES = (32, 64, 128, 256, 256, 128, 96, 96)


class Res16UNet14AIns(Res16UNet14A):
    INSSEG = True


class Res16UNet14BIns(Res16UNet14B):
    INSSEG = True


class Res16UNet18AIns(Res16UNet18A):
    INSSEG = True


class Res16UNet18BIns(Res16UNet18B):
    INSSEG = True


class Res16UNet34CIns(Res16UNet34C):
    INSSEG = True


@gin.configurable
class EncodedRes16UNet(Res16UNet):
    """Res16UNet on learned per-point features (reference res16unet.py:604-706): the input channels are positionally encoded
    (no gradient), a per-point MLP `enc_mlp` brings them to ENC_PLANES[-1] channels, `.sparse()` averages the points of a voxel,
    the U runs up to block8, and a per-point MLP `dec_mlp` on [enc_mlp output | block8 output read back at the points] feeds the
    classifier.  `final` is a MinkowskiLinear here (keys final.linear.weight / .bias), not the U-Net's 1x1 convolution."""

    def __init__(self, in_channel, out_channel, ENC_PLANES=(32, 32), DEC_PLANES=(48, 48), D=3, ME=None, sparse_mode=(0,) * 9):
        Res16UNet.__init__(self, in_channel=ENC_PLANES[-1], out_channel=out_channel, D=D, ME=ME, sparse_mode=sparse_mode)
        self.ENC_PLANES, self.DEC_PLANES = tuple(ENC_PLANES), tuple(DEC_PLANES)
        ME = self._ME
        self.encoding = ME.MinkowskiPositionalEncoding(in_channel)
        self.enc_mlp = self._mlp((self.encoding.out_channels, *self.ENC_PLANES))
        self.dec_mlp = self._mlp((self._dec_in_channel(), *self.DEC_PLANES))
        self.final = ME.MinkowskiLinear(self.DEC_PLANES[-1], out_channel, bias=True)

    def _dec_in_channel(self):
        return self.inplanes + self.ENC_PLANES[-1]  # (inplanes: the width after block8)

    def _mlp(self, widths):
        ME = self._ME
        return nn.Sequential(*[nn.Sequential(ME.MinkowskiLinear(a, b, bias=True), get_nonlinearity(self.nonlinearity, ME)())
                               for a, b in zip(widths[:-1], widths[1:])])

    def _encode(self, x):
        """-> (the encoded field, enc_mlp of it, block8's output)"""
        ME = self._ME
        with torch.no_grad():
            enc = self.encoding(x)
        feat = self.enc_mlp(enc)
        return enc, feat, self._unet(feat.sparse(quantization_mode=ME.SparseTensorQuantizationMode.UNWEIGHTED_AVERAGE))

    def forward(self, x):
        _, feat, out = self._encode(x)
        return self.final(self.dec_mlp(self._ME.cat(feat, out.slice(feat)))).F


@gin.configurable
class EncodedRes16UNet2(EncodedRes16UNet):
    """The second form (reference res16unet.py:709-795): `dec_mlp` reads [the raw encoding | block8 output at the points]."""

    def __init__(self, in_channel, out_channel, ENC_PLANES=(32, 32), DEC_PLANES=(48, 48), D=3, ME=None, sparse_mode=(0,) * 9):
        EncodedRes16UNet.__init__(self, in_channel, out_channel, ENC_PLANES=ENC_PLANES, DEC_PLANES=DEC_PLANES, D=D, ME=ME,
                                  sparse_mode=sparse_mode)

    def _dec_in_channel(self):
        return self.encoding.out_channels + self.inplanes

    def forward(self, x):
        enc, feat, out = self._encode(x)
        return self.final(self.dec_mlp(self._ME.cat(enc, out.slice(feat)))).F
