"""A small sparse occupancy autoencoder in the shape of ME's completion / reconstruction examples: the encoder strides the
input map down, every decoder block GENERATES the children of its voxels, classifies them and PRUNES those it takes for empty --
the one network family here whose coordinate maps are made inside the network (minkowski/generative.py, csrc/generate.hip)."""
import torch
import torch.nn.functional as F

from .base_model import MinkowskiBaseModel


class _DecoderBlock(torch.nn.Module):
    """generative transpose -> BN -> ReLU -> 3x3x3 conv -> BN -> ReLU -> 1x1x1 classifier (one logit per voxel) -> pruning"""

    def __init__(self, ME, cin, cout):
        super().__init__()
        self.up = ME.MinkowskiGenerativeConvolutionTranspose(cin, cout, kernel_size=2, stride=2, dimension=3)
        self.bn1 = ME.MinkowskiBatchNorm(cout)
        self.conv = ME.MinkowskiConvolution(cout, cout, kernel_size=3, stride=1, dimension=3)
        self.bn2 = ME.MinkowskiBatchNorm(cout)
        self.cls = ME.MinkowskiConvolution(cout, 1, kernel_size=1, stride=1, bias=True, dimension=3)
        self.relu = ME.MinkowskiReLU()
        self.prune = ME.MinkowskiPruning()


class CompletionNet(MinkowskiBaseModel):
    """Encoder: two stride-2 3x3x3 conv-BN-ReLU stages (tensor stride 1 -> 2 -> 4).  Decoder: two blocks (4 -> 2 -> 1).

    `forward(x, target=None)` -> (levels, out): `levels` holds one (logits SparseTensor, occupancy target bool [n] or None)
    pair per decoder block, over every voxel the block generated; `out` is the last block's tensor after pruning.  With a
    `target` (a SparseTensor whose coordinate map is the shape to reconstruct, usually on another manager) a block keeps the
    voxels of the target -- teacher forcing -- and, in training mode, also those its own classifier takes for occupied
    (ME's examples: `keep = logits > 0; if self.training: keep += target`); without one it keeps `logits > 0`.
    `out_channel` is unused: every level predicts one occupancy logit per voxel."""

    CHANNELS = (16, 32)

    def __init__(self, in_channel, out_channel=1, ME=None):
        super().__init__(3, ME)
        ME = self._ME
        c1, c2 = self.CHANNELS
        self.enc1 = ME.MinkowskiConvolution(in_channel, c1, kernel_size=3, stride=2, dimension=3)
        self.enc_bn1 = ME.MinkowskiBatchNorm(c1)
        self.enc2 = ME.MinkowskiConvolution(c1, c2, kernel_size=3, stride=2, dimension=3)
        self.enc_bn2 = ME.MinkowskiBatchNorm(c2)
        self.relu = ME.MinkowskiReLU()
        self.dec1 = _DecoderBlock(ME, c2, c1)
        self.dec2 = _DecoderBlock(ME, c1, c1)

    def forward(self, x, target=None):
        ME = self._ME
        if isinstance(x, ME.TensorField):
            x = x.sparse()
        y = self.relu(self.enc_bn1(self.enc1(x)))
        y = self.relu(self.enc_bn2(self.enc2(y)))
        levels = []
        for blk in (self.dec1, self.dec2):
            y = blk.relu(blk.bn1(blk.up(y)))
            y = blk.relu(blk.bn2(blk.conv(y)))
            logits = blk.cls(y)
            pred = logits.F.detach()[:, 0] > 0
            occ = None
            if target is not None:
                occ = ME.generative.occupancy(logits, target)
                keep = occ | pred if self.training else occ
            else:
                keep = pred
            levels.append((logits, occ))
            y = blk.prune(y, keep)
        return levels, y

    @staticmethod
    def loss(levels):
        """The mean over the levels of binary cross-entropy with logits against each level's occupancy target."""
        return sum(F.binary_cross_entropy_with_logits(lg.F[:, 0], occ.to(lg.F.dtype)) for lg, occ in levels) / len(levels)


class _SkipDecoderBlock(_DecoderBlock):
    """generative transpose -> BN -> ReLU -> union with the encoder tensor of that tensor stride (the skip) -> 3x3x3 conv -> BN ->
    ReLU -> 1x1x1 classifier -> pruning"""

    def __init__(self, ME, cin, cout):
        super().__init__(ME, cin, cout)
        self.union = ME.MinkowskiUnion()


class CompletionUNet(MinkowskiBaseModel):
    """The U-shaped form of CompletionNet, as ME's completion and reconstruction networks are built: a stride-1 3x3x3 stem and
    three stride-2 3x3x3 conv-BN-ReLU stages (tensor stride 1 -> 2 -> 4 -> 8) whose tensors at strides 4, 2 and 1 are kept, and
    three decoder blocks (8 -> 4 -> 2 -> 1) that each join the children they generated with the encoder tensor of the same
    tensor stride over the UNION of the two coordinate maps (ME.MinkowskiUnion: the two live on different managers) before
    they convolve, classify and prune.  So a voxel of the input survives to the classifier of its level whether or not the
    level above kept its parent.

    `forward(x, target=None)` -> (levels, out), the keep rule and `loss` are CompletionNet's."""

    CHANNELS = (16, 16, 32, 64)  # stem, then the three encoder stages

    def __init__(self, in_channel, out_channel=1, ME=None):
        super().__init__(3, ME)
        ME = self._ME
        c0, c1, c2, c3 = self.CHANNELS
        self.stem = ME.MinkowskiConvolution(in_channel, c0, kernel_size=3, stride=1, dimension=3)
        self.stem_bn = ME.MinkowskiBatchNorm(c0)
        self.enc1 = ME.MinkowskiConvolution(c0, c1, kernel_size=3, stride=2, dimension=3)
        self.enc_bn1 = ME.MinkowskiBatchNorm(c1)
        self.enc2 = ME.MinkowskiConvolution(c1, c2, kernel_size=3, stride=2, dimension=3)
        self.enc_bn2 = ME.MinkowskiBatchNorm(c2)
        self.enc3 = ME.MinkowskiConvolution(c2, c3, kernel_size=3, stride=2, dimension=3)
        self.enc_bn3 = ME.MinkowskiBatchNorm(c3)
        self.relu = ME.MinkowskiReLU()
        self.dec1 = _SkipDecoderBlock(ME, c3, c2)
        self.dec2 = _SkipDecoderBlock(ME, c2, c1)
        self.dec3 = _SkipDecoderBlock(ME, c1, c0)

    def forward(self, x, target=None):
        ME = self._ME
        if isinstance(x, ME.TensorField):
            x = x.sparse()
        s1 = self.relu(self.stem_bn(self.stem(x)))
        s2 = self.relu(self.enc_bn1(self.enc1(s1)))
        s4 = self.relu(self.enc_bn2(self.enc2(s2)))
        y = self.relu(self.enc_bn3(self.enc3(s4)))
        levels = []
        for blk, skip in ((self.dec1, s4), (self.dec2, s2), (self.dec3, s1)):
            y = blk.relu(blk.bn1(blk.up(y)))
            y = blk.union(y, skip)
            y = blk.relu(blk.bn2(blk.conv(y)))
            logits = blk.cls(y)
            pred = logits.F.detach()[:, 0] > 0
            occ = None
            if target is not None:
                occ = ME.generative.occupancy(logits, target)
                keep = occ | pred if self.training else occ
            else:
                keep = pred
            levels.append((logits, occ))
            y = blk.prune(y, keep)
        return levels, y

    loss = staticmethod(CompletionNet.loss)
