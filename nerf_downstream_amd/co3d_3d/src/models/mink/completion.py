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
