"""PointNet on a TensorField (counterpart of the reference's co3d_3d/src/models/mink/pointnet.py:61-109): five
Linear - BN - ReLU blocks on every point, a global max over the points of each batch sample -- which may hold any number
of points --, Linear - BN - ReLU, dropout, Linear -> logits.  No voxel is ever formed: the field's rows of one batch index
are the sample.  Module names follow the reference: conv{1..5}.{0.linear,1.bn}, linear1.{0.linear,1.bn}, linear2.linear.
The reference's dense `PointNet` and its `stack_collate_fn` (fixed point counts) are not part of this backend."""
import torch.nn as nn

from nerf_downstream_amd import gin_lite as gin

from .base_model import MinkowskiBaseModel


@gin.configurable
class MinkowskiPointNet(MinkowskiBaseModel):
    def __init__(self, in_channel, out_channel, embedding_channel=1024, dimension=3, ME=None):
        super().__init__(dimension, ME=ME)
        ME = self._ME

        def block(cin, cout):
            return nn.Sequential(ME.MinkowskiLinear(cin, cout, bias=False), ME.MinkowskiBatchNorm(cout), ME.MinkowskiReLU())

        self.conv1 = block(in_channel, 64)
        self.conv2 = block(64, 64)
        self.conv3 = block(64, 64)
        self.conv4 = block(64, 128)
        self.conv5 = block(128, embedding_channel)
        self.max_pool = ME.MinkowskiGlobalMaxPooling()
        self.linear1 = block(embedding_channel, 512)
        self.dp1 = ME.MinkowskiDropout()
        self.linear2 = ME.MinkowskiLinear(512, out_channel, bias=True)

    def forward(self, x):
        x = self.conv5(self.conv4(self.conv3(self.conv2(self.conv1(x)))))
        x = self.max_pool(x)
        x = self.linear1(x)
        x = self.dp1(x)
        return self.linear2(x).F
