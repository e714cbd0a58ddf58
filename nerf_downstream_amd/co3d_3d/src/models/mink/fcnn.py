"""Point-based fully convolutional classifiers (counterpart of the reference's co3d_3d/src/models/mink/fcnn.py:9-208).

    points (TensorField)  -- mlp1: Linear - BN - LeakyReLU on every point
    .sparse() / .splat()                                              ts 1
    conv1 (s1) - max_pool -> y1 (ts 2),  conv2 (s2) - max_pool -> y2 (ts 8),
    conv3 (s2) - max_pool -> y3 (ts 32), conv4 (s2) - max_pool -> y4 (ts 128)
    y1..y4 read back at the points (slice / interpolate), concatenated per point, .sparse() again
    conv5: three stride-2 blocks up to embedding_channel, global max | global average, two MLP blocks, Linear -> logits

Module names and order follow the reference so state dicts map one to one: mlp1.{0.linear,1.bn}, conv{1..4}.{0,1.bn},
conv5.{0,1,2}.{0,1.bn}, final.{1,3}.{0.linear,1.bn}, final.4.linear (max_pool, final.0 and the dropout hold no parameters).
There is no native-trunk form of these networks: every layer runs as its own module."""
import torch.nn as nn

from nerf_downstream_amd import gin_lite as gin

from .base_model import MinkowskiBaseModel


class GlobalMaxAvgPool(nn.Module):
    def __init__(self, ME):
        super().__init__()
        self._cat = ME.cat
        self.global_max_pool = ME.MinkowskiGlobalMaxPooling()
        self.global_avg_pool = ME.MinkowskiGlobalAvgPooling()

    def forward(self, tensor):
        return self._cat(self.global_max_pool(tensor), self.global_avg_pool(tensor))


@gin.configurable
class MinkowskiFCNN(MinkowskiBaseModel):
    def __init__(self, in_channel, out_channel, kernel_size=3, embedding_channel=1024, channels=(32, 48, 64, 96, 128), D=3,
                 ME=None):
        super().__init__(D, ME=ME)
        self.network_initialization(in_channel, out_channel, channels=channels, embedding_channel=embedding_channel,
                                    kernel_size=kernel_size, D=D)
        self.weight_initialization()

    def get_mlp_block(self, in_channel, out_channel):
        ME = self._ME
        return nn.Sequential(ME.MinkowskiLinear(in_channel, out_channel, bias=False), ME.MinkowskiBatchNorm(out_channel),
                             ME.MinkowskiLeakyReLU())

    def get_conv_block(self, in_channel, out_channel, kernel_size, stride):
        ME = self._ME
        return nn.Sequential(ME.MinkowskiConvolution(in_channel, out_channel, kernel_size=kernel_size, stride=stride, dimension=self.D),
                             ME.MinkowskiBatchNorm(out_channel), ME.MinkowskiLeakyReLU())

    def network_initialization(self, in_channel, out_channel, channels, embedding_channel, kernel_size, D=3):
        ME = self._ME
        self.mlp1 = self.get_mlp_block(in_channel, channels[0])
        self.conv1 = self.get_conv_block(channels[0], channels[1], kernel_size=kernel_size, stride=1)
        self.conv2 = self.get_conv_block(channels[1], channels[2], kernel_size=kernel_size, stride=2)
        self.conv3 = self.get_conv_block(channels[2], channels[3], kernel_size=kernel_size, stride=2)
        self.conv4 = self.get_conv_block(channels[3], channels[4], kernel_size=kernel_size, stride=2)
        self.conv5 = nn.Sequential(
            self.get_conv_block(channels[1] + channels[2] + channels[3] + channels[4], embedding_channel // 4, kernel_size=3, stride=2),
            self.get_conv_block(embedding_channel // 4, embedding_channel // 2, kernel_size=3, stride=2),
            self.get_conv_block(embedding_channel // 2, embedding_channel, kernel_size=3, stride=2),
        )
        self.max_pool = ME.MinkowskiMaxPooling(kernel_size=3, stride=2, dimension=D)
        self.final = nn.Sequential(
            GlobalMaxAvgPool(ME),
            self.get_mlp_block(embedding_channel * 2, 512),
            ME.MinkowskiDropout(),
            self.get_mlp_block(512, 512),
            ME.MinkowskiLinear(512, out_channel, bias=True),
        )

    def weight_initialization(self):
        ME = self._ME
        for m in self.modules():
            if isinstance(m, ME.MinkowskiConvolution):
                ME.utils.kaiming_normal_(m.kernel, mode="fan_out", nonlinearity="relu")
            if isinstance(m, ME.MinkowskiBatchNorm):
                nn.init.constant_(m.bn.weight, 1)
                nn.init.constant_(m.bn.bias, 0)

    def _pyramid(self, y):
        y1 = self.max_pool(self.conv1(y))
        y2 = self.max_pool(self.conv2(y1))
        y3 = self.max_pool(self.conv3(y2))
        y4 = self.max_pool(self.conv4(y3))
        return y1, y2, y3, y4

    def forward(self, x):
        x = self.mlp1(x)
        ys = self._pyramid(x.sparse())
        x = self._ME.cat(*[y.slice(x) for y in ys])  # (HIP backend: the four gathers and the concatenation are one launch)
        y = self.conv5(x.sparse())
        return self.final(y).F


@gin.configurable
class MinkowskiSplatFCNN(MinkowskiFCNN):
    """The same network with the points spread over the corners of their cells (`splat`) instead of averaged per voxel, and the
    four stages read back by trilinear interpolation (reference fcnn.py:169-208)."""

    def __init__(self, in_channel, out_channel, kernel_size=3, embedding_channel=1024, channels=(32, 48, 64, 96, 128), D=3,
                 ME=None):
        MinkowskiFCNN.__init__(self, in_channel, out_channel, kernel_size, embedding_channel, channels, D, ME=ME)

    def forward(self, x):
        x = self.mlp1(x)
        ys = self._pyramid(x.splat())
        x = self._ME.cat(*[y.interpolate(x) for y in ys])
        y = self.conv5(x.sparse())
        return self.final(y).F
