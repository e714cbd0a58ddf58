"""2-D comparison models (counterpart of the reference's co3d_2d/src/model/models.py:9-34): `ResNetBased` = a
torchvision ResNet (zero_init_residual=True) with its `fc` replaced by Identity, followed by Dropout and
Linear(in_features, 51).  The ResNet itself is defined here on the dense layers of model/dense.py with torchvision's
module and parameter names (`model.conv1.weight`, `model.layer1.0.bn2.running_var`, `model.layer2.0.downsample.0.weight`
...), so a torchvision checkpoint loads unchanged.  `ViTBased` (:37-54) wraps the Vision Transformer of model/vit.py, which
keeps timm's parameter names (`model.blocks.0.attn.qkv.weight` ...) and runs its attention in csrc/attn.hip (csrc/attn16.hip
with `ViTBased.math = "bf16"`); `select_model`
routes the three `vit_*_patch16_224` names of the reference's configs to it.  The Bottleneck networks (`resnet50/101/152`,
`wide_resnet50_2/101_2`, `resnext50_32x4d`, `resnext101_32x8d`) are torchvision's too: stride on the 3x3 `conv2`, and for
ResNeXt a grouped `conv2` (32 groups) that runs in csrc/gconv.hip.  The `deit3_*` names of the reference's list (layer scale,
in no config) stay unknown names."""
import torch
import torch.nn as nn

from nerf_downstream_amd import gin_lite as gin

from . import dense, vit


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = dense.Conv2d(inplanes, planes, 3, stride, 1)
        self.bn1 = dense.BatchNorm2d(planes)
        self.conv2 = dense.Conv2d(planes, planes, 3, 1, 1)
        self.bn2 = dense.BatchNorm2d(planes)
        self.downsample = downsample

    def forward(self, x, grid):
        identity = x
        st = self.training
        h, g, p = self.conv1(x, grid, bn_stats=st)
        h = self.bn1(h, relu=True, partial=p)
        h, g, p = self.conv2(h, g, bn_stats=st)
        if self.downsample is not None:
            identity, _, pd = self.downsample[0](x, grid, bn_stats=st)
            identity = self.downsample[1](identity, partial=pd)
        return self.bn2(h, relu=True, residual=identity, partial=p), g


class Bottleneck(nn.Module):
    """torchvision's Bottleneck (v1.5: the stride sits on the 3x3 conv2): 1x1 -> 3x3 (grouped for ResNeXt) -> 1x1."""

    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None, groups=1, width_per_group=64):
        super().__init__()
        width = int(planes * (width_per_group / 64.0)) * groups
        self.conv1 = dense.Conv2d(inplanes, width, 1, 1, 0)
        self.bn1 = dense.BatchNorm2d(width)
        self.conv2 = dense.Conv2d(width, width, 3, stride, 1, groups=groups)
        self.bn2 = dense.BatchNorm2d(width)
        self.conv3 = dense.Conv2d(width, planes * self.expansion, 1, 1, 0)
        self.bn3 = dense.BatchNorm2d(planes * self.expansion)
        self.downsample = downsample

    def forward(self, x, grid):
        identity = x
        st = self.training
        h, g, p = self.conv1(x, grid, bn_stats=st)
        h = self.bn1(h, relu=True, partial=p)
        h, g, p = self.conv2(h, g, bn_stats=st)
        h = self.bn2(h, relu=True, partial=p)
        h, g, p = self.conv3(h, g, bn_stats=st)
        if self.downsample is not None:
            identity, _, pd = self.downsample[0](x, grid, bn_stats=st)
            identity = self.downsample[1](identity, partial=pd)
        return self.bn3(h, relu=True, residual=identity, partial=p), g


class _Downsample(nn.Sequential):
    pass


class ResNet(nn.Module):
    def __init__(self, layers, num_classes=1000, zero_init_residual=False, block=BasicBlock, groups=1, width_per_group=64):
        super().__init__()
        self.inplanes = 64
        self.block = block
        self.block_args = {} if block is BasicBlock else {"groups": groups, "width_per_group": width_per_group}
        self.conv1 = dense.Conv2d(3, 64, 7, 2, 3)
        self.bn1 = dense.BatchNorm2d(64)
        self.maxpool = dense.MaxPool2d(3, 2, 1)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.fc = nn.Linear(512 * block.expansion, num_classes)
        if zero_init_residual:
            for m in self.modules():
                if isinstance(m, BasicBlock):
                    nn.init.constant_(m.bn2.weight, 0)
                elif isinstance(m, Bottleneck):
                    nn.init.constant_(m.bn3.weight, 0)

    def _make_layer(self, planes, blocks, stride):
        block, out = self.block, planes * self.block.expansion
        down = None
        if stride != 1 or self.inplanes != out:
            down = _Downsample(dense.Conv2d(self.inplanes, out, 1, stride, 0), dense.BatchNorm2d(out))
        seq = [block(self.inplanes, planes, stride, down, **self.block_args)]
        self.inplanes = out
        seq += [block(out, planes, **self.block_args) for _ in range(1, blocks)]
        return nn.ModuleList(seq)

    def forward(self, images):
        x, grid = dense.to_rows(images)
        x, grid, p = self.conv1(x, grid, bn_stats=self.training)
        x = self.bn1(x, relu=True, partial=p)
        x, grid = self.maxpool(x, grid)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                x, grid = blk(x, grid)
        x = dense.global_avg_pool(x, grid)
        return self.fc(x) if not isinstance(self.fc, nn.Identity) else x


_LAYERS = {"resnet18": (2, 2, 2, 2), "resnet34": (3, 4, 6, 3)}
# name -> (layers, groups, width_per_group) of the Bottleneck networks, torchvision's table
_BOTTLENECK = {
    "resnet50": ((3, 4, 6, 3), 1, 64),
    "resnet101": ((3, 4, 23, 3), 1, 64),
    "resnet152": ((3, 8, 36, 3), 1, 64),
    "resnext50_32x4d": ((3, 4, 6, 3), 32, 4),
    "resnext101_32x8d": ((3, 4, 23, 3), 32, 8),
    "wide_resnet50_2": ((3, 4, 6, 3), 1, 128),
    "wide_resnet101_2": ((3, 4, 23, 3), 1, 128),
}


@gin.configurable
class ResNetBased(nn.Module):
    def __init__(self, model="resnet18", dropout_rate=0.2, pretrained=False):
        super().__init__()
        if model not in _LAYERS and model not in _BOTTLENECK:
            raise NameError(f"Unknown model name : {model} (BasicBlock ResNets {sorted(_LAYERS)} and Bottleneck / wide / ResNeXt "
                            f"networks {sorted(_BOTTLENECK)} are built here)")
        if pretrained:
            raise NotImplementedError("no network access for pretrained weights: load a torchvision state dict instead")
        if model in _LAYERS:
            net = ResNet(_LAYERS[model], zero_init_residual=True)
        else:
            layers, groups, width = _BOTTLENECK[model]
            net = ResNet(layers, zero_init_residual=True, block=Bottleneck, groups=groups, width_per_group=width)
        in_features = net.fc.in_features
        net.fc = nn.Identity()
        self.fc = nn.Linear(in_features, 51, bias=True)
        self.dropout = nn.Dropout(dropout_rate)
        self.model = net

    def forward(self, x):
        return self.fc(self.dropout(self.model(x)))


@gin.configurable
class ViTBased(nn.Module):
    """`img_size` (extension, for tests and small runs): a multiple of 16; `pos_embed` is sized to it.  `math`: "fp32", or
    "bf16" for the mixed-precision blocks of model/vit.py (bf16 linears, attention in csrc/attn16.hip); it goes with
    `run.precision = 16`, and the parameters and the state dict are the same in both."""

    def __init__(self, model="vit_small_patch16_224", pretrained=False, img_size=224, math="fp32"):
        super().__init__()
        if math not in vit.MATHS:
            raise ValueError(f"ViTBased.math={math!r}: one of {vit.MATHS}")
        self.math = math
        if model not in vit.SIZES:
            raise NameError(f"Unknown model name : {model} (Vision Transformers {sorted(vit.SIZES)} are built here)")
        if pretrained:
            raise NotImplementedError("no network access for pretrained weights: load a timm state dict instead")
        dim, depth, heads = vit.SIZES[model]
        self.model = vit.VisionTransformer(img_size=img_size, dim=dim, depth=depth, heads=heads, num_classes=51, math=math)

    def forward(self, x):
        return self.model(x)


def select_model(model_name):
    if model_name is None:
        raise NameError("Oops?")
    if model_name in vit.SIZES:
        return ViTBased(model_name)
    return ResNetBased(model_name)
