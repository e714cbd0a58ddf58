"""Model registry (counterpart of the reference's co3d_3d/src/models/__init__.py:18-20:
lookup by class name through the gin-configurable `get_model`)."""
from nerf_downstream_amd import gin_lite as gin

from .mink.resnet import ResNet14, ResNet18, ResNet34, ResNet50, ResNet101

from .mink import res16unet as _unet
from .mink import resunet as _resunet
from .mink.completion import CompletionNet, CompletionUNet
from .mink.dgcnn import DGCNN_cls
from .mink.fcnn import MinkowskiFCNN, MinkowskiSplatFCNN
from .mink.paconv import PAConvDGCNN, PAConvPointNet
from .mink.pointnet import MinkowskiPointNet

MODELS = {c.__name__: c for c in (ResNet14, ResNet18, ResNet34, ResNet50, ResNet101)}
MODELS.update({n: c for n, c in vars(_unet).items() if n.startswith("Res16UNet") and isinstance(c, type)})
MODELS.update({c.__name__: c for c in (_unet.EncodedRes16UNet, _unet.EncodedRes16UNet2)})  # (the *Ins variants come by name above)
MODELS.update({n: c for n, c in vars(_resunet).items()  # registration feature extractors (ResUNet2 itself is abstract)
               if n.startswith("ResUNet") and isinstance(c, type) and c.NORM_TYPE is not None})
MODELS.update({c.__name__: c for c in (MinkowskiFCNN, MinkowskiSplatFCNN, MinkowskiPointNet, DGCNN_cls, PAConvPointNet, PAConvDGCNN)})  # point-based classifiers
MODELS[CompletionNet.__name__] = CompletionNet  # sparse occupancy autoencoder: generative transpose -> classifier -> pruning
MODELS[CompletionUNet.__name__] = CompletionUNet  # its U-shaped form: every decoder block joins the encoder tensor of its stride (MinkowskiUnion)


@gin.configurable
def get_model(name: str, in_channel, out_channel, sparse=None, ME=None):
    """`sparse`: the nine SparseConvMode values of the Res16UNet family (`sparse_mode`, reference res16unet.py:42; what the
    reference's `eval.py --sparsify --sparse_mode ...` binds).  Deliberate deviation: the reference's get_model
    (models/__init__.py:18-20) accepts the binding and drops it; here it reaches the network, and a model without weight-sparse
    layers raises when any entry is non-zero.  None or all zeros builds the dense model, unchanged."""
    if name not in MODELS:
        raise KeyError(f"model {name!r} is not implemented; available: {sorted(MODELS)}")
    modes = [int(getattr(v, "value", v)) for v in sparse] if sparse is not None else []
    if any(modes):
        if not issubclass(MODELS[name], _unet.Res16UNet):
            raise ValueError(f"get_model.sparse={list(sparse)!r}: only the Res16UNet family has weight-sparse layers, {name} does not")
        return MODELS[name](in_channel=in_channel, out_channel=out_channel, ME=ME, sparse_mode=modes)
    return MODELS[name](in_channel=in_channel, out_channel=out_channel, ME=ME)
