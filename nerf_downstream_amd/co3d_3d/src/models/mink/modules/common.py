"""Layer factories of the Mink-ResNet family (counterpart of the reference's
co3d_3d/src/models/mink/modules/common.py:22-32,73-125,128-179).  `conv_mode` 1 (SPARSE) and 2 (ZAXIS) build the weight-sparse
modules of modules/sparse_conv.py (HIP backend only); 3 (NATIVE) and 5 (SPARSE_DENSE) build the dense module, as the reference
does when MinkowskiEngine has no native weight-sparse operator; 4 (SKIP), the reference's timing stub, is refused.

Every factory takes the ME namespace to build from, so one model definition runs on the HIP
backend (default) and, in tests, on the CPU oracle."""
from nerf_downstream_amd import minkowski as _HIP_ME


POWERNORM_HINT = ("MinkowskiPowerNorm layers come from converting every batch norm of a network: "
                  "--ginb \"train.convert_powernorm=True\" / --ginb \"evaluate.convert_powernorm=True\", or "
                  "ME.MinkowskiPowerNorm.convert_powernorm(model)")


def default_me():
    return _HIP_ME


def get_norm(norm_type, n_channels, D=3, bn_momentum=0.1, ME=None):
    """"BN" / "IN" / "LN" (reference common.py:22-32).  "PN" (PowerNorm, part of the reference's pruning study) is not
    implemented as a norm type: the layer exists (ME.MinkowskiPowerNorm) and is reached by converting a network's batch norms
    (POWERNORM_HINT)."""
    ME = ME or _HIP_ME
    if norm_type == "BN":
        return ME.MinkowskiBatchNorm(n_channels, momentum=bn_momentum)
    if norm_type == "IN":
        return ME.MinkowskiInstanceNorm(n_channels)
    if norm_type == "LN":
        return ME.MinkowskiLayerNorm(n_channels)
    if norm_type == "PN":
        raise ValueError(f"Norm type: PN (PowerNorm) is not implemented as a norm type; use BN, IN or LN. {POWERNORM_HINT}")
    raise ValueError(f"Norm type: {norm_type} not supported (BN, IN and LN are; PN is not implemented)")


def takes_conv_stats(norm):
    """True for the norm layers that accept the column statistics a convolution computes in its epilogue
    (`conv(x, bn_stats=True)`): batch norm only -- per-sample and per-row statistics are not column sums."""
    return hasattr(norm, "bn")


def get_nonlinearity(nonlinearity_type, ME=None):
    ME = ME or _HIP_ME
    table = {"MinkowskiReLU": ME.MinkowskiReLU, 0: ME.MinkowskiReLU}
    if nonlinearity_type not in table:
        raise ValueError(f"nonlinearity {nonlinearity_type} not supported (only MinkowskiReLU is on the path)")
    return table[nonlinearity_type]


def _sparse_module(mode, ME, transpose):
    """The weight-sparse class for a non-zero `conv_mode`, or None where the reference falls through to the dense module
    (NATIVE, SPARSE_DENSE).  The sparse kernel exists on the HIP backend only: with an injected namespace a non-zero mode raises."""
    from . import sparse_conv as S

    m = S.as_mode(mode)
    if ME is not None and ME is not _HIP_ME:
        raise ValueError(f"conv_mode={m.name}: weight-sparse inference runs on the HIP backend only (an ME namespace was injected)")
    if m in (S.SparseConvMode.NATIVE, S.SparseConvMode.SPARSE_DENSE):
        return None
    S._check_mode(m)  # refuses SKIP
    return S.WeightSparseConvolutionTranspose if transpose else S.WeightSparseConvolution


def conv(in_planes, out_planes, kernel_size, stride=1, dilation=1, bias=False, D=-1, conv_mode=0, ME=None):
    assert D > 0, "Dimension must be a positive integer"
    mode = int(getattr(conv_mode, "value", conv_mode))
    if mode != 0:
        sparse = _sparse_module(mode, ME, transpose=False)
        if sparse is not None:
            return sparse(in_channels=in_planes, out_channels=out_planes, kernel_size=kernel_size, stride=stride,
                          dilation=dilation, bias=bias, dimension=D, sparse_mode=mode)
    ME = ME or _HIP_ME
    return ME.MinkowskiConvolution(in_channels=in_planes, out_channels=out_planes, kernel_size=kernel_size,
                                   stride=stride, dilation=dilation, bias=bias, dimension=D)


def conv_tr(in_planes, out_planes, kernel_size, upsample_stride=1, dilation=1, bias=False, D=-1, conv_mode=0, ME=None):
    """Up-sampling (transposed) convolution of the segmentation family (reference common.py:128-179)."""
    assert D > 0, "Dimension must be a positive integer"
    mode = int(getattr(conv_mode, "value", conv_mode))
    if mode != 0:
        sparse = _sparse_module(mode, ME, transpose=True)
        if sparse is not None:
            return sparse(in_channels=in_planes, out_channels=out_planes, kernel_size=kernel_size, stride=upsample_stride,
                          dilation=dilation, bias=bias, dimension=D, sparse_mode=mode)
    ME = ME or _HIP_ME
    return ME.MinkowskiConvolutionTranspose(in_channels=in_planes, out_channels=out_planes, kernel_size=kernel_size,
                                            stride=upsample_stride, dilation=dilation, bias=bias, dimension=D)
