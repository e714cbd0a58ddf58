"""nn.Module layer of the HIP backend: the ME modules the reference hot path instantiates
(SURVEY.md 8b).  Constructor signatures, parameter names (`kernel`, `bias`, `bn.*`) and
initialisation follow ME so reference checkpoints / configs map one to one."""
import math

import torch
import torch.nn as nn

from .. import gin_lite as gin
from . import functional as Fn
from .coords import ORIGIN_TS, CoordinateMapKey, _as_int
from .eltwise import ActivationFunction, ReLUFunction
from .field import FieldGatherCatFunction, lazy_index_csr
from .interp import InterpolationFunction
from .norm import (
    BatchNormFunction,
    BNReLUSumPoolFunction,
    InstanceNormFunction,
    LayerNormFunction,
    PowerNormFunction,
    SyncBatchNormFunction,
)
from .pool import (
    AvgPoolFunction,
    GlobalAvgPoolFunction,
    GlobalMaxPoolFunction,
    GlobalSumPoolFunction,
    OverlapSumPoolFunction,
    SparseMaxPoolFunction,
    SumPoolFunction,
)
from .posenc import PositionalEncodingFunction
from .tensor import SparseTensor, TensorField


def _features(input):
    """The feature matrix of a SparseTensor or a TensorField.  A field may come straight from the prepare stream: its
    manager, coordinates and features are made usable on the current stream first (TensorField._settle, once per field)."""
    if isinstance(input, TensorField):
        input._settle()
    return input.F


def _same_kind(input, features):
    """`features` on the rows of `input`: a TensorField with its coordinates and manager for a field (reference fcnn.py:143,
    pointnet.py:100-109 run Linear / BatchNorm / activation / Dropout on the points), a SparseTensor on its map otherwise."""
    if isinstance(input, TensorField):
        return input._like(features)
    return SparseTensor(features, input.coordinate_map_key, input.coordinate_manager)


def _check_same(input, other):
    if isinstance(input, TensorField):
        if not isinstance(other, TensorField) or other.coordinate_manager is not input.coordinate_manager or other.F.shape[0] != input.F.shape[0]:
            raise ValueError("TensorFields must share the coordinate manager and the rows")
    else:
        input._check(other)


def _sample_offsets(input):
    """int32 [B+1] device row ranges of the batch samples: the map's for a SparseTensor, the field's own rows for a TensorField."""
    m = input.coordinate_manager
    if isinstance(input, TensorField):
        input._settle()
        return m.field_batch_offsets(input.C)
    return m.batch_offsets(input.coordinate_map_key)


class MinkowskiNetwork(nn.Module):
    """Base class of reference models (models/mink/base_model.py:6-8)."""

    def __init__(self, D):
        super().__init__()
        self.D = D


KERNEL_SIZES = (1, 2, 3, 5, 7)


def _kernel_size(kernel_size):
    """The edge of a cubic kernel the convolution kernels implement, or ValueError naming what they do."""
    ks = list(kernel_size) if isinstance(kernel_size, (list, tuple)) else [kernel_size]
    if len(set(int(k) for k in ks)) != 1 or int(ks[0]) not in KERNEL_SIZES:
        raise ValueError(f"kernel_size={kernel_size!r}: implemented are the cubic kernels of size 1, 2 (offsets {{0,1}}), 3, 5 and 7 "
                         "(centred; 5 and 7 through csrc/conv_bigk.hip, fp32, strides 1 and 2); other sizes and anisotropic "
                         "kernels are not")
    return int(ks[0])


class MinkowskiConvolution(nn.Module):
    """ME.MinkowskiConvolution as called by `conv()` (modules/common.py:116-125).

    kernel: (K, Cin, Cout), or (Cin, Cout) when the kernel volume is 1 and every stride is 1
    (`use_mm`, witness sparse_conv.py:323-335); bias: (1, Cout).  Init U(+-1/sqrt(Cin*K))
    (sparse_conv.py:427-435)."""

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=None):
        super().__init__()
        assert dimension == 3, "the HIP backend implements dimension=3"
        assert kernel_generator is None and not expand_coordinates, "custom kernel generators are out of scope"
        self.in_channels, self.out_channels = in_channels, out_channels
        self.kernel_size, self.stride, self.dilation = _kernel_size(kernel_size), _as_int(stride), _as_int(dilation)
        self.kernel_volume = self.kernel_size ** 3
        self.dimension = dimension
        self.use_mm = self.kernel_volume == 1 and self.stride == 1
        shape = (in_channels, out_channels) if self.use_mm else (self.kernel_volume, in_channels, out_channels)
        self.kernel = nn.Parameter(torch.empty(*shape))
        self.bias = nn.Parameter(torch.empty(1, out_channels)) if bias else None
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.in_channels * self.kernel_volume)
        with torch.no_grad():
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def forward(self, input, coordinates=None, bn_stats=False):
        """`bn_stats` (extension): also produce the per-channel (sum, sum of squares) partials of the
        output while it is being written (attribute `_bn_partial` of the result), so that a
        MinkowskiBatchNorm in training mode applied to it skips its own reduction pass."""
        assert coordinates is None, "explicit output coordinates are out of scope"
        m = input.coordinate_manager
        in_key = input.coordinate_map_key
        holder = [] if (bn_stats and self.bias is None and not self.use_mm) else None
        if self.use_mm:  # plain matmul on the feature matrix, same coordinates
            out_key = in_key
            if input.F.shape[0] >= 4096 and self.kernel.requires_grad and torch.is_grad_enabled():
                out = Fn.PointwiseConvolutionFunction.apply(input.F, self.kernel, lambda m=m, k=in_key: m.identity_table(k))
            else:
                out = input.F.mm(self.kernel)
        else:
            out_key = m.stride(in_key, self.stride)
            ks, dil = self.kernel_size, self.dilation

            def table_fn(transposed, m=m, in_key=in_key, out_key=out_key):
                nbr, nbr_t = m.kernel_table(in_key, out_key, ks, dil, transposed=transposed)
                # (the 5^3 / 7^3 data gradient reads the transposed table as it is: no parity-class permutation)
                perm = m.class_perm(in_key) if transposed and self.stride == 2 and ks <= 3 else None
                return nbr, nbr_t, perm

            # stride 1 and an odd (centred) kernel: the transposed table is the table itself with the offsets
            # flipped; an even kernel (offsets {0,1}) has no such symmetry and takes the explicit transposed table
            same_map = self.stride == 1 and self.kernel_size % 2 == 1
            out = Fn.ConvolutionFunction.apply(input.F, self.kernel, table_fn, same_map, holder)
        if self.bias is not None:
            out = out + self.bias
        res = SparseTensor(out, out_key, m)
        if holder:
            res._bn_partial = holder[0]
        return res

    def extra_repr(self):
        return (f"in={self.in_channels}, out={self.out_channels}, kernel_size={self.kernel_size}, "
                f"stride={self.stride}, dilation={self.dilation}")


class MinkowskiConvolutionTranspose(MinkowskiConvolution):
    """ME.MinkowskiConvolutionTranspose as called by `conv_tr()` (reference modules/common.py:171-179;
    res16unet.py:196-206): up-samples from tensor stride ts to ts / stride onto the coordinate map that
    already exists there (the encoder's), out[i] += in[o] @ kernel[k] over the pairs (i, o, k) of the
    ordinary convolution fine -> coarse.  kernel: (K, Cin, Cout), init U(+-1/sqrt(Cout*K)) (ME initialises
    transposed kernels from the OUT channel count).

    On the device this is the data-gradient kernel of the down-sampling convolution run forward: a gather
    over the transposed neighbour table with rows grouped by parity class (CoordinateManager.class_perm), so a
    tile multiplies only the kernel offsets its rows can have.  kernel_size == stride (2: the Res16UNet family):
    one parent per voxel, one offset per tile.  kernel_size 3 over stride 2 (the ResUNet2 registration family): a
    fine voxel has up to eight parents and a parity class 1, 2, 4 or 8 live offsets among the 27 -- the table shape
    the data gradient of every stride-2 3x3x3 convolution of the ResNets has, through the same launch plan
    (tests/test_gpu_resunet.py checks this shape operator by operator against the oracle)."""

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False,
                 kernel_generator=None, expand_coordinates=False, convolution_mode=None, dimension=None):
        super().__init__(in_channels, out_channels, kernel_size, stride, dilation, bias, kernel_generator,
                         expand_coordinates, convolution_mode, dimension)
        assert self.stride == 2 and not self.use_mm, "the HIP backend up-samples by 2 (upsample_stride=2)"
        if self.kernel_size > 3:
            raise ValueError(f"MinkowskiConvolutionTranspose(kernel_size={self.kernel_size}): transposed convolutions are implemented "
                             "for kernel sizes 2 and 3 (the 5 and 7 cubes only for MinkowskiConvolution)")
        stdv = 1.0 / math.sqrt(self.out_channels * self.kernel_volume)
        with torch.no_grad():
            self.kernel.uniform_(-stdv, stdv)
            if self.bias is not None:
                self.bias.uniform_(-stdv, stdv)

    def forward(self, input, coordinates=None, bn_stats=False):
        assert coordinates is None, "explicit output coordinates are out of scope"
        m = input.coordinate_manager
        in_key = input.coordinate_map_key
        ts = in_key.get_tensor_stride()[0]
        if ts % self.stride or not m.has_level(ts // self.stride):
            raise RuntimeError(f"MinkowskiConvolutionTranspose: no coordinate map at tensor stride {ts // self.stride} to "
                               "up-sample onto (generative up-sampling is out of scope)")
        out_key = CoordinateMapKey(ts // self.stride)
        ks, dil = self.kernel_size, self.dilation

        def table_fn(transposed, m=m, in_key=in_key, out_key=out_key):
            # tables of the ordinary convolution fine (out_key) -> coarse (in_key), used the other way round
            nbr, nbr_t = m.kernel_table(out_key, in_key, ks, dil, transposed=True)
            if transposed:  # towards the coarse input: its rows gather their children
                return nbr_t, nbr, None
            return nbr_t, nbr, m.class_perm(out_key)

        out = Fn.ConvolutionFunction.apply(input.F, self.kernel, table_fn, False, None)
        if self.bias is not None:
            out = out + self.bias
        return SparseTensor(out, out_key, m)


def cat(*tensors):
    """ME.cat (reference res16unet.py:410-425): feature-wise concatenation of sparse tensors that share
    one coordinate map -- or of TensorFields that share a manager and their rows (reference fcnn.py:163), giving a
    TensorField.  When every argument is a strided slice whose gather is still pending (`y.slice(x)` at a tensor stride
    beyond 1), the concatenated rows are written by one launch (mink_field_gather_cat), bit for bit what torch.cat of the
    separate slices gives, forward and backward."""
    fields = [isinstance(t, TensorField) for t in tensors]
    if any(fields):
        if not all(fields):
            raise ValueError("ME.cat: SparseTensors and TensorFields cannot be mixed")
        first = tensors[0]
        for t in tensors[1:]:
            if t.coordinate_manager is not first.coordinate_manager or t.C.shape[0] != first.C.shape[0]:
                raise ValueError("TensorFields must share the coordinate manager and the rows")
        if len(tensors) <= 8 and all(t._F is None and t._pending is not None for t in tensors):
            out = FieldGatherCatFunction.apply(tuple(t._pending[1] for t in tensors), *[t._pending[0] for t in tensors])
        else:
            out = torch.cat([t.F for t in tensors], dim=1)
        return first._like(out)
    for t in tensors[1:]:
        tensors[0]._check(t)
    return SparseTensor(torch.cat([t.F for t in tensors], dim=1), tensors[0].coordinate_map_key,
                        tensors[0].coordinate_manager)


def _bn_momentum(bn):
    """The running-statistics update factor of `nn.BatchNorm1d`: `momentum`, or -- for momentum=None, the cumulative
    moving average -- 1 / num_batches_tracked (read after this step's increment; one host read-back, rare config)."""
    if bn.momentum is not None:
        return bn.momentum
    if bn.num_batches_tracked is None:
        return 0.0
    return 1.0 / max(float(bn.num_batches_tracked), 1.0)


class MinkowskiBatchNorm(nn.Module):
    """ME.MinkowskiBatchNorm: an `nn.BatchNorm1d` (attribute `bn`, so state-dict keys are
    `*.bn.weight` ... and the reference init loop resnet.py:101-105 finds it) applied to F.

    Extension used by this repo's fused blocks: `forward(x, relu=True, residual=r)` computes
    relu(bn(x) + r) in one pass (one HIP kernel forward, one reduction + one pass backward)."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True):
        super().__init__()
        self.bn = nn.BatchNorm1d(num_features, eps=eps, momentum=momentum, affine=affine,
                                 track_running_stats=track_running_stats)
        self.counted_by_parent = False  # a parent network may bump all BN step counters in one launch

    def forward(self, input, relu=False, residual=None):
        bn = self.bn
        training = bn.training or not bn.track_running_stats
        if training and bn.track_running_stats and not self.counted_by_parent:
            bn.num_batches_tracked += 1
        F = _features(input)
        if residual is not None:
            _check_same(input, residual)
        gamma = bn.weight if bn.affine else torch.ones(bn.num_features, device=F.device)
        beta = bn.bias if bn.affine else torch.zeros(bn.num_features, device=F.device)
        out = BatchNormFunction.apply(
            F, gamma, beta, bn.running_mean, bn.running_var, training,
            _bn_momentum(bn), bn.eps,
            residual.F if residual is not None else None, bool(relu),
            getattr(input, "_bn_partial", None) if training else None)
        return _same_kind(input, out)


class MinkowskiSyncBatchNorm(MinkowskiBatchNorm):
    """ME.MinkowskiSyncBatchNorm (reference train.py:106-107; off by default, train.py:83): batch
    statistics over the voxels of ALL ranks.  Falls back to local statistics when no process
    group is initialised or in eval mode."""

    def __init__(self, num_features, eps=1e-5, momentum=0.1, affine=True, track_running_stats=True, process_group=None):
        super().__init__(num_features, eps=eps, momentum=momentum, affine=affine, track_running_stats=track_running_stats)
        self.process_group = process_group

    def forward(self, input, relu=False, residual=None):
        import torch.distributed as dist

        bn = self.bn
        training = bn.training or not bn.track_running_stats
        if not (training and dist.is_available() and dist.is_initialized() and dist.get_world_size(self.process_group) > 1):
            return super().forward(input, relu=relu, residual=residual)
        if bn.track_running_stats and not self.counted_by_parent:
            bn.num_batches_tracked += 1
        if residual is not None:
            _check_same(input, residual)
        out = SyncBatchNormFunction.apply(
            _features(input), bn.weight, bn.bias, bn.running_mean, bn.running_var, _bn_momentum(bn),
            bn.eps, residual.F if residual is not None else None, bool(relu), self.process_group)
        return _same_kind(input, out)

    @classmethod
    def convert_sync_batchnorm(cls, module, process_group=None):
        """Recursively replace every MinkowskiBatchNorm by a MinkowskiSyncBatchNorm sharing its
        parameters and buffers (same contract as ME / torch.nn.SyncBatchNorm)."""
        if isinstance(module, MinkowskiBatchNorm) and not isinstance(module, MinkowskiSyncBatchNorm):
            bn = module.bn
            new = cls(bn.num_features, bn.eps, bn.momentum, bn.affine, bn.track_running_stats, process_group)
            new.bn = bn
            new.counted_by_parent = module.counted_by_parent
            new.train(module.training)
            return new
        for name, child in list(module.named_children()):
            setattr(module, name, cls.convert_sync_batchnorm(child, process_group))
        if hasattr(module, "_norms"):  # networks that keep a list of their norm layers
            module._norms = [m for m in module.modules() if isinstance(m, MinkowskiBatchNorm)]
        return module


class MinkowskiReLU(nn.Module):
    def __init__(self, inplace=False):
        super().__init__()
        self.inplace = inplace

    def forward(self, input):
        return _same_kind(input, ReLUFunction.apply(_features(input)))


class _Activation(nn.Module):
    """Pointwise activation on the feature matrix; subclasses name the ME class (modules/common.py:36-51 looks the
    classes up by `__name__`) and take torch's constructor arguments (`ARG` = the name of the shape parameter)."""

    KIND, ALPHA, ARG = None, 0.0, None

    def __init__(self, *args, **kwargs):
        super().__init__()
        self.alpha = self.ALPHA
        if self.ARG is not None:
            self.alpha = float(args[0] if args else kwargs.get(self.ARG, self.ALPHA))

    def forward(self, input):
        return _same_kind(input, ActivationFunction.apply(_features(input), self.KIND, self.alpha, None))


class MinkowskiLeakyReLU(_Activation):
    KIND, ALPHA, ARG = "leaky_relu", 0.01, "negative_slope"


class MinkowskiELU(_Activation):
    KIND, ALPHA, ARG = "elu", 1.0, "alpha"


class MinkowskiCELU(_Activation):
    KIND, ALPHA, ARG = "celu", 1.0, "alpha"


class MinkowskiSELU(_Activation):
    KIND = "selu"


class MinkowskiGELU(_Activation):
    KIND = "gelu"


class MinkowskiPReLU(nn.Module):
    """ME.MinkowskiPReLU = torch.nn.PReLU on F: `weight` [num_parameters] initialised to `init`."""

    def __init__(self, num_parameters=1, init=0.25):
        super().__init__()
        self.weight = nn.Parameter(torch.full((num_parameters,), float(init)))

    def forward(self, input):
        return _same_kind(input, ActivationFunction.apply(_features(input), "prelu", 0.0, self.weight))


class MinkowskiInstanceNorm(nn.Module):
    """ME.MinkowskiInstanceNorm(num_features) (reference modules/common.py:25-26): every batch sample's voxels are
    normalised per channel by that sample's own mean / biased variance, then scaled and shifted by `weight` (ones) /
    `bias` (zeros).  The rows of one sample are contiguous: the segmented kernels of csrc/norm.hip read the manager's
    device-resident batch offsets, so the layer is three launches forward and four backward whatever the batch size, with
    no host synchronisation.  No running buffers: eval mode behaves as training mode.
    eps: ME's instance norm divides by sqrt(var + 1e-8) [ME-recall of MinkowskiInstanceNormFunction; parity unpinned: ME
    is absent and the reference holds no fixture for this layer -- it is only named by the layer factory, not used by a
    shipped model]; the value is an attribute so a caller that knows better can set it.

    Extension shared with MinkowskiBatchNorm: `forward(x, relu=True, residual=r)` computes relu(norm(x) + r) in one pass."""

    def __init__(self, num_features):
        super().__init__()
        self.num_features, self.eps = num_features, 1e-8
        self.weight = nn.Parameter(torch.ones(1, num_features))
        self.bias = nn.Parameter(torch.zeros(1, num_features))

    def forward(self, input, relu=False, residual=None):
        if residual is not None:
            _check_same(input, residual)
        out = InstanceNormFunction.apply(_features(input), self.weight.reshape(-1), self.bias.reshape(-1),
                                            _sample_offsets(input), self.eps,
                                            residual.F if residual is not None else None, bool(relu))
        return _same_kind(input, out)

    def extra_repr(self):
        return f"{self.num_features}, eps={self.eps}"


class MinkowskiLayerNorm(nn.Module):
    """ME.MinkowskiLayerNorm(num_features) (reference modules/common.py:27-28): an `nn.LayerNorm` (attribute `ln`, so
    state-dict keys are `*.ln.weight` / `*.ln.bias`) over the channels of every row of F -- one HIP launch forward, two
    backward (csrc/norm.hip), 1 <= num_features <= 512.  Takes a SparseTensor or a TensorField and returns the same kind.
    No running buffers: eval mode behaves as training mode.

    Extension shared with MinkowskiBatchNorm: `forward(x, relu=True, residual=r)` computes relu(norm(x) + r) in one pass."""

    def __init__(self, num_features, eps=1e-5, affine=True):
        super().__init__()
        if not 1 <= int(num_features) <= 512:
            raise ValueError(f"MinkowskiLayerNorm({num_features}): the row-wise kernels hold a row in registers and take at most 512 channels")
        self.ln = nn.LayerNorm(num_features, eps=eps, elementwise_affine=affine)

    def forward(self, input, relu=False, residual=None):
        ln = self.ln
        F = _features(input)
        if residual is not None:
            _check_same(input, residual)
        C = ln.normalized_shape[0]
        gamma = ln.weight if ln.weight is not None else torch.ones(C, device=F.device)
        beta = ln.bias if ln.bias is not None else torch.zeros(C, device=F.device)
        out = LayerNormFunction.apply(F, gamma, beta, ln.eps, residual.F if residual is not None else None, bool(relu))
        return _same_kind(input, out)


class _PowerNormState(nn.Module):
    """Parameters, buffers and settings of one PowerNorm layer under the names the reference's MaskPowerNorm gives them
    (modules/powernorm.py:142-177), so `*.pn.weight`, `*.pn.bias`, `*.pn.running_phi`, `*.pn.ema_gz` and `*.pn.iters` load
    key for key.  `weight` and `bias` are always parameters; `affine` is stored and ignored, as there."""

    def __init__(self, num_features, eps, alpha_fwd, alpha_bkw, affine, warmup_iters, group_num):
        super().__init__()
        self.num_features, self.eps, self.affine = num_features, eps, affine
        self.weight = nn.Parameter(torch.ones(num_features))
        self.bias = nn.Parameter(torch.zeros(num_features))
        self.register_buffer("running_phi", torch.ones(1, num_features, 1, 1))
        self.register_buffer("ema_gz", torch.zeros(1, num_features, 1, 1))
        self.register_buffer("iters", torch.zeros(1, dtype=torch.int64))
        self.afwd, self.abkw = alpha_fwd, alpha_bkw
        self.warmup_iters, self.group_num = warmup_iters, group_num


@gin.configurable
class MinkowskiPowerNorm(nn.Module):
    """The reference's MinkowskiPowerNorm (modules/powernorm.py:246-329): every row is scaled by the root second moment of
    each of its `group_num` channel groups, every channel by the root of the batch's second moment (the first
    `warmup_iters` training steps) or of the running one `pn.running_phi` (afterwards, and in eval mode); no mean is
    subtracted.  The backward is PowerNorm's approximate derivative with the running state `pn.ema_gz`.  The step counter
    `pn.iters`, the warm-up branch and the buffer updates live on the device (csrc/powernorm.hip): no host synchronisation
    per layer and step, where the reference reads the counter back with `.item()`.
    Takes a SparseTensor or a TensorField and returns the same kind; at most 4096 channels, divisible by `group_num`.
    Statistics and `ema_gz` are local to a rank under data parallelism.

    Extension shared with MinkowskiBatchNorm: `forward(x, relu=True, residual=r)` computes relu(norm(x) + r) in one pass."""

    def __init__(self, num_features, eps=1e-5, alpha_fwd=0.9, alpha_bkw=0.9, affine=True, warmup_iters=10000, group_num=1):
        super().__init__()
        if int(group_num) < 1 or int(num_features) % int(group_num):
            raise ValueError(f"MinkowskiPowerNorm({num_features}, group_num={group_num}): the channels must divide into the groups")
        self.pn = _PowerNormState(num_features, eps, alpha_fwd, alpha_bkw, affine, warmup_iters, group_num)

    def forward(self, input, relu=False, residual=None):
        pn = self.pn
        if residual is not None:
            _check_same(input, residual)
        out = PowerNormFunction.apply(
            _features(input), pn.weight, pn.bias, pn.running_phi, pn.ema_gz, pn.iters, pn.training, pn.eps, pn.afwd, pn.abkw,
            pn.warmup_iters, pn.group_num, residual.F if residual is not None else None, bool(relu))
        return _same_kind(input, out)

    def __repr__(self):
        pn = self.pn
        return (f"{self.__class__.__name__}({pn.num_features}, eps={pn.eps}, affine={pn.affine}, alpha_fwd={pn.afwd}, "
                f"alpha_bkw={pn.abkw}, warmup_iters={pn.warmup_iters}, group_num={pn.group_num})")

    @classmethod
    def convert_powernorm(cls, module):
        """Recursively replace every MinkowskiBatchNorm (its synchronised subclass included) by a
        MinkowskiPowerNorm(C, eps=bn.eps, affine=bn.affine) that shares `weight` and `bias`, takes `running_var` as
        `running_phi` and `num_batches_tracked` as `iters`; `running_mean` is dropped (reference powernorm.py:291-329).
        Networks that cached what they know about their batch norms (the list of step counters one launch bumps, the native
        trunk's plan) are told to look again: a converted network runs module by module."""
        if isinstance(module, MinkowskiBatchNorm):
            bn = module.bn
            new = cls(bn.num_features, eps=bn.eps, affine=bn.affine)
            pn = new.pn
            if bn.affine:
                pn.weight, pn.bias = bn.weight, bn.bias
            ref = bn.weight if bn.affine else bn.running_var
            if ref is not None:
                new.to(ref.device)
            if bn.running_var is not None:
                pn.running_phi = bn.running_var.detach().reshape(1, -1, 1, 1)
            if bn.num_batches_tracked is not None:
                pn.iters = bn.num_batches_tracked.detach().reshape(1)
            new.train(module.training)
            return new
        for name, child in list(module.named_children()):
            setattr(module, name, cls.convert_powernorm(child))
        if hasattr(module, "_norms"):  # the batch norms whose step counters the network bumps in one launch: none are left below
            module._norms = [m for m in module.modules() if isinstance(m, MinkowskiBatchNorm)]
        if hasattr(module, "_trunk_plan"):
            module._trunk_plan = None
        return module


class MinkowskiLinear(nn.Module):
    """ME.MinkowskiLinear: torch.nn.Linear on the feature matrix (same parameter names through `.linear`)."""

    def __init__(self, in_features, out_features, bias=True):
        super().__init__()
        self.linear = nn.Linear(in_features, out_features, bias=bias)

    def forward(self, input):
        return _same_kind(input, self.linear(_features(input)))


@gin.configurable
class MinkowskiPositionalEncoding(nn.Module):
    """Sinusoidal encoding of every feature channel of a SparseTensor or a TensorField (reference
    models/mink/modules/encoding.py:74-209); the result is of the same kind on the same manager.

    With L = num_encoding_functions and C = in_channel there are Q = 2 L C encoded columns, and column q is
    sin(frequencies[q] * x[:, q // (2L)] + offset[0, q]) with frequencies[q] = f[q mod L].  f_j = 2^j, or with `min_resolution`
    f = 2 ** linspace(m - L - 1, m, L), m = log2(0.5 / min_resolution): L + 1 octaves in L steps, not L - 1 -- a quirk of the
    reference that trained weights depend on, kept.  A second one, kept for the same reason: the phase is 0 for q < C L and
    pi / 2 for q >= C L, a split by COLUMN, not per channel -- so the channels of the first half get their L sines twice and
    those of the second half their L cosines twice (the middle channel of an odd C gets both).
    `include_original_channel_range = (lo, hi)` appends x[:, lo:hi] after the Q columns.  L < 1: the identity, no state.

    State dict as the reference's three non-trainable parameters: `coo` int64 [2, Q] = rows (q // (2L), q) (the layout of the
    reference's sparse matrix; not read here), `frequencies` fp32 [Q], `offset` fp32 [1, Q].  The kernel (mink_posenc_fwd)
    reads `frequencies` and `offset`, so a loaded checkpoint's values rule."""

    def __init__(self, in_channel, num_encoding_functions=4, include_original_channel_range=None, min_resolution=None):
        super().__init__()
        C, L = int(in_channel), int(num_encoding_functions)
        self.num_encoding_functions, self.include_original_channel_range = L, include_original_channel_range
        if L < 1:
            self.shape = (C, C)
            return
        if include_original_channel_range is not None:
            lo, hi = (int(v) for v in include_original_channel_range)
            if not 0 <= lo <= hi <= C:
                raise ValueError(f"include_original_channel_range={include_original_channel_range}: 0 <= lo <= hi <= {C}")
            self.include_original_channel_range = (lo, hi)
        if min_resolution is not None:
            if not isinstance(min_resolution, (int, float)) or min_resolution <= 0:
                raise ValueError(f"min_resolution={min_resolution!r} must be a positive number")
            top = math.log2(0.5 / min_resolution)
            f = 2.0 ** torch.linspace(top - L - 1, top, L)
        else:
            f = 2.0 ** torch.arange(L)
        Q = 2 * L * C
        q = torch.arange(Q)
        self.out_enc_channel = Q
        self.coo = nn.Parameter(torch.stack([q // (2 * L), q]), requires_grad=False)
        self.frequencies = nn.Parameter(f.float()[q % L].contiguous(), requires_grad=False)
        self.offset = nn.Parameter(((q >= C * L).float() * (math.pi / 2)).view(1, Q), requires_grad=False)
        lo, hi = self.include_original_channel_range or (0, 0)
        self.shape = (C, Q + hi - lo)

    @property
    def out_channels(self):
        return self.shape[1]

    def extra_repr(self):
        return f"in_channel={self.shape[0]}, out_channel={self.shape[1]}, num_encoding_functions={self.num_encoding_functions}"

    def forward(self, input):
        if self.num_encoding_functions < 1:
            return input
        F = _features(input)
        if F.dim() != 2 or F.shape[1] != self.shape[0]:
            raise ValueError(f"MinkowskiPositionalEncoding: {tuple(F.shape)} features, in_channel = {self.shape[0]}")
        lo, hi = self.include_original_channel_range or (0, 0)
        out = PositionalEncodingFunction.apply(F, self.frequencies, self.offset.view(-1), self.num_encoding_functions, lo, hi)
        return _same_kind(input, out)


class MinkowskiDropout(nn.Module):
    def __init__(self, p=0.5, inplace=False):
        super().__init__()
        self.p = p

    def forward(self, input):
        return _same_kind(input, nn.functional.dropout(_features(input), self.p, self.training))


def _local_pool_args(name, kernel_size, stride, dilation, kernel_generator, dimension):
    """(kernel_size, stride) of a local pooling layer, or ValueError naming the limit: dimension 3, dilation 1, no custom
    kernel generator, a kernel that is odd (centred offsets) or equal to the stride (offsets {0..k-1}) with at most 27 cells."""
    if dimension != 3:
        raise ValueError(f"{name}: dimension={dimension!r}; the HIP backend implements dimension=3")
    if kernel_generator is not None:
        raise ValueError(f"{name}: custom kernel generators are not implemented (kernel_generator must be None)")
    try:
        ks, s, dil = _as_int(kernel_size), _as_int(stride), _as_int(dilation)
    except AssertionError as e:
        raise ValueError(f"{name}: {e}") from None
    if dil != 1:
        raise ValueError(f"{name}: dilation={dil}; only dilation=1 is implemented")
    if ks < 1 or s < 1:
        raise ValueError(f"{name}: kernel_size={ks}, stride={s}; both must be >= 1")
    if ks ** 3 > 27:
        raise ValueError(f"{name}: kernel_size={ks}; at most 27 kernel cells (kernel_size <= 3) are implemented")
    if ks % 2 == 0 and ks != s:
        raise ValueError(f"{name}: kernel_size={ks}, stride={s}; the kernel size must be odd or equal to the stride")
    return ks, s


class _LocalPooling(nn.Module):
    """Local pooling on the coordinate map `CoordinateManager.stride(in_key, stride)` (the input map for stride 1) through the
    neighbour tables the convolutions use: kernel_table(in_key, out_key, kernel_size, 1, transposed=True)."""

    def __init__(self, kernel_size, stride=1, dilation=1, kernel_generator=None, dimension=None):
        super().__init__()
        self.kernel_size, self.stride = _local_pool_args(type(self).__name__, kernel_size, stride, dilation, kernel_generator,
                                                         dimension)
        self.dilation, self.dimension = 1, dimension

    def _tables(self, input):
        m, in_key = input.coordinate_manager, input.coordinate_map_key
        out_key = m.stride(in_key, self.stride)
        nbr, nbr_t = m.kernel_table(in_key, out_key, self.kernel_size, 1, transposed=True)
        return m, out_key, nbr, nbr_t

    def extra_repr(self):
        return f"kernel_size={self.kernel_size}, stride={self.stride}, dilation=1"


class MinkowskiAvgPooling(_LocalPooling):
    """ME.MinkowskiAvgPooling(kernel_size, stride=1, dilation=1, kernel_generator=None, dimension=None) (reference co3d.py:107,
    scannet.py:511): every output voxel is the sum of the input voxels present in its window divided by HOW MANY are present,
    not by the kernel volume [ME-recall of MinkowskiAvgPooling; parity unpinned: ME is absent and the reference holds no
    fixture for this layer].  Windows may overlap (kernel_size=3, stride=2 or 1); stride 1 pools onto the input map."""

    def forward(self, input):
        m, out_key, nbr, nbr_t = self._tables(input)
        out, _ = AvgPoolFunction.apply(input.F, nbr, nbr_t)
        return SparseTensor(out, out_key, m)


class MinkowskiMaxPooling(_LocalPooling):
    """ME.MinkowskiMaxPooling(kernel_size, stride=1, dilation=1, kernel_generator=None, dimension=None) (reference fcnn.py:121:
    kernel_size=3, stride=2): the channel-wise maximum over the input voxels present in the window; on a tie the gradient goes
    to the first present voxel in kernel-offset order."""

    def forward(self, input):
        m, out_key, nbr, nbr_t = self._tables(input)
        out, _ = SparseMaxPoolFunction.apply(input.F, nbr, nbr_t)
        return SparseTensor(out, out_key, m)


class MinkowskiSumPooling(nn.Module):
    """ME.MinkowskiSumPooling(kernel_size=2, stride=2, dimension=3) (resnet.py:62-64).  kernel_size == stride is the
    non-overlapping pooling of the ResNet stem (its own kernels and fused forms); an odd kernel_size != stride (3 over
    stride 2 or 1) sums overlapping windows through the kernels of MinkowskiAvgPooling, without the division."""

    def __init__(self, kernel_size, stride=1, dilation=1, kernel_generator=None, dimension=None):
        super().__init__()
        self.kernel_size, self.stride = _local_pool_args("MinkowskiSumPooling", kernel_size, stride, dilation, kernel_generator,
                                                         dimension)
        self.overlapping = self.kernel_size != self.stride

    def forward(self, input, norm=None, conv=None):
        """`norm` (extension): a MinkowskiBatchNorm to apply, followed by ReLU, to `input` on the
        fly -- pool(relu(norm(input))) in one pass without materialising the normalised tensor (any
        other norm layer -- instance norm, layer norm, SyncBN -- runs as norm(input, relu=True), then the pooling).
        `conv` (extension, with `norm`): a MinkowskiConvolution to apply first --
        pool(relu(norm(conv(input)))), the stem of the reference ResNets, as one autograd node
        whose backward never materialises the gradient of the convolution output either."""
        if conv is not None:
            fused = self._conv_norm_pool(input, norm, conv)
            if fused is not None:
                return fused
            input = conv(input, bn_stats=isinstance(norm, MinkowskiBatchNorm) and norm.bn.training)
        m, in_key = input.coordinate_manager, input.coordinate_map_key
        if self.overlapping:  # (no fused forms: the norm, if any, runs as its own layer)
            if norm is not None:
                input = norm(input, relu=True)
            out_key = m.stride(in_key, self.stride)
            nbr, nbr_t = m.kernel_table(in_key, out_key, self.kernel_size, 1, transposed=True)
            out, _ = OverlapSumPoolFunction.apply(input.F, nbr, nbr_t)
            return SparseTensor(out, out_key, m)
        out_key = m.stride(in_key, self.stride)
        nbr, _ = m.kernel_table(in_key, out_key, self.kernel_size, 1)
        i2o = m.stride_map(in_key, out_key)
        fusable = type(norm) is MinkowskiBatchNorm and norm.bn.affine
        if fusable and (norm.bn.training or not torch.is_grad_enabled()):
            bn = norm.bn
            training = bn.training or not bn.track_running_stats
            if training and bn.track_running_stats and not norm.counted_by_parent:
                bn.num_batches_tracked += 1
            out = BNReLUSumPoolFunction.apply(input.F, bn.weight, bn.bias, bn.running_mean, bn.running_var, training,
                                                 _bn_momentum(bn), bn.eps, nbr, i2o,
                                                 getattr(input, "_bn_partial", None) if training else None)
        else:
            if norm is not None:
                input = norm(input, relu=True)
            out = SumPoolFunction.apply(input.F, nbr, i2o)
        return SparseTensor(out, out_key, m)


    def _conv_norm_pool(self, input, norm, conv):
        """The fully fused stem, or None when it does not apply (eval mode, input gradient wanted,
        conv with bias / stride, SyncBN, or a shape the streaming weight-gradient kernel leaves
        to the general one)."""
        if (self.overlapping or norm is None or type(norm) is not MinkowskiBatchNorm or not norm.bn.affine or not norm.bn.training
                or not norm.bn.track_running_stats or conv.bias is not None or conv.use_mm or conv.stride != 1
                or conv.kernel_volume != 27 or conv.dilation != 1 or input.F.requires_grad or not torch.is_grad_enabled()):
            return None
        m, in_key = input.coordinate_manager, input.coordinate_map_key
        nbr, _ = m.kernel_table(in_key, in_key, conv.kernel_size, conv.dilation)
        if not Fn.ConvBNReLUSumPoolFunction.supported(input.F, conv.kernel, nbr):
            return None
        out_key = m.stride(in_key, self.stride)
        nbr_pool, _ = m.kernel_table(in_key, out_key, self.kernel_size, 1)
        i2o = m.stride_map(in_key, out_key)
        bn = norm.bn
        if not norm.counted_by_parent:
            bn.num_batches_tracked += 1
        out = Fn.ConvBNReLUSumPoolFunction.apply(
            input.F, conv.kernel, bn.weight, bn.bias, bn.running_mean, bn.running_var,
            _bn_momentum(bn), bn.eps, nbr, nbr_pool, i2o)
        return SparseTensor(out, out_key, m)


class MinkowskiGlobalAvgPooling(nn.Module):
    """ME.MinkowskiGlobalAvgPooling() (resnet.py:15-22): row b of the output is batch index b."""

    def forward(self, input):
        out = GlobalAvgPoolFunction.apply(_features(input), _sample_offsets(input))
        return SparseTensor(out, CoordinateMapKey(ORIGIN_TS), input.coordinate_manager)


class MinkowskiGlobalMaxPooling(nn.Module):
    """ME.MinkowskiGlobalMaxPooling() (reference fcnn.py:12, pointnet.py:90): row b of the output is the channel-wise maximum
    over the voxels of batch index b (zeros for a sample without voxels), on the origin map like MinkowskiGlobalAvgPooling --
    so ME.cat(global_max(x), global_avg(x)) is the head of fcnn.py:15-18.  Segmented over the manager's device-resident batch
    offsets: two launches forward, one backward whatever the batch size, no host synchronisation."""

    def __init__(self):
        super().__init__()

    def forward(self, input):
        out, _ = GlobalMaxPoolFunction.apply(_features(input), _sample_offsets(input))
        return SparseTensor(out, CoordinateMapKey(ORIGIN_TS), input.coordinate_manager)


class MinkowskiGlobalSumPooling(nn.Module):
    """ME.MinkowskiGlobalSumPooling(): row b of the output is the sum over the voxels of batch index b (accumulated in double)."""

    def __init__(self):
        super().__init__()

    def forward(self, input):
        out = GlobalSumPoolFunction.apply(_features(input), _sample_offsets(input))
        return SparseTensor(out, CoordinateMapKey(ORIGIN_TS), input.coordinate_manager)


class MinkowskiInterpolation(nn.Module):
    """ME.MinkowskiInterpolation(return_kernel_map=False, return_weights=False) (reference data/transforms.py:472,514-521)
    [ME-recall of interpolation_map_weight; parity unpinned, ME is absent]: forward(input, tfield) reads the SparseTensor
    `input`, at any tensor stride, at the float rows tfield[N, 4] = (b, x, y, z) by trilinear interpolation -> a tensor
    [N, C].  A corner absent from the map contributes nothing (no renormalisation); the gradient goes to the features only.
    With `return_kernel_map=True` or `return_weights=True` the result is ME's tuple (features, in_map, out_map, weights): the
    found entries in (query, corner) order, in_map = rows of `input`, out_map = rows of tfield (one host synchronisation)."""

    def __init__(self, return_kernel_map=False, return_weights=False):
        super().__init__()
        self.return_kernel_map, self.return_weights = bool(return_kernel_map), bool(return_weights)

    def forward(self, input, tfield):
        imap, w = input.coordinate_manager.interpolation_map_weight(input.coordinate_map_key, tfield)
        out = InterpolationFunction.apply(input.F, imap, w, lazy_index_csr(imap, input.F.shape[0]))
        if not (self.return_kernel_map or self.return_weights):
            return out
        flat = imap.reshape(-1)
        found = torch.nonzero(flat >= 0).reshape(-1)
        return out, flat[found].long(), found // 8, w.reshape(-1)[found]
