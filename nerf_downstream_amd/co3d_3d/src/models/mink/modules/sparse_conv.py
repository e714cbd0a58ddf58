"""Weight-sparse convolutions for the inference of pruned networks (counterpart of the reference's
co3d_3d/src/models/mink/modules/sparse_conv.py: SparseConvMode :19-25, WeightSparseConvolutionBase :267-452,
WeightSparseConvolution :455-516, WeightSparseConvolutionTranspose :519-559).

The reference keeps one torch sparse matrix per kernel offset and drives one `spmm` per offset from Python; here `sparsify()`
packs the kernel once (minkowski/wsconv.py: pack_csr) and the forward pass is ONE launch of mink_wsconv_fwd.  Parameter names,
shapes and initialisation are those of MinkowskiConvolution(Transpose), so a dense checkpoint loads into a sparse-mode model;
the packed arrays are non-persistent buffers: they follow `.to()` and stay out of `state_dict()`.

Path choice: a sparsified layer whose density is above `wsconv.MAX_DENSITY` runs the dense gather-GEMM on its masked weights, one
at or below it the sparse kernel; `module.path = "sparse" | "dense"` forces either (tests and benchmarks do)."""
from enum import Enum

import torch

from nerf_downstream_amd.minkowski import functional as Fn
from nerf_downstream_amd.minkowski import wsconv
from nerf_downstream_amd.minkowski.coords import CoordinateMapKey
from nerf_downstream_amd.minkowski.modules import MinkowskiConvolution, MinkowskiConvolutionTranspose
from nerf_downstream_amd.minkowski.tensor import SparseTensor


class SparseConvMode(Enum):
    DENSE = 0
    SPARSE = 1
    ZAXIS = 2
    NATIVE = 3
    SKIP = 4
    SPARSE_DENSE = 5


LAYOUTS = ("csr", "coo", "strided")
ZAXIS_OFFSETS = [4, 13, 22]  # (0, 0, dz) of a 3x3x3 kernel, x fastest (reference sparse_conv.py:378-379)
_PACKED = ("koffs", "rowptr", "colidx", "vals", "cptr")


def as_mode(mode):
    """SparseConvMode from an enum member or its integer."""
    return mode if isinstance(mode, SparseConvMode) else SparseConvMode(int(mode))


def _check_mode(mode):
    mode = as_mode(mode)
    if mode is SparseConvMode.SKIP:
        raise ValueError("SparseConvMode.SKIP is the reference's timing stub (its layers return zeros or ones, sparse_conv.py:34-35,"
                         "49-50): it computes no convolution and is refused here")
    if mode not in (SparseConvMode.SPARSE, SparseConvMode.ZAXIS):
        raise ValueError(f"{mode}: a weight-sparse module takes SparseConvMode.SPARSE or ZAXIS (DENSE, NATIVE and SPARSE_DENSE are "
                         "the dense module, modules/common.py)")
    return mode


class _WeightSparse:
    """What the two modules share; mixed in ahead of the dense module whose parameters, init and tables they keep."""

    def _init_sparse(self, sparse_mode):
        self.sparse_mode = _check_mode(sparse_mode)
        self.valid_kernel, self.layout, self.path = [], None, None
        self.nnz, self.density, self._koff_list = 0, 1.0, []
        for name in _PACKED + ("nnz_per_offset", "zmask"):
            self.register_buffer("_ws_" + name, None, persistent=False)
        self._flops = None

    def sparsify(self, layout="csr"):
        """Fix the kernel's zero pattern for inference (reference :346-379).  "csr" and "coo" select the sparse kernel (on a
        GPU the distinction is a torch storage detail), "strided" the dense function on the masked weights.  Idempotent."""
        if layout not in LAYOUTS:
            raise ValueError(f"sparsify(layout={layout!r}): one of {LAYOUTS}")
        self.layout = layout
        if self.use_mm:  # a plain matrix product stays one (reference :347)
            return
        if self.kernel.shape[0] > 27:
            raise ValueError(f"sparsify: the weight-sparse kernel holds 27 offsets at most; this kernel has {self.kernel.shape[0]} "
                             "(kernel sizes 5 and 7 run dense, through ME.MinkowskiConvolution)")
        with torch.no_grad():
            w = self.kernel.detach()
            if self.sparse_mode is SparseConvMode.ZAXIS:
                if w.shape[0] != 27:
                    raise ValueError(f"SparseConvMode.ZAXIS keeps offsets {ZAXIS_OFFSETS} of a 3x3x3 kernel; this kernel has "
                                     f"{w.shape[0]} offsets")
                zmask = torch.zeros(27, 1, 1, dtype=w.dtype, device=w.device)
                zmask[ZAXIS_OFFSETS] = 1
                self._ws_zmask = zmask
                w = w * zmask
            p = wsconv.pack_csr(w)
            for name in _PACKED:
                setattr(self, "_ws_" + name, getattr(p, name))
            self._ws_nnz_per_offset = (w != 0).reshape(w.shape[0], -1).sum(1)
            self.nnz, self.density, self._koff_list = p.nnz, p.density, p.valid_kernel
            self.valid_kernel = list(ZAXIS_OFFSETS) if self.sparse_mode is SparseConvMode.ZAXIS else list(p.valid_kernel)

    def _packed(self):
        K, cin, cout = self.kernel.shape
        return wsconv.Packed(self._ws_koffs, self._ws_rowptr, self._ws_colidx, self._ws_vals, self._ws_cptr, self.nnz,
                             self.density, self._koff_list, K, cin, cout)

    def _use_sparse(self):
        if self.layout == "strided" or self.path == "dense":
            return False
        return self.path == "sparse" or self.density <= wsconv.MAX_DENSITY

    def _masked_kernel(self):
        return self.kernel if self._ws_zmask is None else self.kernel * self._ws_zmask

    @staticmethod
    def _pairs(m, nbr):
        """int64 [K]: the pairs of every offset of a table, counted once per table: the manager that owns the table keeps the
        count, so the layers of a level share it."""
        cache = m.__dict__.setdefault("_ws_pair_counts", {})
        hit = cache.get(nbr.data_ptr())
        if hit is None or hit[0] is not nbr:
            hit = cache[nbr.data_ptr()] = (nbr, (nbr >= 0).sum(0))
        return hit[1]

    def _count(self, m, nbr, rows):
        """The reference's operation count (:38,53,395,419), a 0-dim int64 tensor on the device (no host synchronisation):
        per valid offset the stored weights (all cin * cout of them under "strided") times the offset's pairs, plus the bias."""
        pairs = self._pairs(m, nbr)
        if self.layout == "strided":
            K, cin, cout = self.kernel.shape
            per = (self._ws_nnz_per_offset > 0).to(torch.int64) * (cin * cout)
        else:
            per = self._ws_nnz_per_offset
        ops = (pairs * per).sum()
        if self.bias is not None:
            ops = ops + self.bias.numel() * rows
        return ops

    def _forward_mm(self, input):
        out = input.F.mm(self.kernel)
        ops = out.numel() * input.F.shape[1]
        if self.bias is not None:
            out = out + self.bias
            ops += self.bias.numel() * out.shape[0]
        self._flops = torch.full((), ops, dtype=torch.int64, device=out.device)  # (a fill, not a copy from the host: no synchronisation)
        return SparseTensor(out, input.coordinate_map_key, input.coordinate_manager)

    def _run(self, input, nbr, out_key, dense_fn):
        m = input.coordinate_manager
        n_out = nbr.shape[0]
        if self._use_sparse():
            out = wsconv.wsconv_forward(input.F, self._packed(), nbr, n_out, self.bias)
        else:
            with torch.no_grad():
                out = dense_fn(self._masked_kernel())
                if self.bias is not None:
                    out = out + self.bias
        self._flops = self._count(m, nbr, n_out)
        return SparseTensor(out, out_key, m)

    def extra_repr(self):
        s = super().extra_repr() + f", sparse_mode={self.sparse_mode.name}"
        if self.layout is not None and not self.use_mm:
            s += f", layout={self.layout}, density={self.density:.4f}"
        return s


class WeightSparseConvolution(_WeightSparse, MinkowskiConvolution):
    """Reference sparse_conv.py:455-516.  kernel (K, Cin, Cout), or (Cin, Cout) for `use_mm`; bias (1, Cout)."""

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 expand_coordinates=False, convolution_mode=None, dimension=None, sparse_mode=1):
        MinkowskiConvolution.__init__(self, in_channels, out_channels, kernel_size, stride, dilation, bias, kernel_generator,
                                      expand_coordinates, convolution_mode, dimension)
        self._init_sparse(sparse_mode)

    def forward(self, input, coordinates=None, bn_stats=False):
        """`bn_stats` is accepted and ignored (the fused units and blocks pass it): inference has no batch statistics."""
        assert coordinates is None, "explicit output coordinates are out of scope"
        if self.use_mm:
            return self._forward_mm(input)
        if self.layout is None:
            raise RuntimeError("WeightSparseConvolution.forward before sparsify(): the layer has no packed kernel")
        m, in_key = input.coordinate_manager, input.coordinate_map_key
        out_key = m.stride(in_key, self.stride)
        ks, dil = self.kernel_size, self.dilation
        nbr, _ = m.kernel_table(in_key, out_key, ks, dil)

        def dense_fn(w):
            return Fn.ConvolutionFunction.apply(input.F, w, lambda transposed: (nbr, None, None), False, None)

        return self._run(input, nbr, out_key, dense_fn)


class WeightSparseConvolutionTranspose(_WeightSparse, MinkowskiConvolutionTranspose):
    """Reference sparse_conv.py:519-559: up-samples onto the coordinate map that exists at tensor stride ts / stride, through
    the tables MinkowskiConvolutionTranspose.forward takes from the manager (the transposed table of the convolution fine ->
    coarse); lanes are output rows, so the parity-class row permutation of the dense kernel is not needed."""

    def __init__(self, in_channels, out_channels, kernel_size=-1, stride=1, dilation=1, bias=False, kernel_generator=None,
                 expand_coordinates=False, convolution_mode=None, dimension=None, sparse_mode=1):
        MinkowskiConvolutionTranspose.__init__(self, in_channels, out_channels, kernel_size, stride, dilation, bias,
                                               kernel_generator, expand_coordinates, convolution_mode, dimension)
        self._init_sparse(sparse_mode)

    def forward(self, input, coordinates=None, bn_stats=False):
        assert coordinates is None, "explicit output coordinates are out of scope"
        if self.layout is None:
            raise RuntimeError("WeightSparseConvolutionTranspose.forward before sparsify(): the layer has no packed kernel")
        m, in_key = input.coordinate_manager, input.coordinate_map_key
        ts = in_key.get_tensor_stride()[0]
        if ts % self.stride or not m.has_level(ts // self.stride):
            raise RuntimeError(f"WeightSparseConvolutionTranspose: no coordinate map at tensor stride {ts // self.stride} to "
                               "up-sample onto (generative up-sampling is out of scope)")
        out_key = CoordinateMapKey(ts // self.stride)
        ks, dil = self.kernel_size, self.dilation
        nbr, nbr_t = m.kernel_table(out_key, in_key, ks, dil, transposed=True)

        def dense_fn(w):
            return Fn.ConvolutionFunction.apply(input.F, w, lambda transposed: (nbr_t, nbr, m.class_perm(out_key)), False, None)

        return self._run(input, nbr_t, out_key, dense_fn)
