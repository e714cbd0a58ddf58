"""Weight-sparse convolution of the HIP backend: the operator behind WeightSparseConvolution(Transpose) (reference
co3d_3d/src/models/mink/modules/sparse_conv.py:57-152: one `spmm` per kernel offset over the CSR of W[k]^T).

    pack_csr(kernel)                      once, at sparsify(): the CSR the reference's sparsify("csr") keeps, concatenated over
                                          the offsets that hold a nonzero, plus the per-chunk row pointers the kernel walks
    wsconv_forward(x, packed, nbr, n_out) one launch of mink_wsconv_fwd (csrc/wsconv.hip); inference only, never requires grad

`MAX_DENSITY` is the density up to which a sparsified layer takes the sparse kernel; above it the layer runs the dense
gather-GEMM on its masked weights (profiles/wsconv_kernels.txt, DESIGN.md "Weight-sparse convolution")."""
from collections import namedtuple

import torch

from .._lib import WSCONV_CHUNK, check, lib
from ._rt import _f32c, _ptr, _stream

# The largest tested density at which mink_wsconv_fwd beat mink_conv_gather_gemm on EVERY timed shape (profiles/wsconv_kernels.txt).
MAX_DENSITY = 0.0

Packed = namedtuple("Packed", "koffs rowptr colidx vals cptr nnz density valid_kernel K cin cout")


def pack_csr(kernel, chunk=WSCONV_CHUNK):
    """kernel [K, cin, cout] -> Packed, on the kernel's device.

    koffs [n_valid] int32: the offsets with a nonzero, ascending (= valid_kernel, a Python list);
    rowptr [n_valid, cout + 1] int32, colidx [nnz] int32, vals [nnz] float32: CSR of W[k]^T per valid offset (rows = output
    channels, columns = input channels ascending), rowptr indexing the concatenated colidx / vals;
    cptr [n_valid, cout, nchunks + 1] int32: the first nonzero of a row at or behind column j * chunk (derived; the kernel
    stages `chunk` input channels at a time); nnz, density = nnz / kernel.numel()."""
    assert kernel.dim() == 3, "pack_csr takes a [K, cin, cout] kernel"
    with torch.no_grad():
        w = kernel.detach().float()
        K, cin, cout = w.shape
        dev = w.device
        wt = w.transpose(1, 2)  # [K, cout, cin]: rows of W[k]^T
        nz = wt != 0
        per_offset = nz.reshape(K, -1).sum(1)
        valid = torch.nonzero(per_offset > 0).reshape(-1)
        valid_kernel = [int(k) for k in valid.tolist()]
        nv = len(valid_kernel)
        nzv = nz[valid]  # [nv, cout, cin]
        # row-major nonzero order of [nv, cout, cin] = offsets ascending, rows ascending, columns ascending
        idx = torch.nonzero(nzv.reshape(-1)).reshape(-1)
        colidx = (idx % cin).to(torch.int32)
        vals = wt[valid].reshape(-1)[idx].contiguous()
        nnz = int(idx.numel())
        nchunks = -(-cin // chunk)
        # nonzeros of a row in front of every chunk boundary
        edges = [min(j * chunk, cin) for j in range(nchunks + 1)]
        cum = torch.zeros(nv, cout, cin + 1, dtype=torch.int64, device=dev)
        if nv:
            cum[:, :, 1:] = nzv.to(torch.int64).cumsum(2)
        counts = cum[:, :, cin].reshape(-1)  # nonzeros per (offset, row)
        start = torch.zeros(nv * cout + 1, dtype=torch.int64, device=dev)
        if nv:
            start[1:] = counts.cumsum(0)
        rowptr = torch.empty(nv, cout + 1, dtype=torch.int64, device=dev)
        if nv:
            rowptr[:, :cout] = start[:-1].reshape(nv, cout)
            rowptr[:, cout] = start[cout::cout]
        cptr = start[:-1].reshape(nv, cout, 1) + cum[:, :, edges]
        assert nnz < 2 ** 31
        return Packed(valid.to(torch.int32), rowptr.to(torch.int32).contiguous(), colidx.contiguous(), vals,
                      cptr.to(torch.int32).contiguous(), nnz, nnz / max(w.numel(), 1), valid_kernel, K, cin, cout)


def densify(packed):
    """The [K, cin, cout] kernel a Packed holds (tests; the inverse of pack_csr)."""
    w = torch.zeros(packed.K, packed.cout, packed.cin, dtype=packed.vals.dtype, device=packed.vals.device)
    rp = packed.rowptr.long()
    for v, k in enumerate(packed.valid_kernel):
        for co in range(packed.cout):
            a, b = int(rp[v, co]), int(rp[v, co + 1])
            w[k, co, packed.colidx[a:b].long()] = packed.vals[a:b]
    return w.transpose(1, 2).contiguous()


def wsconv_forward(x, packed, nbr, n_out, bias=None):
    """y [n_out, cout] = the weight-sparse convolution of x [n_in, cin] through the neighbour table nbr [n_out, K] (int32, -1 =
    no neighbour; a transposed convolution passes its transposed table).  Runs under no_grad; the result never requires grad."""
    with torch.no_grad():
        x = _f32c(x.detach())
        assert x.dim() == 2 and x.shape[1] == packed.cin, (tuple(x.shape), packed.cin)
        assert nbr.dtype == torch.int32 and nbr.dim() == 2 and nbr.shape[0] == n_out and nbr.shape[1] == packed.K, \
            (tuple(nbr.shape), n_out, packed.K)
        nbr = nbr.contiguous()
        if bias is not None:
            bias = _f32c(bias.detach()).reshape(-1)
            assert bias.numel() == packed.cout
        y = torch.empty(n_out, packed.cout, dtype=torch.float32, device=x.device)
        check(lib().mink_wsconv_fwd(
            x.data_ptr(), x.shape[0], x.stride(0) if x.shape[0] else packed.cin, packed.cin, nbr.data_ptr(), n_out, packed.K,
            packed.koffs.data_ptr(), len(packed.valid_kernel), packed.rowptr.data_ptr(), packed.cptr.data_ptr(),
            packed.colidx.data_ptr(), packed.vals.data_ptr(), packed.nnz, y.data_ptr(), packed.cout, packed.cout, _ptr(bias),
            _stream()))
        return y
