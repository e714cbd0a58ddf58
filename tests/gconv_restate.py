"""Grouped convolution over a neighbour table (csrc/gconv.hip), restated in float64 with plain torch indexing, and the bounds a
float32 run of it has to meet.

    rows  x [n_in, G ci], y and dy [n_out, G co]: group g owns the input columns g ci .. and the output columns g co ..
    table nbr [n_out, K], -1 = outside: such an entry contributes nothing and is not multiplied
    w     [K, G, ci, co], the packed layout (and the layout of dw)

    forward          y[r, g, o]          = sum_k sum_c x[nbr[r, k], g, c] w[k, g, c, o]
    data gradient    dx[nbr[r, k], g, c] += sum_o dy[r, g, o] w[k, g, c, o]      (a scatter through the FORWARD table: the kernel
                                                                                  gathers through the transposed or flipped one)
    weight gradient  dw[k, g, c, o]      = sum_r x[nbr[r, k], g, c] dy[r, g, o]

`bounds()`: for each output element S is the float64 sum of the absolute values of its products, u = 2^-24, and the bound is
1.01 n u S + 1e-37 with n the LONGEST sum an element can have -- K ci (forward), K co (data gradient), the number of table rows
(weight gradient).  An fp32 FMA chain of m <= n products errs by at most gamma_m S <= 1.01 m u S (Higham, Accuracy and
Stability, section 3.1; m u < 0.01 here), in any order of the terms, and a sum split into partial sums that are then added stays
inside the same figure (each product passes through at most m - 1 additions either way).  Derived, not measured."""
import math

import torch

U = 2.0 ** -24


def pack(weight, groups):
    """torch's [G co, ci, kh, kw] -> the packed [kh kw, G, ci, co]."""
    GO, ci, kh, kw = weight.shape
    co = GO // groups
    return weight.reshape(groups, co, ci, kh, kw).permute(3, 4, 0, 2, 1).reshape(kh * kw, groups, ci, co)


def unpack(w, k):
    """the packed [k k, G, ci, co] -> torch's [G co, ci, k, k]."""
    K, G, ci, co = w.shape
    return w.reshape(k, k, G, ci, co).permute(2, 4, 3, 0, 1).reshape(G * co, ci, k, k)


def forward(x, w, nbr, absolute=False):
    K, G, ci, co = w.shape
    x, w = x.double(), w.double()
    if absolute:
        x, w = x.abs(), w.abs()
    y = torch.zeros(nbr.shape[0], G, co, dtype=torch.float64)
    for k in range(K):
        idx = nbr[:, k].long()
        v = idx >= 0
        y[v] += torch.einsum("rgc,gco->rgo", x[idx[v]].reshape(-1, G, ci), w[k])
    return y.reshape(nbr.shape[0], G * co)


def data_gradient(dy, w, nbr, n_in, absolute=False):
    K, G, ci, co = w.shape
    dy, w = dy.double(), w.double()
    if absolute:
        dy, w = dy.abs(), w.abs()
    dx = torch.zeros(n_in, G, ci, dtype=torch.float64)
    for k in range(K):
        idx = nbr[:, k].long()
        v = idx >= 0
        dx.index_add_(0, idx[v], torch.einsum("rgo,gco->rgc", dy[v].reshape(-1, G, co), w[k]))
    return dx.reshape(n_in, G * ci)


def weight_gradient(x, dy, nbr, K, G, ci, co, absolute=False):
    x, dy = x.double(), dy.double()
    if absolute:
        x, dy = x.abs(), dy.abs()
    dw = torch.zeros(K, G, ci, co, dtype=torch.float64)
    for k in range(K):
        idx = nbr[:, k].long()
        v = idx >= 0
        dw[k] = torch.einsum("rgc,rgo->gco", x[idx[v]].reshape(-1, G, ci), dy[v].reshape(-1, G, co))
    return dw


def bounds(x, w, dy, nbr):
    """{"y", "dx", "dw"}: the float64 bound of every element (module docstring)."""
    K, G, ci, co = w.shape
    f = 1.01 * U
    return {"y": f * K * ci * forward(x, w, nbr, absolute=True) + 1e-37,
            "dx": f * K * co * data_gradient(dy, w, nbr, x.shape[0], absolute=True) + 1e-37,
            "dw": f * max(int(nbr.shape[0]), 1) * weight_gradient(x, dy, nbr, K, G, ci, co, absolute=True) + 1e-37}


def reference(x, w, dy, nbr):
    K, G, ci, co = w.shape
    return {"y": forward(x, w, nbr), "dx": data_gradient(dy, w, nbr, x.shape[0]), "dw": weight_gradient(x, dy, nbr, K, G, ci, co)}


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound; inf when a value is not finite or an error stands against a zero bound."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def inputs(n_in, n_out, K, G, ci, co, seed, offset=0.0):
    """fp32 (x [n_in, G ci], w [K, G, ci, co], dy [n_out, G co]) from a seeded normal; `offset` is added to x."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_in, G * ci, generator=g) + offset
    w = torch.randn(K, G, ci, co, generator=g) / math.sqrt(K * ci)
    dy = torch.randn(n_out, G * co, generator=g)
    return x, w, dy
