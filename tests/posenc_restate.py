"""Float64 restatement of MinkowskiPositionalEncoding, written from the formulas (not from the kernel, not from the module):

    Q = 2 L C;  column q reads channel q // (2L) with frequency f[q mod L] and phase 0 (q < C L) or pi / 2 (q >= C L)
    y[:, q] = sin(f[q mod L] * x[:, q // (2L)] + phase[q]);   then x[:, lo:hi] behind the Q columns
    dx[:, c] = sum over q in channel c of f_q cos(f_q x_c + phase_q) dy[:, q]   (+ dy of the pass-through column of c)

The loops are explicit on purpose; tests/test_posenc_cpu.py holds them to a dense-matrix form under torch autograd."""
import math

import torch

EPS = 2.0 ** -23  # one ulp of a float in [1, 2)


def base_frequencies(L, min_resolution=None):
    """float64 [L]: 2^j, or 2 ** linspace(m - L - 1, m, L) with m = log2(0.5 / min_resolution) -- L + 1 octaves in L steps."""
    if min_resolution is None:
        return torch.tensor([2.0 ** j for j in range(L)], dtype=torch.float64)
    m = math.log2(0.5 / min_resolution)
    if L == 1:
        return torch.tensor([2.0 ** (m - L - 1)], dtype=torch.float64)
    return torch.tensor([2.0 ** (m - L - 1 + j * (L + 1) / (L - 1)) for j in range(L)], dtype=torch.float64)


def columns(C, L, min_resolution=None):
    """(channel int64 [Q], freq float64 [Q], phase float64 [Q]) of the Q = 2 L C encoded columns."""
    f = base_frequencies(L, min_resolution)
    Q = 2 * L * C
    chan = torch.tensor([q // (2 * L) for q in range(Q)], dtype=torch.int64)
    freq = torch.stack([f[q % L] for q in range(Q)]) if Q else torch.zeros(0, dtype=torch.float64)
    phase = torch.tensor([0.0 if q < C * L else math.pi / 2 for q in range(Q)], dtype=torch.float64)
    return chan, freq, phase


def argument(x, chan, freq, phase):
    """a[:, q] = freq[q] * x[:, chan[q]] + phase[q] in float64, from whatever precision the operands were given in."""
    return freq.double()[None, :] * x.double()[:, chan] + phase.double()[None, :]


def forward(x, chan, freq, phase, rng=None):
    """-> y float64 [n, Q + hi - lo].  `freq`, `phase`: the layer's constants (fp32 values are taken as they are)."""
    lo, hi = rng or (0, 0)
    return torch.cat([torch.sin(argument(x, chan, freq, phase)), x.double()[:, lo:hi]], dim=1)


def backward(x, dy, chan, freq, phase, rng=None):
    """-> dx float64 [n, C]"""
    lo, hi = rng or (0, 0)
    n, C = x.shape
    Q = chan.numel()
    a, dy = argument(x, chan, freq, phase), dy.double()
    dx = torch.zeros(n, C, dtype=torch.float64)
    for q in range(Q):
        dx[:, int(chan[q])] += freq[q].double() * torch.cos(a[:, q]) * dy[:, q]
    for c in range(lo, hi):
        dx[:, c] += dy[:, Q + c - lo]
    return dx


def forward_bound(x, chan, freq, phase):
    """(|a| + 4) 2^-23 per encoded column: one fp32 rounding of the argument (fused or not) moves it by at most |a| 2^-24 ... 2^-23
    and the sine has slope at most 1; a few ulps of a result of at most 1 are the constant."""
    return (argument(x, chan, freq, phase).abs() + 4) * EPS


def backward_bound(x, dy, chan, freq, phase, ref):
    """2^-22 sum_q f_q |dy_q| (|a_q| + 4) + 4 ulps of |ref| per element of dx."""
    n, C = x.shape
    a = argument(x, chan, freq, phase)
    term = freq.double()[None, :] * dy.double()[:, : chan.numel()].abs() * (a.abs() + 4)
    s = torch.zeros(n, C, dtype=torch.float64)
    s.index_add_(1, chan, term)
    return 2 * EPS * s + 4 * EPS * ref.abs()


def inputs(n, C, seed, big_column=True):
    """Normal inputs with sd 1.5; the last column scaled to |x| ~ 100."""
    g = torch.Generator().manual_seed(seed)
    x = 1.5 * torch.randn(n, C, generator=g)
    if big_column and n:
        x[:, C - 1] *= 100 / 1.5
    return x
