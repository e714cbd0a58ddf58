"""float64 numpy restatement of the sparse convolution with 5^3 / 7^3 kernels (csrc/conv_bigk.hip), written from the definition
and independent of the backend: forward, data gradient and weight gradient from a neighbour table nbr[n_out, K] (input row or -1),
offset by offset, absent pairs SKIPPED (so a NaN only travels through pairs the table names).

Every function returns (value, T, S) per output element: T = the number of products that enter it, S = the sum of their absolute
values.  The bound the GPU results are held to,

    |err| <= 2 (T + 2) 2^-24 S                                                                                       (bound())

is the worst case of a T-term fp32 sum in any order, about T 2^-24 S (one rounding per product, one per addition), with a factor
2 for the few extra roundings of slice and split reductions and of the bias.  It is derived, not measured."""
import numpy as np

EPS = 2.0 ** -24


def _np64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, "detach") else t, dtype=np.float64)


def _tab(nbr):
    return np.asarray(nbr.detach().cpu().numpy() if hasattr(nbr, "detach") else nbr, dtype=np.int64)


def forward(x, w, nbr, bias=None):
    """y[o] = sum_k x[nbr[o, k]] @ w[k] (+ bias) -> (y, T, S), each [n_out, cout]."""
    x, w, nbr = _np64(x), _np64(w), _tab(nbr)
    n, K = nbr.shape
    cin, cout = w.shape[1], w.shape[2]
    y, S = np.zeros((n, cout)), np.zeros((n, cout))
    for k in range(K):
        o = np.nonzero(nbr[:, k] >= 0)[0]
        if o.size:
            g = x[nbr[o, k], :cin]
            y[o] += g @ w[k]
            S[o] += np.abs(g) @ np.abs(w[k])
    T = np.repeat(((nbr >= 0).sum(1) * cin)[:, None], cout, 1).astype(np.float64)
    if bias is not None:
        b = _np64(bias).reshape(1, cout)
        y, S, T = y + b, S + np.abs(b), T + 1
    return y, T, S


def dgrad(dy, w, nbr, n_in):
    """dx[i] = sum over the pairs (o, k) with nbr[o, k] = i of dy[o] @ w[k]^T -> (dx, T, S), each [n_in, cin]."""
    dy, w, nbr = _np64(dy), _np64(w), _tab(nbr)
    K, cin, cout = w.shape
    dx, S, cnt = np.zeros((n_in, cin)), np.zeros((n_in, cin)), np.zeros(n_in)
    for k in range(K):
        o = np.nonzero(nbr[:, k] >= 0)[0]
        if o.size:
            i = nbr[o, k]  # (an input row has one output per offset: no repeated index)
            dx[i] += dy[o, :cout] @ w[k].T
            S[i] += np.abs(dy[o, :cout]) @ np.abs(w[k]).T
            cnt[i] += 1
    return dx, np.repeat((cnt * cout)[:, None], cin, 1), S


def wgrad(x, dy, nbr, cin=None, cout=None):
    """dW[k] = x[nbr[:, k]]^T @ dy over the rows that have offset k -> (dW, T, S), each [K, cin, cout]."""
    x, dy, nbr = _np64(x), _np64(dy), _tab(nbr)
    cin, cout = cin or x.shape[1], cout or dy.shape[1]
    K = nbr.shape[1]
    dw, S, T = np.zeros((K, cin, cout)), np.zeros((K, cin, cout)), np.zeros((K, cin, cout))
    for k in range(K):
        o = np.nonzero(nbr[:, k] >= 0)[0]
        if o.size:
            g = x[nbr[o, k], :cin]
            dw[k] = g.T @ dy[o, :cout]
            S[k] = np.abs(g).T @ np.abs(dy[o, :cout])
            T[k] = o.size
    return dw, T, S


def bound(T, S):
    return 2.0 * (T + 2.0) * EPS * S


def worst_ratio(got, ref, T, S):
    """max over the elements of |got - ref| / bound (0 / 0 counts as 0: an element no product enters must be exactly the reference's)."""
    got = _np64(got)
    err, b = np.abs(got - ref), bound(T, S)
    if err.size == 0:
        return 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(b > 0, err / b, np.where(err == 0, 0.0, np.inf))
    return float(r.max())
