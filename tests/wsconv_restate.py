"""Float64 restatement of the weight-sparse convolution (include/mink_hip.h, mink_wsconv_fwd), written from its definition:

    y[r][co] = bias[co] + sum over the valid offsets k, ascending, with i = nbr[r][k] >= 0,
                          of sum over the nonzeros (ci, co, v) of W[k]:  x[i][ci] * v

as a loop over the valid offsets doing gather, masked matmul, index-add.  Beside y it returns, per output element, T = the number
of products summed (+1 with a bias) and S = sum |x * v| (+ |bias|): the operands of the textbook bound for an fp32 fma / add
chain of T terms in any order, |y32 - y64| <= gamma_T S with gamma_T = T u / (1 - T u), u = 2^-24."""
import torch

U = 2.0 ** -24


def restate(x, kernel, nbr, n_out, bias=None, valid=None):
    """x [n_in, cin], kernel [K, cin, cout] (its zeros are the pruned weights), nbr [n_out, K] -> (y, T, S), all float64 /
    int64 [n_out, cout] on the CPU.  `valid`: the offsets to visit (default: those that hold a nonzero)."""
    x64 = x.detach().double().cpu()
    w64 = kernel.detach().double().cpu()
    nbr = nbr.detach().cpu().long()
    K, cin, cout = w64.shape
    mask = (w64 != 0).double()
    if valid is None:
        valid = [k for k in range(K) if bool(mask[k].any())]
    y = torch.zeros(n_out, cout, dtype=torch.float64)
    S = torch.zeros(n_out, cout, dtype=torch.float64)
    T = torch.zeros(n_out, cout, dtype=torch.int64)
    # a NaN / Inf of x only reaches y through a stored weight: products with a pruned weight are not formed (not 0 * NaN)
    finite_x = torch.nan_to_num(x64, nan=0.0, posinf=0.0, neginf=0.0)
    bad_x = (~torch.isfinite(x64)).double()
    poisoned = torch.zeros(n_out, cout, dtype=torch.bool)
    for k in valid:
        rows = torch.nonzero(nbr[:, k] >= 0).reshape(-1)
        if rows.numel() == 0:
            continue
        src = nbr[rows, k]
        g = finite_x[src]
        y.index_add_(0, rows, g @ (w64[k] * mask[k]))
        S.index_add_(0, rows, g.abs() @ (w64[k] * mask[k]).abs())
        T.index_add_(0, rows, mask[k].sum(0).long().expand(rows.numel(), cout).contiguous())
        hit = (bad_x[src] @ mask[k]) > 0
        poisoned[rows] |= hit
    if bias is not None:
        b = bias.detach().double().cpu().reshape(1, cout)
        y, S, T = y + b, S + b.abs(), T + 1
    y[poisoned] = float("nan")
    return y, T, S


def bound(T, S):
    """gamma_T S per element."""
    tu = T.double() * U
    return tu / (1 - tu) * S


def dense_masked_conv(x, kernel, nbr, n_out, bias=None):
    """The ordinary convolution with the (masked) kernel in float64: every offset, zero weights multiplied like any other."""
    x64, w64, nbr = x.detach().double().cpu(), kernel.detach().double().cpu(), nbr.detach().cpu().long()
    y = torch.zeros(n_out, w64.shape[2], dtype=torch.float64)
    for k in range(w64.shape[0]):
        rows = torch.nonzero(nbr[:, k] >= 0).reshape(-1)
        y.index_add_(0, rows, x64[nbr[rows, k]] @ w64[k])
    return y if bias is None else y + bias.detach().double().cpu().reshape(1, -1)


def random_table(n_out, K, n_in, p_missing=0.4, seed=0):
    """int32 [n_out, K]: entries uniform in [0, n_in), -1 with probability `p_missing`."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, max(n_in, 1), (n_out, K), generator=g, dtype=torch.int32)
    t[torch.rand(n_out, K, generator=g) < p_missing] = -1
    return t


def random_kernel(K, cin, cout, density, seed=0, integer=False):
    """[K, cin, cout] with about `density` of its weights kept (exactly one nonzero for density "one", none for 0)."""
    g = torch.Generator().manual_seed(seed + 1000)
    w = torch.randint(-3, 4, (K, cin, cout), generator=g).float() if integer else torch.randn(K, cin, cout, generator=g)
    if density == "one":
        z = torch.zeros_like(w)
        z[K // 2, cin - 1, cout // 2] = 2.0 if integer else 0.37
        return z
    if density >= 1.0:
        return w if not integer else torch.where(w == 0, torch.ones_like(w), w)
    if density <= 0.0:
        return torch.zeros_like(w)
    return w * (torch.rand(K, cin, cout, generator=g) < density)
