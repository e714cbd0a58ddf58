"""float64 restatement of the dynamic graph layers (csrc/graph.hip, nerf_downstream_amd/minkowski/graph.py) and of DGCNN_cls,
written from the algorithm (Wang et al., Dynamic Graph CNN: EdgeConv with the asymmetric edge function h(x_i, x_j - x_i)) and
independent of the backend: direct squared distances and a stable sort find the neighbours, the edge convolution is the plain
[n, k, 2 Cin] @ W^T, torch float64 autograd differentiates.  Nothing here calls the code under test.

kNN.  Row i's neighbours are the k rows j of its own sample with the smallest sum_c (x_i[c] - x_j[c])^2, itself included, in
ascending distance, equal distances in ascending row order (a stable sort of the distances of rows s0 .. s1 - 1).

Edge convolution.  e[i][j] = W [x_idx[i][j] - x_i ; x_i]; batch norm over the n k edges per channel (biased variance, eps
1e-5; or given statistics, eval mode); LeakyReLU(0.2); y[i] = the maximum over j, arg = the lowest j attaining it.

Error bounds.  The fp32 bounds the GPU tests assert are running-error bounds: every quantity the kernels form is a sum of
products, and |fl(sum a b) - sum a b| <= L u sum |a b| to first order, L the number of roundings on the longest path and
u = 2^-24 -- the 'absolute-value sums' of `edge_bounds`; an error a factor already carries goes through a product times the
absolute value of the other factor.  The one non-polynomial step, invstd = (var + eps)^-1/2, carries the relative error of
var through: |d var| / (2 (var + eps))."""
import torch

F64 = torch.float64
U32 = 2.0 ** -24  # unit roundoff of fp32
BN_EPS = 1e-5
SLOPE = 0.2


# ------------------------------------------------------------------------------------------------ kNN
def sq_dists(x, lo, hi):
    """float64 [hi - lo, hi - lo] squared distances inside rows lo .. hi - 1, by direct differences."""
    s = x[lo:hi].to(F64)
    return ((s[:, None, :] - s[None, :, :]) ** 2).sum(-1)


def knn(x, off, k):
    """idx int64 [n, k] of global rows; `off` = the B + 1 row offsets of the samples (an empty sample is skipped, a sample
    of fewer than k rows is an error)."""
    out = torch.empty(x.shape[0], k, dtype=torch.int64)
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        if hi == lo:
            continue
        if hi - lo < k:
            raise ValueError(f"sample {b} holds only {hi - lo} points")
        out[lo:hi] = torch.sort(sq_dists(x, lo, hi), dim=1, stable=True).indices[:, :k] + lo
    return out


def knn_tau(x, lo, hi):
    """tau [hi - lo] of the validity check for the expanded form  s_ij = ||x_j||^2 - 2 x_i . x_j  in fp32 (see
    tests/test_gpu_dgcnn.py::test_knn_validity_on_normal_data for the derivation): 2 (C + 2) u (||x_i|| + max_j ||x_j||)^2."""
    nrm = x[lo:hi].to(F64).norm(dim=1)
    return 2.0 * (x.shape[1] + 2) * U32 * (nrm + nrm.max()) ** 2


def knn_violations(x, off, idx, k):
    """The validity of a neighbour table against the float64 distances of x: -> (rows with an index outside their sample, rows
    with a repeated index, the largest (d64 - d_(k) - tau_i) over the chosen, the largest (d_(k) - tau_i - d64) over the
    unchosen); the table is valid when the first two are 0 and the last two <= 0."""
    idx = idx.long()
    outside = repeated = 0
    worst_in = worst_out = -float("inf")
    for b in range(len(off) - 1):
        lo, hi = off[b], off[b + 1]
        if hi == lo:
            continue
        d = sq_dists(x, lo, hi)
        tau = knn_tau(x, lo, hi)
        dk = torch.sort(d, dim=1).values[:, k - 1]
        loc = idx[lo:hi] - lo
        bad = ((loc < 0) | (loc >= hi - lo)).any(1)
        outside += int(bad.sum())
        loc = loc.clamp(0, hi - lo - 1)
        repeated += int((torch.sort(loc, dim=1).values.diff(dim=1) == 0).any(1).sum())
        chosen = torch.zeros_like(d, dtype=torch.bool).scatter_(1, loc, True)
        over = d - (dk + tau)[:, None]
        under = (dk - tau)[:, None] - d
        worst_in = max(worst_in, float(over[chosen].max()))
        if bool((~chosen).any()):
            worst_out = max(worst_out, float(under[~chosen].max()))
    return outside, repeated, worst_in, worst_out


def knn_valid(x, off, idx, k):
    outside, repeated, worst_in, worst_out = knn_violations(x, off, idx, k)
    return outside == 0 and repeated == 0 and worst_in <= 0 and worst_out <= 0


# ------------------------------------------------------------------------------------------------ edge convolution
def lrelu(z):
    return torch.where(z > 0, z, SLOPE * z)


def edges(x, W, idx):
    """e float64 [n, k, Cout] = [x_j - x_i ; x_i] @ W^T, the plain way."""
    xi = x[:, None, :].expand(-1, idx.shape[1], -1)
    return torch.cat([x[idx] - xi, xi], -1) @ W.reshape(W.shape[0], -1).t()


def first_argmax(z):
    """The lowest slot attaining the maximum over dim 1 of z [n, k, C] -> int64 [n, C]."""
    top = z.max(1, keepdim=True).values  # (a NaN is the maximum, the first one the arg: torch's rule)
    hit = (z == top) | (torch.isnan(z) & torch.isnan(top))
    k = z.shape[1]
    slots = torch.arange(k).reshape(1, k, 1).expand_as(z)
    return torch.where(hit, slots, torch.full_like(slots, k)).min(1).values


def edge_conv(x, W, gamma, beta, idx, stats=None, eps=BN_EPS):
    """-> (y [n, Cout], arg int64 [n, Cout], (mean, biased var) used).  `stats` = (mean, var): eval mode."""
    e = edges(x, W, idx)
    if stats is None:
        flat = e.reshape(-1, e.shape[-1])
        mean = flat.mean(0)
        var = ((flat - mean) ** 2).mean(0)
    else:
        mean, var = stats
    z = (e - mean) / torch.sqrt(var + eps) * gamma + beta
    arg = first_argmax(z.detach())
    y = lrelu(z.gather(1, arg[:, None, :])[:, 0, :])
    return y, arg, (mean, var)


def running_update(running_mean, running_var, mean, var, count, momentum=0.1):
    """torch's update: the batch mean and the UNBIASED batch variance (count / (count - 1))."""
    return ((1 - momentum) * running_mean + momentum * mean, (1 - momentum) * running_var + momentum * var * count / (count - 1))


def edge_bounds(x, W, gamma, beta, idx, dy, stats=None, eps=BN_EPS):
    """First-order fp32 bounds for y, dx, dW, dgamma, dbeta (and the batch mean / var) of one edge layer evaluated as
    e = P[idx] + Q[i], P = X W1^T, Q = X (W2 - W1)^T, by the rule of the module docstring: a sum of L rounded products is off
    by at most L u times the sum of their absolute values; an error already present in a factor is carried through times the
    absolute value of the other factor.  All float64, no gradient; the arg slots and the LeakyReLU decisions are the
    restatement's (the tests assert the former).
      e        : Cin products, the rounding of W2 - W1, the add: L_e = Cin + 2 on A_e = |x_j| |W1| + |x_i| (|W2| + |W1|)
      mean, var: double sums of the fp32 e's, so they inherit e's error: d mean <= (L_e + 1) u A_mu, A_mu = mean A_e;
                 d var <= 2 (L_e + 2) u A_var, A_var = mean |e - mu| (A_e + A_mu); r = d var / (2 (var + eps)) + 2 u is the
                 relative error of invstd (eval mode: r = 4 u, the add, the rsqrt and the conversions)
      xhat     : (e - mu) invstd: xhat_err = (L_e + 3) u (A_e + A_mu) invstd + |xhat| r
      z, y     : gamma xhat + beta, then the slope: |gamma| xhat_err + 2 u (|gamma xhat| + |beta|) + u |y|
      g        : dy times 1 or 0.2: u |g|.  dbeta = sum g and dgamma = sum g xhat_arg are double sums rounded once:
                 3 u sum |g|, and sum |g| xhat_err + 4 u sum |g xhat|
      dQ       : scale (g - k dbeta / M - Sx dgamma / M), Sx = sum_j xhat_ij a float sum of k terms, scale = gamma invstd: the
                 errors of dbeta, dgamma and Sx each times the absolute value of its cofactor, six roundings of the bracket's
                 terms, and (r + 3 u) |dQ| for the scale
      dP       : the same over the cnt edges arriving at a row, G = sum [arg] g among them a float sum of cnt terms
      dx, dW   : GEMMs of dP, dQ with |W1|, |W2 - W1| <= |W1| + |W2| (2 Cout + 3 roundings) and with X over the n rows (n + 2)"""
    x, W, gamma, beta, dy = (t.detach().to(F64) for t in (x, W, gamma, beta, dy))
    n, cin = x.shape
    k = idx.shape[1]
    W = W.reshape(W.shape[0], -1)
    cout = W.shape[0]
    M = n * k
    training = stats is None
    flat = idx.reshape(-1)
    e = edges(x, W, idx)
    y, arg, (mean, var) = edge_conv(x, W, gamma, beta, idx, stats, eps)
    inv = 1.0 / torch.sqrt(var + eps)
    xhat = (e - mean) * inv
    A_e = edges(x.abs(), torch.cat([W[:, :cin].abs(), W[:, cin:].abs() + 2 * W[:, :cin].abs()], 1), idx)  # |x_j||W1| + |x_i|(|W2| + |W1|)
    L_e = cin + 2
    if training:
        A_mu = A_e.reshape(-1, cout).mean(0)
        A_var = ((e - mean).abs() * (A_e + A_mu)).reshape(-1, cout).mean(0)
        r = (L_e + 2) * U32 * A_var / (var + eps) + 2 * U32
    else:
        A_mu = mean.abs()
        r = 4 * U32 * torch.ones_like(var)
    xhat_err = (L_e + 3) * U32 * (A_e + A_mu) * inv + xhat.abs() * r
    pick = lambda t: t.gather(1, arg[:, None, :])[:, 0, :]  # noqa: E731
    z = gamma * pick(xhat) + beta
    y_b = gamma.abs() * pick(xhat_err) + 2 * U32 * (gamma.abs() * pick(xhat.abs()) + beta.abs()) + U32 * y.abs()
    # backward
    g = dy * torch.where(z > 0, torch.ones_like(z), SLOPE * torch.ones_like(z))
    dbeta, dgamma = g.sum(0), (g * pick(xhat)).sum(0)
    dbeta_b = 3 * U32 * g.abs().sum(0)
    dgamma_b = (g.abs() * pick(xhat_err)).sum(0) + 4 * U32 * (g * pick(xhat)).abs().sum(0)
    into = lambda t: torch.zeros(n, cout, dtype=F64).index_add_(0, flat, t.reshape(-1, cout))  # noqa: E731  (sums over arriving edges)
    cnt = torch.bincount(flat, minlength=n).to(F64)[:, None]
    onehot = torch.zeros(n, k, cout, dtype=F64).scatter_(1, arg[:, None, :], 1.0)
    G, G_abs = into(onehot * g[:, None, :]), into(onehot * g.abs()[:, None, :])
    scale = gamma * inv
    t = 1.0 if training else 0.0
    Sx, Sx_b = xhat.sum(1), xhat_err.sum(1) + k * U32 * xhat.abs().sum(1)
    Tx, Tx_b = into(xhat), into(xhat_err) + cnt * U32 * into(xhat.abs())
    dQ = scale * (g - t * k * dbeta / M - t * Sx * dgamma / M)
    dP = scale * (G - t * cnt * dbeta / M - t * Tx * dgamma / M)
    dQ_b = scale.abs() * (U32 * g.abs() + t * (k * dbeta_b + Sx_b * dgamma.abs() + Sx.abs() * dgamma_b) / M
                          + 6 * U32 * (g.abs() + t * (k * dbeta.abs() + (Sx * dgamma).abs()) / M)) + (r + 3 * U32) * dQ.abs()
    dP_b = scale.abs() * ((cnt + 1) * U32 * G_abs + t * (cnt * dbeta_b + Tx_b * dgamma.abs() + Tx.abs() * dgamma_b) / M
                          + 6 * U32 * (G_abs + t * (cnt * dbeta.abs() + (Tx * dgamma).abs()) / M)) + (r + 3 * U32) * dP.abs()
    W1a, Wda, xa = W[:, :cin].abs(), W[:, cin:].abs() + W[:, :cin].abs(), x.abs()
    dx_b = dP_b @ W1a + dQ_b @ Wda + (2 * cout + 3) * U32 * (dP.abs() @ W1a + dQ.abs() @ Wda)
    dW2_b = dQ_b.t() @ xa + (n + 1) * U32 * (dQ.abs().t() @ xa)
    dW1_b = dP_b.t() @ xa + dW2_b + (n + 2) * U32 * ((dP.abs() + dQ.abs()).t() @ xa)
    out = {"y": y_b, "dx": dx_b, "dW": torch.cat([dW1_b, dW2_b], 1), "dgamma": dgamma_b, "dbeta": dbeta_b}
    if training:  # the batch statistics themselves (the running statistics are updated from them), each rounded to float once
        out["mean"] = (L_e + 1) * U32 * A_mu + U32 * mean.abs()
        out["var"] = 2 * (L_e + 2) * U32 * A_var + 2 * U32 * var
    return out


# ------------------------------------------------------------------------------------------------ the whole network
def batch_norm(x, gamma, beta, eps=BN_EPS):
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    return (x - mean) / torch.sqrt(var + eps) * gamma + beta


def dgcnn_forward(p, feats, off, k, forced_idx=None):
    """Logits [B, classes] of DGCNN_cls in train mode with dropout off, from the parameters by their state-dict names (float64
    leaves).  -> (logits, [the four neighbour tables used], [the four float64 layer inputs]).  `forced_idx`: four tables to use
    instead of the restatement's own."""
    x = feats.to(F64)
    used, inputs, outs = [], [], []
    for i in range(1, 5):
        inputs.append(x.detach())
        idx = knn(x.detach(), off, k) if forced_idx is None else forced_idx[i - 1].long()
        used.append(idx)
        x, _, _ = edge_conv(x, p[f"conv{i}.0.weight"], p[f"conv{i}.1.weight"], p[f"conv{i}.1.bias"], idx)
        outs.append(x)
    x = torch.cat(outs, 1) @ p["conv5.0.weight"].reshape(p["conv5.0.weight"].shape[0], -1).t()
    x = lrelu(batch_norm(x, p["conv5.1.weight"], p["conv5.1.bias"]))
    B = len(off) - 1
    pooled = torch.cat([torch.stack([x[off[b]:off[b + 1]].max(0).values for b in range(B)]),
                        torch.stack([x[off[b]:off[b + 1]].mean(0) for b in range(B)])], 1)
    h = lrelu(batch_norm(pooled @ p["linear1.weight"].t(), p["bn6.weight"], p["bn6.bias"]))
    h = lrelu(batch_norm(h @ p["linear2.weight"].t() + p["linear2.bias"], p["bn7.weight"], p["bn7.bias"]))
    return h @ p["linear3.weight"].t() + p["linear3.bias"], used, inputs
