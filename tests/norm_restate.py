"""float64 restatement of MinkowskiInstanceNorm and MinkowskiLayerNorm with the fused residual add and ReLU: forward and the
four gradients (dx, dgamma, dbeta, d residual), written out from the formulas -- no autograd -- so that tests/test_norm_cpu.py
can hold it to torch's autograd and tests/test_gpu_norm.py can hold the HIP kernels to it.

    instance norm: sample b owns rows [off[b], off[b+1]); per channel  xhat = (x - mean_b) / sqrt(var_b + eps), biased var
    layer norm   : per row over the C channels                         xhat = (x - mean_r) / sqrt(var_r + eps)
    both         : z = xhat * gamma + beta [+ residual];  y = relu(z) or z
    backward     : g = dy * (y > 0) or dy;  d residual = g;  dgamma = sum_rows g * xhat;  dbeta = sum_rows g
                   dx = gamma * invstd * (g - mean(g) - xhat * mean(g * xhat))            (instance: means over the sample's rows)
                   dx = invstd * (g gamma - mean(g gamma) - xhat * mean(g gamma xhat))    (layer: means over the row's channels)
An empty sample contributes nothing; a one-row sample has variance 0, xhat = 0 and y = beta.
Also the fp32 error bounds the non-centred GPU tests assert (forward_bound / grad_bounds)."""
import torch

EPS32 = 2.0 ** -23  # one ulp of a float in [1, 2)


def _f64(t):
    return None if t is None else t.detach().double().cpu()


def sample_of_rows(offsets, n):
    """int64 [n]: the sample of every row, from explicit offsets [B+1]."""
    off = torch.as_tensor(offsets, dtype=torch.int64)
    assert int(off[0]) == 0 and int(off[-1]) == n and bool((off[1:] >= off[:-1]).all()), "offsets must cover the rows in order"
    return torch.repeat_interleave(torch.arange(off.numel() - 1), off[1:] - off[:-1])


def instance_stats(x, offsets, eps):
    """(mean [B, C], invstd [B, C], xhat [n, C]); an empty sample's mean / invstd are 0."""
    x = _f64(x)
    off = [int(o) for o in offsets]
    B, C = len(off) - 1, x.shape[1]
    mean, invstd, xhat = torch.zeros(B, C, dtype=torch.float64), torch.zeros(B, C, dtype=torch.float64), torch.empty_like(x)
    for b in range(B):
        s, e = off[b], off[b + 1]
        if e == s:
            continue
        seg = x[s:e]
        mean[b] = seg.mean(0)
        var = ((seg - mean[b]) ** 2).mean(0)
        invstd[b] = 1.0 / torch.sqrt(var + eps)
        xhat[s:e] = (seg - mean[b]) * invstd[b]
    return mean, invstd, xhat


def _tail(z, residual, relu):
    if residual is not None:
        z = z + _f64(residual)
    return z.clamp_min(0) if relu else z


def instance_norm_fwd(x, offsets, gamma, beta, eps, residual=None, relu=False):
    _, _, xhat = instance_stats(x, offsets, eps)
    return _tail(xhat * _f64(gamma).reshape(1, -1) + _f64(beta).reshape(1, -1), residual, relu)


def instance_norm_bwd(dy, x, offsets, gamma, beta, eps, residual=None, relu=False, mask=None):
    """-> (dx, dgamma, dbeta, dresidual).  `mask`: the ReLU decisions to use instead of float64's own (teacher forcing)."""
    x, dy, gamma = _f64(x), _f64(dy), _f64(gamma).reshape(1, -1)
    _, invstd, xhat = instance_stats(x, offsets, eps)
    g = dy
    if relu:
        if mask is None:
            mask = instance_norm_fwd(x, offsets, gamma, beta, eps, residual, True) > 0
        g = torch.where(mask.cpu().bool(), dy, torch.zeros_like(dy))  # (torch's threshold_backward: 0, also for a NaN dy)
    off = [int(o) for o in offsets]
    dx = torch.empty_like(x)
    for b in range(len(off) - 1):
        s, e = off[b], off[b + 1]
        if e == s:
            continue
        gs, xs = g[s:e], xhat[s:e]
        dx[s:e] = gamma * invstd[b] * (gs - gs.mean(0) - xs * (gs * xs).mean(0))
    return dx, (g * xhat).sum(0), g.sum(0), g


def layer_stats(x, eps):
    x = _f64(x)
    mean = x.mean(1, keepdim=True)
    var = ((x - mean) ** 2).mean(1, keepdim=True)
    invstd = 1.0 / torch.sqrt(var + eps)
    return mean, invstd, (x - mean) * invstd


def layer_norm_fwd(x, gamma, beta, eps, residual=None, relu=False):
    _, _, xhat = layer_stats(x, eps)
    return _tail(xhat * _f64(gamma).reshape(1, -1) + _f64(beta).reshape(1, -1), residual, relu)


def layer_norm_bwd(dy, x, gamma, beta, eps, residual=None, relu=False, mask=None):
    x, dy, gamma = _f64(x), _f64(dy), _f64(gamma).reshape(1, -1)
    _, invstd, xhat = layer_stats(x, eps)
    g = dy
    if relu:
        if mask is None:
            mask = layer_norm_fwd(x, gamma, beta, eps, residual, True) > 0
        g = torch.where(mask.cpu().bool(), dy, torch.zeros_like(dy))  # (torch's threshold_backward: 0, also for a NaN dy)
    gh = g * gamma
    dx = invstd * (gh - gh.mean(1, keepdim=True) - xhat * (gh * xhat).mean(1, keepdim=True))
    return dx, (g * xhat).sum(0), g.sum(0), g


# ------------------------------------------------------------------------------------------------ fp32 error bounds
# What fp32 INPUTS allow, whatever the kernel does inside.  The kernel reads x as floats and must hand mean and invstd to its
# apply pass as floats: the subtraction x - mean then carries an absolute error of up to ulp(max |x|) = max|x| * 2^-23 (half an
# ulp from rounding the mean, the rest from the subtraction and from x's own last bit being all the input says), which the
# normalisation multiplies by invstd * |gamma|.  On top come a few ulps of the result itself (the multiply-adds, the
# residual add, the store).  ULPS_OF_RESULT = 4 counts them: invstd rounding, two multiplies, one add.
ULPS_OF_RESULT = 4


def forward_bound(x, invstd_rows, gamma, y_ref):
    """[n, C] bound on |y - y_ref|: max|x| 2^-23 invstd |gamma| + ULPS_OF_RESULT ulps of y (of its largest term)."""
    x, gamma = _f64(x), _f64(gamma).reshape(1, -1)
    return x.abs().max() * EPS32 * invstd_rows * gamma.abs() + ULPS_OF_RESULT * EPS32 * y_ref.abs().clamp_min(1e-30)


def _group_mean(t, groups):
    """Mean of t over its normalisation group, broadcast back: over the rows of a sample (`groups` = sample of every row) per
    channel, or (`groups` None) over the channels of a row.  -> (mean, group size per element)."""
    if groups is None:
        return t.mean(1, keepdim=True).expand_as(t), torch.full_like(t, t.shape[1])
    B = int(groups.max()) + 1 if groups.numel() else 0
    cnt = torch.bincount(groups, minlength=B).double().clamp_min(1)
    m = torch.zeros(B, t.shape[1], dtype=torch.float64).index_add_(0, groups, t) / cnt[:, None]
    return m[groups], cnt[groups][:, None].expand_as(t)


def grad_bounds(g, x, xhat, invstd_rows, gamma, groups, dx_ref):
    """Bounds on the gradients, 'the same factor on the gradient terms'.  `groups`: NR.sample_of_rows(...) for instance norm
    (means over a sample's rows, gamma outside the means), None for layer norm (means over a row's channels of t = g gamma).
      e = max|x| 2^-23 invstd is the forward error xhat inherits from the float mean (gamma aside); it is COMMON to the
      group (one rounded mean), so it moves m2 = mean(t xhat) by e |m1|, m1 = mean(t), not by e mean|t|.
      dx = scale (t - m1 - xhat m2), scale = invstd |gamma| (instance) or invstd (layer).  Per element:
          xhat m2 : e |m2|  (xhat's error)  +  |xhat| (e |m1| + S mean|t xhat| + 2^-23 |m2|)  (m2's error: the common shift, the
                    rounding of the sum, m2 rounded to float),  S = log2(group size) 2^-24, the pairwise-sum bound
          m1      : S mean|t| + 2^-24 |m1|
          the two subtractions and the products: ULPS_OF_RESULT ulps of the largest of |t|, |m1|, |xhat m2|
      times scale, plus ULPS_OF_RESULT ulps of dx itself (invstd, gamma, the final multiplies).
      dgamma = sum g xhat: the common shift moves it by sum_groups |sum g| e; every product carries 2 ulps of itself (xhat's
               own rounding, the product), summed in double; plus the final rounding to float.
      dbeta  = sum g: exact in double up to the final rounding -> 2^-23 |dbeta| (+ one ulp of the largest term)."""
    x, g, gamma = _f64(x), _f64(g), _f64(gamma).reshape(1, -1)
    e = x.abs().max() * EPS32 * invstd_rows
    t = g if groups is not None else g * gamma
    scale = invstd_rows * (gamma.abs() if groups is not None else 1.0)
    m1, cnt = _group_mean(t, groups)
    m2, _ = _group_mean(t * xhat, groups)
    mabs, _ = _group_mean(t.abs(), groups)
    mxabs, _ = _group_mean((t * xhat).abs(), groups)
    S = torch.log2(cnt.clamp_min(2)) * EPS32 / 2
    m2_err = e * m1.abs() + S * mxabs + EPS32 * m2.abs()
    m1_err = S * mabs + EPS32 / 2 * m1.abs()
    largest = torch.maximum(torch.maximum(t.abs(), m1.abs()), (xhat * m2).abs())
    dx_b = scale * (e * m2.abs() + xhat.abs() * m2_err + m1_err + ULPS_OF_RESULT * EPS32 * largest) + ULPS_OF_RESULT * EPS32 * dx_ref.abs()
    if groups is not None:  # |sum g| per (sample, channel) times that sample's e, summed over the samples
        gsum = m1.abs() * e  # per row: |mean g| e; summed over the rows of a sample = |sum g| e
        shift = gsum.sum(0)
    else:  # every row has its own mean: the shifts are independent, |g_r| e_r each
        shift = (g.abs() * e).sum(0)
    dgamma_b = shift + (2 * EPS32 * (g * xhat).abs()).sum(0) + EPS32 * (g * xhat).sum(0).abs()
    dbeta_b = EPS32 * (g.sum(0).abs() + g.abs().max(0).values)
    return dx_b, dgamma_b, dbeta_b
