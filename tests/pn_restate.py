"""float64 restatement of MinkowskiPowerNorm with the fused residual add and ReLU: forward (training and eval), the four
gradients (dx, dweight, dbias, d residual) and both buffer updates, written out from the formulas -- no autograd -- so that
tests/test_powernorm_cpu.py can hold it to the recorded reference run (tests/golden/powernorm_ref_v1.npz) and to torch's
autograd for the differentiable part, and tests/test_gpu_powernorm.py can hold the HIP kernels (csrc/powernorm.hip) to it.

    group scaling : G groups of Cg = C / G channels;  m = mean over the group's channels of x^2;  r = 1/sqrt(m + 1e-5);  xh = x r
    training      : it = iters + 1;  var = mean over rows of xh^2;  s = 1/sqrt(var + eps) if it <= W else 1/sqrt(phi + eps)
                    (phi before the update);  z = xh s;  y = [relu](w z + b [+ residual]);
                    if it < W: phi = phi (it-1)/it + var/it;   always: phi = afwd phi + (1 - afwd) var
    eval          : s = 1/sqrt(phi + eps), nothing changes
    backward      : dym = dy * (y > 0) or dy;  g = dym w;  a = g - (1 - abkw) ema z;  ema += mean over rows of a z;
                    dxh = a / sqrt(var + eps) (training: the BATCH var also after warm-up; eval: a s);
                    dw = sum_rows dym z;  db = sum_rows dym;  d residual = dym;
                    dx = r (dxh - xh * mean over the group's channels of dxh xh)
Also the fp32 error bounds the GPU tests assert (forward_bound / phi_bound / grad_bounds)."""
import torch

EPS32 = 2.0 ** -23  # one ulp of a float in [1, 2)
U = EPS32 / 2       # one rounding to nearest
EPS_G = 1e-5        # the group scaling's own epsilon


def _f64(t):
    return None if t is None else t.detach().double().cpu()


def f32(v):
    """The fp32 value a Python scalar becomes when it is handed to a kernel as `float`."""
    return float(torch.tensor(float(v), dtype=torch.float32))


class State:
    """running_phi [C], ema_gz [C] (float64) and the step counter."""

    def __init__(self, running_phi, ema_gz, iters):
        self.running_phi, self.ema_gz, self.iters = _f64(running_phi).reshape(-1).clone(), _f64(ema_gz).reshape(-1).clone(), int(iters)

    @classmethod
    def fresh(cls, C):
        return cls(torch.ones(C), torch.zeros(C), 0)

    def clone(self):
        return State(self.running_phi, self.ema_gz, self.iters)


def group_scale(x, groups):
    """-> (r [n, G], xh [n, C])."""
    x = _f64(x)
    n, C = x.shape
    assert C % groups == 0
    xg = x.reshape(n, groups, C // groups)
    r = 1.0 / torch.sqrt((xg * xg).mean(2) + EPS_G)
    return r, (xg * r[:, :, None]).reshape(n, C)


def group_scale_bwd(dxh, r, xh, groups):
    """dx = r (dxh - xh * mean over the group's channels of dxh xh)."""
    n, C = xh.shape
    t = (dxh * xh).reshape(n, groups, C // groups).mean(2, keepdim=True)
    return ((dxh.reshape(n, groups, -1) - xh.reshape(n, groups, -1) * t) * r[:, :, None]).reshape(n, C)


def forward(x, w, b, state, eps, alpha_fwd=0.9, warmup_iters=10000, groups=1, training=True, residual=None, relu=False):
    """-> (y, aux, new state).  aux keeps what the backward and the bounds need; `state` is not modified."""
    w, b = _f64(w).reshape(1, -1), _f64(b).reshape(1, -1)
    r, xh = group_scale(x, groups)
    new = state.clone()
    phi = state.running_phi
    var = None
    if training:
        assert xh.shape[0] >= 1, "an empty batch has no second moment"
        it = new.iters = state.iters + 1
        var = (xh * xh).mean(0)
        s = 1.0 / torch.sqrt((var if it <= warmup_iters else phi) + eps)
        p = phi
        if it < warmup_iters:
            p = p * (it - 1) / it + var / it
        new.running_phi = alpha_fwd * p + (1 - alpha_fwd) * var
    else:
        s = 1.0 / torch.sqrt(phi + eps)
    z = xh * s
    wz = w * z
    pre = wz + b
    if residual is not None:
        pre = pre + _f64(residual)
    # (relu as the kernels and torch have it: a NaN stays a NaN)
    y = torch.where(pre <= 0, torch.zeros_like(pre), pre) if relu else pre
    return y, dict(r=r, xh=xh, var=var, s=s, z=z, wz=wz, wzb=wz + b, pre=pre, groups=groups, training=training, eps=eps), new


def backward(dy, aux, w, state, eps, alpha_bkw=0.9, relu=False, mask=None):
    """-> (dx, dweight, dbias, dresidual, new state, the intermediates grad_bounds() takes).  `mask`: the ReLU decisions to use
    instead of float64's own."""
    dy, w = _f64(dy), _f64(w).reshape(1, -1)
    z, xh, r = aux["z"], aux["xh"], aux["r"]
    g0 = dy
    if relu:
        if mask is None:
            mask = aux["pre"] > 0
        g0 = torch.where(mask.cpu().bool(), dy, torch.zeros_like(dy))  # (0 where masked, whatever dy holds)
    new = state.clone()
    if aux["training"]:
        a = g0 * w - ((1 - alpha_bkw) * state.ema_gz) * z
        new.ema_gz = state.ema_gz + (a * z).mean(0)
        dxh = a * (1.0 / torch.sqrt(aux["var"] + eps))
    else:
        a = g0 * w
        dxh = a * aux["s"]
    dx = group_scale_bwd(dxh, r, xh, aux["groups"])
    return dx, (g0 * z).sum(0), g0.sum(0), g0, new, dict(a=a, dxh=dxh, g0=g0)


# ------------------------------------------------------------------------------------------------ fp32 error bounds
# What a kernel with fp32 storage of r, var, s and of every per-element intermediate, and sums carried in double, can be held
# to.  Every count below is a number of roundings to nearest, u = 2^-24 relative each (EPS32 = 2u is one ulp); products of
# (1 + k u) factors are taken to first order and the second-order rest is covered by rounding every count UP to the next half.
#   sums     : the kernel adds Cg squares (group) and N squares / products (column) in double, in lanes, a butterfly and chunk
#              partials; whatever the order, a double sum of L terms of one sign is off by at most L 2^-53 relative:
#              SUM_REL(L) = L 2^-53, which enters every count below as (Cg + N) 2^-53 / u = (Cg + N) 2^-29 roundings -- 0.002 at
#              a million rows.  (A sum carried in fp32 would put log2(L) or L / chunk roundings here instead.)
#   r        : m in double from the exact float x, one rounding of 1/sqrt                                     1 u
#   xh = x r : r, the product                                                                                2 u
#   var      : every xh^2 off by 4 u, all of one sign so the mean is; its rounding to float                   5 u
#   s        : 1/sqrt(var + eps) halves var's error (eps > 0 only helps), one rounding            2.5 + 1 = 3.5 u   (training,
#              it <= W);  from the float running_phi the test hands over there is the rounding only: 1 u -- the larger holds
#   z = xh s : 2 + 3.5 + the product                                                                       6.5 u
#   w z      : the product (an fma into the add drops it: the bound keeps it)                              7.5 u  -> 4 ulps of |w z|
#   + b, + residual, relu: one rounding each of the running value: 1 u of |w z + b| + 1 u of |y| <= 1 ulp of the larger
Z_ROUNDINGS = 6.5
WZ_ULPS = 4.0       # ceil(7.5 u) in ulps
VAR_ROUNDINGS = 5.0
ISV_ROUNDINGS = 3.5


def sum_roundings(Cg, n):
    return (Cg + n) * 2.0 ** -29


def forward_bound(aux, y_ref, n=None):
    """[n, C] bound on |y - y_ref|: (WZ_ULPS + sums) ulps of |w z| + one ulp of max(|w z + b|, |y|)."""
    C = aux["z"].shape[1]
    n = aux["z"].shape[0] if n is None else n
    k = WZ_ULPS + sum_roundings(C // aux["groups"], n) / 2
    return k * EPS32 * aux["wz"].abs() + EPS32 * torch.maximum(aux["wzb"].abs(), y_ref.abs()) + 1e-37


def phi_bound(aux, state_before, state_after, alpha_fwd, warmup_iters):
    """[C] bound on |running_phi - reference|: var's error through the update's coefficient on var, plus the rounding of the
    new value (the update itself runs in double from the float phi and var)."""
    it = state_before.iters + 1
    coef = (alpha_fwd / it if it < warmup_iters else 0.0) + (1 - alpha_fwd)
    n, C = aux["z"].shape
    k = VAR_ROUNDINGS + sum_roundings(C // aux["groups"], n)
    return k * U * coef * aux["var"] + U * state_after.running_phi.abs() + 1e-37


def grad_bounds(aux, bwd, w, state_before, alpha_bkw, ref):
    """Bounds on (dx, dweight, dbias, ema_gz) from the magnitudes of the terms; `bwd` is the last dict backward() returns,
    `ref` = (dx, dweight, dbias, new ema_gz) of the restatement.  With ez = Z_ROUNDINGS u the relative error of the float z:
      a = g w - ke z, ke = fl((1 - abkw) ema):  u |g w| + (ez + 2 u) |ke z| + u |a|            (two products, ke, the subtraction)
      dxh = a isv:  isv err(a) + (ISV_ROUNDINGS + 1) u |dxh|      (eval: isv = s, the same count holds)
      ema  = fl(ema + mean a z):  mean(|z| err(a) + ez |a z|) + u |ema_new|
      dw   = fl(sum g z):  ez sum|g z| + u |dw|;        db = fl(sum g): u |db|   (both sums in double; + the sums' own term)
      t    = fl(mean_group dxh xh):  mean(|xh| err(dxh) + 2 u |dxh xh|) + u |t|                  <- the one cancellation: dx is
      dx   = fl(r fl(dxh - fl(xh t))):  r (err(dxh) + |xh| err(t) + 3 u |xh t| + u |dxh - xh t|) + 2 u |dx|   bounded by its terms"""
    w = _f64(w).reshape(1, -1)
    z, xh, r, G = aux["z"], aux["xh"], aux["r"], aux["groups"]
    n, C = z.shape
    Cg = C // G
    sr = sum_roundings(Cg, n) * U
    ez = Z_ROUNDINGS * U + sr
    a, dxh, g0 = bwd["a"], bwd["dxh"], bwd["g0"]
    dx_ref, dw_ref, db_ref, ema_ref = ref
    if aux["training"]:
        kez = ((1 - alpha_bkw) * state_before.ema_gz).reshape(1, -1) * z
        isv = (1.0 / torch.sqrt(aux["var"] + aux["eps"])).reshape(1, -1)
    else:
        kez = torch.zeros_like(z)
        isv = aux["s"].reshape(1, -1).abs()
    a_err = U * (g0 * w).abs() + (ez + 2 * U) * kez.abs() + U * a.abs()
    dxh_err = isv * a_err + ((ISV_ROUNDINGS + 1) * U + sr) * dxh.abs()
    ema_b = (z.abs() * a_err + ez * (a * z).abs()).mean(0) + (U + sr) * ema_ref.abs() + 1e-37
    dw_b = ez * (g0 * z).abs().sum(0) + (U + sr) * dw_ref.abs() + 1e-37
    db_b = (U + sr) * (db_ref.abs() + g0.abs().max(0).values) + 1e-37
    t = (dxh * xh).reshape(n, G, Cg).mean(2, keepdim=True)
    t_err = ((xh.abs() * dxh_err + 2 * U * (dxh * xh).abs()).reshape(n, G, Cg).mean(2, keepdim=True) + (U + sr) * t.abs())
    xhg, xt = xh.reshape(n, G, Cg), xh.reshape(n, G, Cg) * t
    diff_err = dxh_err.reshape(n, G, Cg) + xhg.abs() * t_err + 3 * U * xt.abs() + U * (dxh.reshape(n, G, Cg) - xt).abs()
    dx_b = (r[:, :, None] * diff_err).reshape(n, C) + 2 * U * dx_ref.abs() + 1e-37
    return dx_b, dw_b, db_b, ema_b
