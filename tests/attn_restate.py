"""Float64 restatement of multi-head self-attention and the DERIVED error bounds of an fp32 implementation (not a test).

Written from the formulas, on explicit [B, H, N, D] tensors (tests/test_attn_cpu.py holds it to a per-(b, h, i) loop):

    s_ij = scale * sum_d q_id k_jd        m_i = max_j s_ij        w_ij = exp(s_ij - m_i) / sum_j exp(s_ij - m_i)
    o_id = sum_j w_ij v_jd                lse_i = m_i + log sum_j exp(s_ij - m_i)

and the gradients of sum(o * dout) by autograd in float64.  The backward an implementation runs is

    dV = P^T dO,   dP = dO V^T,   delta_i = sum_d dO_id o_id,   dS = P o (dP - delta),   dQ = scale dS K,   dK = scale dS^T Q

with P = exp(s - lse) recomputed.

The bounds.  First-order rounding analysis with u = 2^-24 (the unit roundoff of fp32), absolute values of the operands
everywhere, and ONE leading factor 2 per bound for the dropped second-order terms.  The inputs (fp32 values) are exact.

  score     An fp32 dot product of D terms as an fmaf chain (what the fp32 MFMA computes: one rounding per product-and-add) is
            off by at most D u sum_d |q_id| |k_jd|; the scale costs at most two more roundings (one when it multiplies the
            finished sum, one more if an implementation scaled q first).  With a_ij = sum_d |q_id| |k_jd|:
                sigma_ij = (D + 2) u scale a_ij.
  weight    The unnormalised weight p_ij = exp(s_ij - m_i) is computed from the rounded score, a rounded subtraction (u |x|,
            x = s_ij - m_i), an exponential that is exp2-based (its argument rounding scales with |x|; together with the
            subtraction that is the |x| u term) and good to a few ulps of its result, and the rescale factors of the online
            softmax: a tile that was weighted against an earlier maximum m' is multiplied by exp(m' - m'') ... whose arguments
            telescope to m' - m_i, so their |x|-proportional errors are those of one exponential of s_ij - m_i.  The constant
            covers the exponentials' own ulps and the rescale multiplications.  The relative error of p_ij is at most
                eta_ij = sigma_ij + (|s_ij - m_i| + 4) u.
            (The maximum an implementation subtracts is itself a rounded score; a common shift of a row cancels in w and in lse.)
            The row sum l_i = sum_j p_ij inherits etabar_i = sum_j w_ij eta_ij and adds N u for its N additions.
  output    o_id = sum_j p_ij v_jd / l_i: the relative error of w_ij is eta_ij + etabar_i + N u (sum), the N-term fmaf chain
            over j adds N u sum_j w_ij |v_jd|, the division and the last rescale two more roundings:
                |o^_id - o_id| <= 2 sum_j w_ij |v_jd| (eta_ij + etabar_i + (2 N + 2) u).
  lse       m^ + log(l^) is the exact log-sum-exp of the rounded scores but for the errors of l^ (etabar_i + N u, and the
            (|x| + 4) u of every p_ij inside etabar), of the logarithm (two ulps of log l_i = lse_i - m_i) and of the last
            addition (u |lse_i|):
                lambda_i = etabar_i + (N + 2) u + u (|lse_i| + 2 |lse_i - m_i|),        |lse^_i - lse_i| <= 2 lambda_i.
  P         The backward's P^_ij = exp(s^_ij - lse^_i) has the relative error (the subtraction is rounded relative to
            |s_ij - lse_i|, the exponential as above, lse^ as given by the forward):
                pi_ij = sigma_ij + 2 lambda_i + (|s_ij - lse_i| + 3) u.
  dV        dV_jd = sum_i w_ij dO_id, an N-term chain over i:
                |dV^_jd - dV_jd| <= 2 sum_i w_ij |dO_id| (pi_ij + (N + 1) u).
  dP        a D-term chain: rho_ij = (D + 1) u b_ij with b_ij = sum_d |dO_id| |v_jd|.
  delta     delta_i = sum_d dO_id o^_id is formed from the forward's ROUNDED output, so it carries the output bound E_id above
            (with its factor 2) besides its own chain:
                tau_i = sum_d |dO_id| E_id + (D + 1) u sum_d |dO_id| |o_id|.
  dS        dS_ij = w_ij (dP_ij - delta_i): the errors of P (relative pi_ij), of dP and delta (absolute, they do NOT shrink when
            dP - delta cancels), one rounding for the subtraction and one for the product:
                |dS^_ij - dS_ij| <= w_ij zeta_ij,   zeta_ij = (pi_ij + 2 u) |dP_ij - delta_i| + rho_ij + tau_i.
  dQ, dK    dQ_id = scale sum_j dS_ij k_jd and dK_jd = scale sum_i dS_ij q_id: N-term chains and one rounding for the scale,
                |dQ^_id - dQ_id| <= 2 scale sum_j |k_jd| w_ij (zeta_ij + (N + 2) u |dP_ij - delta_i|)
                |dK^_jd - dK_jd| <= 2 scale sum_i |q_id| w_ij (zeta_ij + (N + 2) u |dP_ij - delta_i|).

Nothing in a bound is fitted to an implementation's error.  A measured error above its bound means that the implementation or
this derivation is wrong."""
import math

import torch

U = 2.0 ** -24


def split_rows(qkv, B, N, H):
    """packed rows [B N, >= 3 H D] (column s H D + h D + d) -> q, k, v as [B, H, N, D] views in the rows' dtype."""
    D = 64
    x = qkv[:, : 3 * H * D].reshape(B, N, 3, H, D)
    return tuple(x[:, :, s].permute(0, 2, 1, 3) for s in range(3))


def heads_of(rows, B, N, H):
    """rows [B N, >= H D] (column h D + d) -> [B, H, N, D]"""
    D = 64
    return rows[:, : H * D].reshape(B, N, H, D).permute(0, 2, 1, 3)


def rows_of(x):
    """[B, H, N, D] -> rows [B N, H D]"""
    B, H, N, D = x.shape
    return x.permute(0, 2, 1, 3).reshape(B * N, H * D)


def pack_rows(q, k, v):
    """q, k, v [B, H, N, D] -> packed rows [B N, 3 H D]"""
    return torch.cat([rows_of(q), rows_of(k), rows_of(v)], dim=1)


def forward(q, k, v, scale, dtype=torch.float64, variant=None):
    """-> dict(s, m, w, o, lse) computed in `dtype`.  variant: None, or one of the deliberately WRONG forms
    tests/test_attn_cpu.py checks the bounds against: "no_max" (no maximum subtracted), "scale_twice"."""
    q, k, v = q.to(dtype), k.to(dtype), v.to(dtype)
    s = (q @ k.transpose(-1, -2)) * scale
    if variant == "scale_twice":
        s = s * scale
    m = s.max(dim=-1, keepdim=True).values
    shift = torch.zeros_like(m) if variant == "no_max" else m
    p = torch.exp(s - shift)
    l = p.sum(dim=-1, keepdim=True)
    w = p / l
    return {"s": s, "m": m.squeeze(-1), "w": w, "o": w @ v, "lse": (shift + torch.log(l)).squeeze(-1)}


def gradients(q, k, v, scale, dout, dtype=torch.float64, variant=None):
    """-> (dq, dk, dv) of sum(o * dout) by autograd through forward() in `dtype`."""
    q, k, v = (t.detach().to(dtype).clone().requires_grad_(True) for t in (q, k, v))
    o = forward(q, k, v, scale, dtype, variant)["o"]
    return torch.autograd.grad(o, (q, k, v), dout.to(dtype))


def bounds(q, k, v, scale, dout=None):
    """The bounds of the module docstring -> dict(o, lse[, dq, dk, dv]) of float64 tensors shaped like what they bound."""
    q, k, v = q.double(), k.double(), v.double()
    N, D = q.shape[-2], q.shape[-1]
    f = forward(q, k, v, scale)
    s, m, w, o, lse = f["s"], f["m"], f["w"], f["o"], f["lse"]
    a = q.abs() @ k.abs().transpose(-1, -2)
    sigma = (D + 2) * U * scale * a
    eta = sigma + ((s - m[..., None]).abs() + 4) * U
    etabar = (w * eta).sum(-1)
    out = {"o": 2 * ((w * (eta + etabar[..., None] + (2 * N + 2) * U)) @ v.abs())}
    lam = etabar + (N + 2) * U + U * (lse.abs() + 2 * (lse - m).abs())
    out["lse"] = 2 * lam
    if dout is None:
        return out
    g = dout.double()
    pi = sigma + 2 * lam[..., None] + ((s - lse[..., None]).abs() + 3) * U
    out["dv"] = 2 * ((w * (pi + (N + 1) * U)).transpose(-1, -2) @ g.abs())
    rho = (D + 1) * U * (g.abs() @ v.abs().transpose(-1, -2))
    tau = (g.abs() * out["o"]).sum(-1) + (D + 1) * U * (g.abs() * o.abs()).sum(-1)
    diff = (g @ v.transpose(-1, -2) - (g * o).sum(-1, keepdim=True)).abs()
    zeta = (pi + 2 * U) * diff + rho + tau[..., None]
    e = w * (zeta + (N + 2) * U * diff)
    out["dq"] = 2 * scale * (e @ k.abs())
    out["dk"] = 2 * scale * (e.transpose(-1, -2) @ q.abs())
    return out


def worst(got, ref, bound):
    """max over the elements of |got - ref| / bound; inf when a value is not finite or an error stands against a zero bound."""
    err = (got.double() - ref).abs()
    if not bool(torch.isfinite(err).all()):
        return math.inf
    ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
    return float(ratio.max()) if ratio.numel() else 0.0


def inputs(B, H, N, seed, kind="normal"):
    """fp32 (q, k, v, dout) [B, H, N, 64].  kind: "normal" (unit normals: scores of a few units), "wide" (q scaled so the scores
    span about +-200), "offset" (v with a mean of 50: dP - delta cancels)."""
    g = torch.Generator().manual_seed(seed)
    q, k, v, dout = (torch.randn(B, H, N, 64, generator=g) for _ in range(4))
    if kind == "wide":
        s = (q.double() @ k.double().transpose(-1, -2)).abs().max() * 0.125
        q = q * float(200.0 / s)
    elif kind == "offset":
        v = v + 50.0
    else:
        assert kind == "normal", kind
    return q, k, v, dout
