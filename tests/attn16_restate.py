"""DERIVED error bounds of the bf16-row attention (csrc/attn16.hip) against the float64 restatement of tests/attn_restate.py,
and a torch emulation of its arithmetic contract (not a test).

The reference is AR.forward / AR.gradients in float64 on bf16-VALUED inputs (inputs() below rounds AR.inputs() through
.bfloat16()), so the rounding of the inputs is part of no error.  The contract (include/mink_hip.h): every product on the bf16
MFMA with fp32 accumulation -- a product of two bf16 numbers is exact in fp32, so a dot product errs as the fp32 fmaf chain of
attn_restate does -- and everything else fp32, except five roundings to bf16 (nearest even, relative error <= U16 = 2^-8):

    F1  bf16(exp(s - m)) as the operand of P V; the row sum l, and so lse, use the unrounded weights
    F2  the stored out
    B1  bf16(exp(s - lse)) as the operand of dV = P^T dO
    B2  bf16(P o (dP - delta)) as the operand of dQ and dK, formed in fp32 from the unrounded P
    B3  the stored dqkv, after the scale

The bounds.  The notation, u = 2^-24, sigma, eta, etabar, lambda, pi, rho and the rule of ONE leading factor 2 per bound for
the dropped second-order terms are those of attn_restate's docstring; only what the five roundings add is new.

  lse       l sums the unrounded fp32 weights and the scores are never rounded to bf16: the bound is AR.bounds()["lse"],
            unchanged.  (An implementation that summed the rounded weights would carry U16 here, 2^16 times the bound.)
  output    o_id = bf16(sum_j bf16(p_ij) v_jd / l_i).  Each weight gains the relative error U16 of F1 next to the fp32 terms
            eta_ij + etabar_i + (2 N + 2) u, and the stored value the relative error U16 of F2:
                |o^_id - o_id| <= E_id = 2 (sum_j w_ij |v_jd| (eta_ij + etabar_i + (2 N + 2) u + U16) + U16 |o_id|).
  P         exp(s^ - lse^) in fp32 from the unrounded scores and the fp32 lse: pi_ij as in attn_restate.
  dV        dV_jd = bf16(sum_i bf16(P_ij) dO_id): U16 per weight (B1), the N-term chain, U16 of the stored value (B3):
                |dV^_jd - dV_jd| <= 2 (sum_i w_ij |dO_id| (pi_ij + U16 + (N + 1) u) + U16 |dV_jd|).
  dP        bf16 products are exact, the D-term chain is fp32: rho_ij = (D + 1) u b_ij, unchanged.
  delta     delta_i = sum_d dO_id o^_id, an fp32 sum over the STORED out: it carries the output bound E_id above, which now
            includes F1 and F2 (with its factor 2), besides its own chain:
                tau_i = sum_d |dO_id| E_id + (D + 1) u sum_d |dO_id| |o_id|.
  dS        dS_ij = bf16(P_ij (dP_ij - delta_i)): P relative pi_ij, dP and delta absolute, the subtraction and the product one
            fp32 rounding each, then U16 of B2:
                |dS^_ij - dS_ij| <= w_ij zeta_ij,   zeta_ij = (pi_ij + 2 u + U16) |dP_ij - delta_i| + rho_ij + tau_i.
  dQ, dK    N-term fp32 chains, the scale (one rounding), U16 of the stored value (B3):
                |dQ^_id - dQ_id| <= 2 (scale sum_j |k_jd| w_ij (zeta_ij + (N + 2) u |dP_ij - delta_i|) + U16 |dQ_id|)
                |dK^_jd - dK_jd| <= 2 (scale sum_i |q_id| w_ij (zeta_ij + (N + 2) u |dP_ij - delta_i|) + U16 |dK_jd|).

Nothing in a bound is fitted to an implementation's error."""
import torch

import attn_restate as AR

U = AR.U
U16 = 2.0 ** -8
TILE = 64  # keys per step of the online softmax in csrc/attn16.hip


def inputs(B, H, N, seed, kind="normal"):
    """AR.inputs() rounded to bf16 values, kept in fp32: (q, k, v, dout) [B, H, N, 64]"""
    return tuple(t.bfloat16().float() for t in AR.inputs(B, H, N, seed, kind))


def bounds(q, k, v, scale, dout=None):
    """The bounds of the module docstring -> dict(o, lse[, dq, dk, dv]) of float64 tensors shaped like what they bound."""
    base = AR.bounds(q, k, v, scale)
    q, k, v = q.double(), k.double(), v.double()
    N, D = q.shape[-2], q.shape[-1]
    f = AR.forward(q, k, v, scale)
    s, m, w, o, lse = f["s"], f["m"], f["w"], f["o"], f["lse"]
    a = q.abs() @ k.abs().transpose(-1, -2)
    sigma = (D + 2) * U * scale * a
    eta = sigma + ((s - m[..., None]).abs() + 4) * U
    etabar = (w * eta).sum(-1)
    E = 2 * ((w * (eta + etabar[..., None] + (2 * N + 2) * U + U16)) @ v.abs() + U16 * o.abs())
    out = {"o": E, "lse": base["lse"]}
    if dout is None:
        return out
    g = dout.double()
    dq, dk, dv = AR.gradients(q, k, v, scale, g)
    lam = base["lse"] / 2
    pi = sigma + 2 * lam[..., None] + ((s - lse[..., None]).abs() + 3) * U
    out["dv"] = 2 * ((w * (pi + U16 + (N + 1) * U)).transpose(-1, -2) @ g.abs() + U16 * dv.abs())
    rho = (D + 1) * U * (g.abs() @ v.abs().transpose(-1, -2))
    tau = (g.abs() * E).sum(-1) + (D + 1) * U * (g.abs() * o.abs()).sum(-1)
    diff = (g @ v.transpose(-1, -2) - (g * o).sum(-1, keepdim=True)).abs()
    zeta = (pi + 2 * U + U16) * diff + rho + tau[..., None]
    e = w * (zeta + (N + 2) * U * diff)
    out["dq"] = 2 * (scale * (e @ k.abs()) + U16 * dq.abs())
    out["dk"] = 2 * (scale * (e.transpose(-1, -2) @ q.abs()) + U16 * dk.abs())
    return out


def _r(x):
    return x.bfloat16().float()


def emulate(q, k, v, scale, dout=None, variant=None):
    """The contract in torch on the CPU: fp32 arithmetic on bf16-valued inputs, .bfloat16().float() at F1, F2, B1, B2 and B3, the
    online softmax over TILE-key tiles -> dict(o, lse[, dq, dk, dv]).  variant: None, or one of the deliberately WRONG forms
    "scale_twice", "no_max" (no maximum subtracted), "lse_rounded" (l sums the bf16-rounded weights)."""
    q, k, v = q.float(), k.float(), v.float()
    B, H, N, D = q.shape
    sc = scale * scale if variant == "scale_twice" else scale
    m = torch.full((B, H, N), float("-inf"))
    l = torch.zeros(B, H, N)
    acc = torch.zeros(B, H, N, D)
    for k0 in range(0, N, TILE):
        s = (q @ k[:, :, k0:k0 + TILE].transpose(-1, -2)) * sc
        mn = torch.zeros_like(m) if variant == "no_max" else torch.maximum(m, s.max(-1).values)
        alpha = torch.exp(m - mn) if variant != "no_max" else torch.ones_like(m)
        p = torch.exp(s - mn[..., None])
        l = l * alpha + (_r(p) if variant == "lse_rounded" else p).sum(-1)
        acc = acc * alpha[..., None] + _r(p) @ v[:, :, k0:k0 + TILE]  # F1
        m = mn
    o = _r(acc / l[..., None])  # F2
    lse = m + torch.log(l)
    out = {"o": o, "lse": lse}
    if dout is None:
        return out
    g = dout.float()
    delta = (g * o).sum(-1)
    P = torch.exp((q @ k.transpose(-1, -2)) * sc - lse[..., None])
    dP = g @ v.transpose(-1, -2)
    dS = _r(P * (dP - delta[..., None]))  # B2
    out["dv"] = _r(_r(P).transpose(-1, -2) @ g)  # B1, B3
    out["dq"] = _r((dS @ k) * sc)  # B3
    out["dk"] = _r((dS.transpose(-1, -2) @ q) * sc)
    return out
