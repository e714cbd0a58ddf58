"""-m gpu: one NaN or +inf enters mink_attn_fwd_b16 / mink_attn_bwd_b16 (csrc/attn16.hip); where it comes out is held to the float64
restatement (tests/attn_restate.py), with the footprints of tests/test_gpu_attn_nonfinite.py on bf16 rows.  N = 37, so the 64-row tiles are padded: a zero-filled
tile row or a masked key that met the poison (0 x NaN) would show as a leak.

  * a NaN in one q element makes that (b, h, t) row of out and lse non-finite and nothing else;
  * a NaN or +inf in one k or v element makes exactly the reference's footprint non-finite, all of it inside that (b, h) (for k = +inf
    the rows whose score against that key is +inf; the rows whose score is -inf give the key the weight 0 and stay finite, and are
    held to the derived bounds of tests/attn16_restate.py for the attention without that key); a reference infinity may come out as any non-finite value
    (an infinite output element is a sum with an infinite term: which non-finite value it is depends on the order);
  * a NaN in one dout element gives the reference's footprint in dqkv (that row of dq, every dk of the (b, h), one column of dv);
  * everything outside the footprint -- other samples, other heads, the finite rows and columns of the poisoned (b, h) -- holds the
    bits of the clean run, and the pad columns of out and dqkv keep theirs."""
import pytest
import torch

import attn_restate as AR
import attn16_restate as A16
import footprint as FP
from test_gpu_attn16 import SCALE, reference, run_abi

pytestmark = pytest.mark.gpu

B, H, N = 2, 3, 37
AT = (1, 2, 5, 7)  # (b, h, token, channel) of the poisoned element
PAD, FILL = 8, 3.0  # (3.0 is a bf16 number)


def _run(q, k, v, dout):
    """-> out [B, H, N, 64], lse [B, H, N], (dq, dk, dv) on the CPU; the pad columns of both outputs must keep FILL"""
    out, lse, dqkv = run_abi(q, k, v, dout, pad=PAD, out_pad_fill=FILL)
    assert bool((out[:, H * 64:] == FILL).all()) and bool((dqkv[:, 3 * H * 64:] == FILL).all()), "a pad column was written"
    return AR.heads_of(out.cpu(), B, N, H), lse.cpu(), AR.split_rows(dqkv.cpu(), B, N, H)


def _clean():
    (q, k, v, dout), _, _ = reference(B, H, N, "normal")
    return (q, k, v, dout), _run(q, k, v, dout)


def _poisoned(t, value):
    t = t.clone()
    t[AT] = value
    return t


def _same_footprint_rest_clean(got, ref, clean, what):
    fg, fr = FP.footprint(got), FP.footprint(ref)
    assert 0 < int(fr.sum()) < fr.numel() / 2, (what, int(fr.sum()))  # visible: neither empty nor everything
    assert torch.equal(fg, fr), (f"{what}: footprint differs from the float64 reference's: {int((fr & ~fg).sum())} swallowed, "
                                 f"{int((fg & ~fr).sum())} leaked of {int(fr.sum())}")
    other = torch.ones_like(fr)
    other[AT[0], AT[1]] = False
    assert not bool(fr[other].any()), f"{what}: the reference footprint leaves the poisoned (b, h)"
    FP.untouched(got, clean, other, f"{what}: other samples and heads")
    return fr


def test_nan_in_q_poisons_one_output_row():
    (q, k, v, dout), (out0, lse0, _) = _clean()
    out, lse, _ = _run(_poisoned(q, float("nan")), k, v, dout)
    f = AR.forward(_poisoned(q, float("nan")), k, v, SCALE)
    row = torch.zeros(B, H, N, dtype=torch.bool)
    row[AT[:3]] = True
    assert torch.equal(FP.footprint(f["o"]), row[..., None].expand(-1, -1, -1, 64)) and torch.equal(FP.footprint(f["lse"]), row)
    assert torch.equal(FP.footprint(out), FP.footprint(f["o"])) and torch.equal(FP.footprint(lse), row)
    FP.untouched(out, out0, ~row[..., None], "q NaN: every other row of out")
    FP.untouched(lse, lse0, ~row, "q NaN: every other lse")


@pytest.mark.parametrize("value", ["nan", "+inf"])
def test_poison_in_k_follows_the_reference(value):
    (q, k, v, dout), (out0, lse0, _) = _clean()
    kp = _poisoned(k, FP.POISONS[value])
    out, lse, _ = _run(q, kp, v, dout)
    f = AR.forward(q, kp, v, SCALE)
    if value == "nan":  # every score against that key is NaN: every row of the (b, h)
        fr = FP.footprint(f["o"])
        assert bool(fr[AT[0], AT[1]].all())
        other = ~fr
        assert torch.equal(FP.footprint(out), fr) and torch.equal(FP.footprint(lse), FP.footprint(f["lse"]))
        FP.untouched(out, out0, other, "k NaN: other samples and heads")
        FP.untouched(lse, lse0, ~FP.footprint(f["lse"]), "k NaN: other samples and heads (lse)")
        return
    _same_footprint_rest_clean(out, f["o"], out0, "k +inf: out")
    frl = _same_footprint_rest_clean(lse, f["lse"], lse0, "k +inf: lse")
    # the finite rows of the (b, h) give the key the weight 0: attention over the other N - 1 keys, inside its derived bounds
    b, h, j, _ = AT
    rows = ~frl[b, h]
    assert 0 < int(rows.sum()) < N
    keep = torch.arange(N) != j
    sub = (q[b:b + 1, h:h + 1], k[b:b + 1, h:h + 1][:, :, keep], v[b:b + 1, h:h + 1][:, :, keep])
    ref, bd = AR.forward(*sub, SCALE), A16.bounds(*sub, SCALE)
    r_o = AR.worst(out[b, h][rows], ref["o"][0, 0][rows], bd["o"][0, 0][rows])
    r_l = AR.worst(lse[b, h][rows], ref["lse"][0, 0][rows], bd["lse"][0, 0][rows])
    print(f"k +inf: {int(rows.sum())} finite rows, error / bound o={r_o:.3f} lse={r_l:.3f}")
    assert r_o <= 1 and r_l <= 1


@pytest.mark.parametrize("value", ["nan", "+inf"])
def test_poison_in_v_follows_the_reference(value):
    (q, k, v, dout), (out0, lse0, _) = _clean()
    vp = _poisoned(v, FP.POISONS[value])
    out, lse, _ = _run(q, k, vp, dout)
    f = AR.forward(q, k, vp, SCALE)
    fr = _same_footprint_rest_clean(out, f["o"], out0, f"v {value}: out")
    col = torch.zeros(B, H, N, 64, dtype=torch.bool)
    col[AT[0], AT[1], :, AT[3]] = True
    assert torch.equal(fr, col)  # one column of every row of the (b, h)
    FP.untouched(out, out0, ~col, f"v {value}: the other columns")
    assert torch.equal(lse, lse0)  # v does not enter lse


def test_nan_in_dout_follows_the_reference():
    (q, k, v, dout), (out0, lse0, grads0) = _clean()
    gp = _poisoned(dout, float("nan"))
    out, lse, grads = _run(q, k, v, gp)
    assert torch.equal(out, out0) and torch.equal(lse, lse0)
    refs = AR.gradients(q, k, v, SCALE, gp)
    b, h, t, d = AT
    want = {"dq": torch.zeros(B, H, N, 64, dtype=torch.bool), "dk": torch.zeros(B, H, N, 64, dtype=torch.bool),
            "dv": torch.zeros(B, H, N, 64, dtype=torch.bool)}
    want["dq"][b, h, t], want["dk"][b, h], want["dv"][b, h, :, d] = True, True, True
    for name, got, ref, clean in zip(("dq", "dk", "dv"), grads, refs, grads0):
        assert torch.equal(FP.footprint(ref), want[name]), name  # the reference's footprint is the one the docstring names
        assert torch.equal(FP.footprint(got), want[name]), (name, int(FP.footprint(got).sum()), int(want[name].sum()))
        FP.untouched(got, clean, ~want[name], f"dout NaN: {name} outside the footprint")
