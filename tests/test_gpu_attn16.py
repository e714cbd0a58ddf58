"""-m gpu: mink_attn_fwd_b16 / mink_attn_bwd_b16 (csrc/attn16.hip) against the float64 restatement of tests/attn_restate.py on
bf16-valued inputs, inside the DERIVED bounds of tests/attn16_restate.py: out, lse and the three gradients, through the C ABI
and through attention_b16.  Every case runs twice and must give the same bits.  Each test prints the largest error / bound it
saw; above 1 the kernel or the derivation is wrong.

The cases a-i are those of tests/test_gpu_attn.py, with their shapes and kinds; two more sit on the 32-key k-step of the bf16
MFMA:
    j (1, 2, 33)   the second half of a k-step holds one key      k (1, 2, 49)   one key past a filled k-step half"""
import functools

import pytest
import torch

import attn_restate as AR
import attn16_restate as A16
from test_gpu_attn import CASES as CASES32

pytestmark = pytest.mark.gpu

SCALE = 0.125
CASES = dict(CASES32, j=(1, 2, 33, "normal"), k=(1, 2, 49, "normal"))
BF = torch.bfloat16


@functools.lru_cache(None)
def reference(B, H, N, kind, seed=5):
    """(q, k, v, dout: bf16 values in fp32; float64 o, lse, dq, dk, dv; bounds), computed once per shape on the CPU and not
    modified."""
    q, k, v, dout = A16.inputs(B, H, N, seed=seed + N, kind=kind)
    f = AR.forward(q, k, v, SCALE)
    dq, dk, dv = AR.gradients(q, k, v, SCALE, dout)
    return (q, k, v, dout), {"o": f["o"], "lse": f["lse"], "dq": dq, "dk": dk, "dv": dv}, A16.bounds(q, k, v, SCALE, dout)


def padded(rows, pad, fill=float("nan")):
    """rows [n, w] on the GPU inside a bf16 [n, w + pad] matrix whose pad columns hold `fill` -> (matrix, ld)"""
    n, w = rows.shape
    m = torch.full((n, w + pad), fill, dtype=BF, device="cuda")
    m[:, :w] = rows
    return m, w + pad


def run_abi(q, k, v, dout, pad=0, out_pad_fill=float("nan")):
    """One forward and one backward call through the C ABI -> (out, lse, dqkv) as the padded device matrices.  The pad columns
    of the inputs hold NaN, those of the outputs `out_pad_fill`; every logical output element starts as NaN."""
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    B, H, N, D = q.shape
    st = torch.cuda.current_stream().cuda_stream
    qkv, ldq = padded(AR.pack_rows(q, k, v).cuda(), pad)
    g, lddo = padded(AR.rows_of(dout).cuda(), pad)
    out, ldo = padded(torch.full((B * N, H * D), float("nan"), device="cuda"), pad, out_pad_fill)
    dqkv, _ = padded(torch.full((B * N, 3 * H * D), float("nan"), device="cuda"), pad, out_pad_fill)
    lse = torch.full((B, H, N), float("nan"), device="cuda")
    check(L.mink_attn_fwd_b16(qkv.data_ptr(), ldq, B, N, H, D, SCALE, out.data_ptr(), ldo, lse.data_ptr(), st))
    ws = torch.empty(L.mink_attn_bwd_b16_workspace_bytes(B, N, H, D), dtype=torch.uint8, device="cuda")
    check(L.mink_attn_bwd_b16(qkv.data_ptr(), ldq, out.data_ptr(), ldo, lse.data_ptr(), g.data_ptr(), lddo, B, N, H, D, SCALE,
                              dqkv.data_ptr(), ldq, ws.data_ptr(), ws.numel(), st))
    torch.cuda.synchronize()
    return out, lse, dqkv


def ratios(out, lse, dqkv, shape, ref, bd):
    """largest error / bound of the five results, from row-layout device tensors"""
    B, H, N = shape
    gq, gk, gv = AR.split_rows(dqkv.cpu(), B, N, H)
    got = {"o": AR.heads_of(out.cpu(), B, N, H), "lse": lse.cpu(), "dq": gq, "dk": gk, "dv": gv}
    return {n: AR.worst(got[n], ref[n], bd[n]) for n in got}


@pytest.mark.parametrize("case", sorted(CASES))
def test_c_abi_within_the_derived_bounds(case):
    B, H, N, kind = CASES[case]
    (q, k, v, dout), ref, bd = reference(B, H, N, kind)
    first = run_abi(q, k, v, dout)
    r = ratios(*first, (B, H, N), ref, bd)
    print(f"case {case} (B, H, N) = {(B, H, N)} {kind}: error / bound " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    assert all(x <= 1 for x in r.values()), r
    again = run_abi(q, k, v, dout)
    assert all(torch.equal(a, b) for a, b in zip(first, again)), "two runs on the same inputs differ"
    if kind == "wide":
        assert float(ref["lse"].abs().max()) > 100  # (the scores do reach the range where exp without a maximum overflows)


@pytest.mark.parametrize("case", sorted(CASES))
def test_autograd_function_within_the_derived_bounds(case):
    from nerf_downstream_amd.minkowski import attention_b16

    B, H, N, kind = CASES[case]
    (q, k, v, dout), ref, bd = reference(B, H, N, kind)
    results = []
    for _ in range(2):
        qkv = AR.pack_rows(q, k, v).cuda().to(BF).requires_grad_(True)
        out = attention_b16(qkv, B, N, H)  # scale defaults to 64 ** -0.5
        assert out.dtype == BF
        out.backward(AR.rows_of(dout).cuda().to(BF))
        assert qkv.grad.dtype == BF
        results.append((out.detach(), qkv.grad))
    (out, grad), (out2, grad2) = results
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    r = ratios(out, torch.as_tensor(ref["lse"]).float(), grad, (B, H, N), ref, bd)
    print(f"case {case} through AttentionB16Function: error / bound " + " ".join(f"{n}={x:.3f}" for n, x in r.items() if n != "lse"))
    assert all(x <= 1 for n, x in r.items() if n != "lse"), r
    # the same kernels on the same alignment: the bits of the C-ABI run
    a_out, _, a_dqkv = run_abi(q, k, v, dout)
    assert torch.equal(out, a_out) and torch.equal(grad, a_dqkv)


def test_autograd_function_takes_a_row_pitch():
    from nerf_downstream_amd.minkowski import attention_b16

    B, H, N = 2, 3, 17
    (q, k, v, dout), _, _ = reference(B, H, N, "normal")
    rows = AR.pack_rows(q, k, v).cuda().to(BF)
    wide = torch.full((B * N, 3 * H * 64 + 8), float("nan"), dtype=BF, device="cuda")
    wide[:, : 3 * H * 64] = rows
    view = wide[:, : 3 * H * 64].detach().requires_grad_(True)
    plain = rows.clone().requires_grad_(True)
    g = AR.rows_of(dout).cuda().to(BF)
    a, b = attention_b16(view, B, N, H), attention_b16(plain, B, N, H)
    a.backward(g)
    b.backward(g)
    assert torch.equal(a, b) and torch.equal(view.grad, plain.grad)


@pytest.mark.parametrize("pad", [8, 3])  # ld = width + 8 keeps the 16-byte lanes, width + 3 takes the 2-byte lanes
def test_leading_dimensions_with_nan_pads(pad):
    B, H, N = 2, 3, 17
    (q, k, v, dout), ref, bd = reference(B, H, N, "normal")
    first = run_abi(q, k, v, dout, pad=pad)
    out, lse, dqkv = first
    assert bool(torch.isnan(out[:, H * 64:]).all()) and bool(torch.isnan(dqkv[:, 3 * H * 64:]).all())  # pads keep their NaN
    r = ratios(out, lse, dqkv, (B, H, N), ref, bd)
    print(f"ld = width + {pad}: error / bound " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
    assert all(x <= 1 for x in r.values()), r
    assert all(torch.equal(a[:, : a.shape[1] - pad] if a.dim() == 2 else a, b[:, : b.shape[1] - pad] if b.dim() == 2 else b)
               for a, b in zip(first, run_abi(q, k, v, dout, pad=pad)))
    # the narrow lanes compute what the 16-byte lanes compute, and a pitch changes no bit either
    plain = run_abi(q, k, v, dout)
    assert torch.equal(plain[0], out[:, : H * 64]) and torch.equal(plain[1], lse) and torch.equal(plain[2], dqkv[:, : 3 * H * 64])
