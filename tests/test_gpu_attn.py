"""-m gpu: mink_attn_fwd / mink_attn_bwd (csrc/attn.hip) against the float64 restatement of tests/attn_restate.py, inside its
DERIVED bounds: out, lse and the three gradients, through the C ABI and through AttentionFunction.  Every case runs twice and
must give the same bits.  Each test prints the largest error / bound it saw; above 1 the kernel or the derivation is wrong.

    a (1, 1, 1)    softmax of one element                      f (2, 6, 197)  the workload's own token count
    b (2, 3, 5)    a 32^2 image; B != H shows a swapped index  g (1, 1, 577)  several key tiles, online rescaling
    c, d, e (1, 2, 63 / 64 / 65)  around the 64-row tile       h (1, 2, 37)   scores spanning +-200
                                                               i (1, 2, 37)   v with a mean of 50: dP - delta cancels"""
import functools

import pytest
import torch

import attn_restate as AR

pytestmark = pytest.mark.gpu

SCALE = 0.125
CASES = {"a": (1, 1, 1, "normal"), "b": (2, 3, 5, "normal"), "c": (1, 2, 63, "normal"), "d": (1, 2, 64, "normal"),
         "e": (1, 2, 65, "normal"), "f": (2, 6, 197, "normal"), "g": (1, 1, 577, "normal"), "h": (1, 2, 37, "wide"),
         "i": (1, 2, 37, "offset")}


@functools.lru_cache(None)
def reference(B, H, N, kind, seed=5):
    """(q, k, v, dout fp32; float64 o, lse, dq, dk, dv; bounds), computed once per shape on the CPU and not modified."""
    q, k, v, dout = AR.inputs(B, H, N, seed=seed + N, kind=kind)
    f = AR.forward(q, k, v, SCALE)
    dq, dk, dv = AR.gradients(q, k, v, SCALE, dout)
    return (q, k, v, dout), {"o": f["o"], "lse": f["lse"], "dq": dq, "dk": dk, "dv": dv}, AR.bounds(q, k, v, SCALE, dout)


def padded(rows, pad, fill=float("nan")):
    """rows [n, w] on the GPU inside a [n, w + pad] matrix whose pad columns hold `fill` -> (matrix, ld)"""
    n, w = rows.shape
    m = torch.full((n, w + pad), fill, dtype=torch.float32, device="cuda")
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
    check(L.mink_attn_fwd(qkv.data_ptr(), ldq, B, N, H, D, SCALE, out.data_ptr(), ldo, lse.data_ptr(), st))
    ws = torch.empty(L.mink_attn_bwd_workspace_bytes(B, N, H, D), dtype=torch.uint8, device="cuda")
    check(L.mink_attn_bwd(qkv.data_ptr(), ldq, out.data_ptr(), ldo, lse.data_ptr(), g.data_ptr(), lddo, B, N, H, D, SCALE,
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
    from nerf_downstream_amd.minkowski import attention

    B, H, N, kind = CASES[case]
    (q, k, v, dout), ref, bd = reference(B, H, N, kind)
    results = []
    for _ in range(2):
        qkv = AR.pack_rows(q, k, v).cuda().requires_grad_(True)
        out = attention(qkv, B, N, H)  # scale defaults to 64 ** -0.5
        out.backward(AR.rows_of(dout).cuda())
        results.append((out.detach(), qkv.grad))
    (out, grad), (out2, grad2) = results
    assert torch.equal(out, out2) and torch.equal(grad, grad2)
    r = ratios(out, torch.as_tensor(ref["lse"]).float(), grad, (B, H, N), ref, bd)
    print(f"case {case} through AttentionFunction: error / bound " + " ".join(f"{n}={x:.3f}" for n, x in r.items() if n != "lse"))
    assert all(x <= 1 for n, x in r.items() if n != "lse"), r
    # the same kernels on the same alignment: the bits of the C-ABI run
    a_out, _, a_dqkv = run_abi(q, k, v, dout)
    assert torch.equal(out, a_out) and torch.equal(grad, a_dqkv)


@pytest.mark.parametrize("pad", [4, 3])  # ld = width + 4 keeps the 16-byte lanes, width + 3 takes the dword lanes
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
    if pad == 3:  # the dword lanes compute what the 16-byte lanes compute
        plain = run_abi(q, k, v, dout)
        assert torch.equal(plain[0], out[:, : H * 64]) and torch.equal(plain[1], lse) and torch.equal(plain[2], dqkv[:, : 3 * H * 64])
