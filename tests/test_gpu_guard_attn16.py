"""-m gpu: mink_attn_fwd_b16 / mink_attn_bwd_b16 (csrc/attn16.hip) inside guard bands (tests/guarded.py), in the form of
tests/test_gpu_guard_attn.py on Guarded buffers of torch.bfloat16: both entry points are called through the C ABI, every output
is a Guarded of EXACTLY the size include/mink_hip.h names, every input a Guarded.input with NaN bands and NaN pad columns, the
workspace exactly mink_attn_bwd_b16_workspace_bytes().  After each call: check() on every buffer (bands untouched, every logical
element written, pad columns and inputs bit for bit as they were), then every value finite and inside the derived bounds of
tests/attn16_restate.py.

Layouts: exact size (16-byte lanes); pad columns on every matrix (ld = width + 8: still 16-byte lanes; + 3: 2-byte lanes); out
and dqkv 2 bytes behind a 16-byte boundary; qkv 2 bytes behind one (each sends the call to the 2-byte lanes through one
pointer).  N = 1, 65 and 197: a tile of one row, one row past a tile, and the workload's own count.  Nothing here is meant to
fault: no buffer is smaller than the library asks for."""
import pytest
import torch

import attn_restate as AR
from guarded import Guarded, assert_finite, check_all
from test_gpu_attn16 import SCALE, reference

pytestmark = pytest.mark.gpu

B, H = 2, 2
BF = torch.bfloat16
LAYOUTS = {"exact": dict(pad=0), "pads": dict(pad=8), "odd pads": dict(pad=3), "skewed outputs": dict(pad=0, skew_out=2),
           "skewed qkv": dict(pad=0, skew_qkv=2)}


def _within(got, ref, bound, what):
    assert_finite(got, what)
    r = AR.worst(got, ref, bound)
    assert r <= 1, (what, r)
    return r


@pytest.mark.parametrize("N", [1, 65, 197])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_attention_b16_inside_guard_bands(layout, N):
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    cfg = dict(dict(pad=0, skew_out=0, skew_qkv=0), **LAYOUTS[layout])
    pad, dev, st = cfg["pad"], torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
    (q, k, v, dout), ref, bd = reference(B, H, N, "normal")
    W = H * 64
    qkv = Guarded.input(AR.pack_rows(q, k, v).to(dev, BF), ld=3 * W + pad, name="qkv", skew=cfg["skew_qkv"])
    out = Guarded((B * N, W + pad), BF, dev, cols=W, name="out", skew=cfg["skew_out"])
    lse = Guarded((B * H * N,), torch.float32, dev, name="lse")
    vec = pad % 8 == 0 and qkv.ptr % 16 == 0 and out.ptr % 16 == 0  # the host's lane decision, restated
    assert vec == (layout in ("exact", "pads"))
    check(L.mink_attn_fwd_b16(qkv.ptr, 3 * W + pad, B, N, H, 64, SCALE, out.ptr, W + pad, lse.ptr, st))
    torch.cuda.synchronize()
    check_all(qkv, out, lse)
    r = {"o": _within(AR.heads_of(out.logical().cpu(), B, N, H), ref["o"], bd["o"], "out"),
         "lse": _within(lse.t.cpu().reshape(B, H, N), ref["lse"], bd["lse"], "lse")}

    out_in = Guarded.input(out.logical().clone(), ld=W + pad, name="out (input)", skew=cfg["skew_out"])
    lse_in = Guarded.input(lse.t.clone(), name="lse (input)")
    g = Guarded.input(AR.rows_of(dout).to(dev, BF), ld=W + pad, name="dout")
    dqkv = Guarded((B * N, 3 * W + pad), BF, dev, cols=3 * W, name="dqkv", skew=cfg["skew_out"])
    need = L.mink_attn_bwd_b16_workspace_bytes(B, N, H, 64)
    assert need >= B * H * N * 4
    ws = Guarded(int(need), torch.uint8, dev, written="any", name="workspace")
    check(L.mink_attn_bwd_b16(qkv.ptr, 3 * W + pad, out_in.ptr, W + pad, lse_in.ptr, g.ptr, W + pad, B, N, H, 64, SCALE, dqkv.ptr,
                              3 * W + pad, ws.ptr, need, st))
    torch.cuda.synchronize()
    check_all(qkv, out_in, lse_in, g, dqkv, ws)
    for name, got in zip(("dq", "dk", "dv"), AR.split_rows(dqkv.logical().cpu(), B, N, H)):
        r[name] = _within(got, ref[name], bd[name], name)
    print(f"{layout}, N = {N}: error / bound " + " ".join(f"{n}={x:.3f}" for n, x in r.items()))
