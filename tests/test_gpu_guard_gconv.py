"""-m gpu: mink_gconv_fwd / mink_gconv_wgrad (csrc/gconv.hip) inside guard bands (tests/guarded.py), by the rules of
tests/test_gpu_guard_attn.py: both entry points are called through the C ABI, every output is a Guarded of EXACTLY the size
include/mink_hip.h names, every input a Guarded.input with NaN bands and NaN pad columns, the workspace exactly
mink_gconv_wgrad_workspace_bytes().  After each call: check() on every buffer (bands untouched, every logical element written,
pad columns and inputs bit for bit as they were), then every value finite and inside the derived bounds of tests/gconv_restate.py.

Layouts: exact size (16-byte lanes); pad columns on every matrix (ld = width + 4: still 16-byte lanes; + 3: dword lanes); the
output 4 bytes behind a 16-byte boundary; the input 4 bytes behind one (each sends the call to the dword lanes through one
pointer).  Widths: vector FMA (32 x 4), matrix core (32 x 16, 32 x 64), generic (3 x 5 -> 7).  Rows: 1, 65 (one past a tile) and
1,380, a line of pixels with a 3-offset table [r - 1, r, r + 1] whose ends are -1.  Nothing here is meant to fault: no buffer is
smaller than the library asks for."""
import functools

import pytest
import torch

import gconv_restate as GR
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu

K = 3
LAYOUTS = {"exact": dict(pad=0), "pads": dict(pad=4), "odd pads": dict(pad=3), "skewed output": dict(pad=0, skew_out=4),
           "skewed input": dict(pad=0, skew_in=4)}


@functools.lru_cache(maxsize=None)
def reference(n, G, ci, co):
    r = torch.arange(n).view(n, 1) + torch.tensor([-1, 0, 1]).view(1, K)
    nbr = torch.where((r >= 0) & (r < n), r, torch.full_like(r, -1)).int()
    x, w, dy = GR.inputs(n, n, K, G, ci, co, seed=n + G + ci)
    return (x, w, dy, nbr), GR.reference(x, w, dy, nbr), GR.bounds(x, w, dy, nbr)


def _within(got, ref, bound, what):
    assert_finite(got, what)
    r = GR.worst(got, ref, bound)
    assert r <= 1, (what, r)
    return r


@pytest.mark.parametrize("n", [1, 65, 1380])
@pytest.mark.parametrize("G,ci,co", [(32, 4, 4), (32, 16, 16), (32, 64, 64), (3, 5, 7)])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_gconv_inside_guard_bands(layout, G, ci, co, n):
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    cfg = dict(dict(pad=0, skew_out=0, skew_in=0), **LAYOUTS[layout])
    pad, dev, st = cfg["pad"], torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
    (x, w, dy, nbr), ref, bd = reference(n, G, ci, co)
    Ci, Co = G * ci, G * co
    gx = Guarded.input(x.to(dev), ld=Ci + pad, name="x", skew=cfg["skew_in"])
    gw = Guarded.input(w.to(dev), name="w")
    gn = Guarded.input(nbr.to(dev), name="nbr")
    y = Guarded((n, Co + pad), torch.float32, dev, cols=Co, name="y", skew=cfg["skew_out"])
    check(L.mink_gconv_fwd(gx.ptr, n, Ci + pad, gw.ptr, 0, 0, gn.ptr, n, K, G, ci, co, y.ptr, Co + pad, st))
    torch.cuda.synchronize()
    check_all(gx, gw, gn, y)
    r = {"y": _within(y.logical().cpu(), ref["y"], bd["y"], "y")}

    # the data gradient through the same entry point: dy in, the forward weights read transposed and flipped, dx out
    gdy = Guarded.input(dy.to(dev), ld=Co + pad, name="dy", skew=cfg["skew_in"])
    dx = Guarded((n, Ci + pad), torch.float32, dev, cols=Ci, name="dx", skew=cfg["skew_out"])
    check(L.mink_gconv_fwd(gdy.ptr, n, Co + pad, gw.ptr, 1, 1, gn.ptr, n, K, G, co, ci, dx.ptr, Ci + pad, st))
    torch.cuda.synchronize()
    check_all(gdy, gw, gn, dx)
    r["dx"] = _within(dx.logical().cpu(), ref["dx"], bd["dx"], "dx")

    need = L.mink_gconv_wgrad_workspace_bytes(n, K, G, ci, co)
    assert need >= K * G * ci * co * 4
    dw = Guarded((K * G * ci * co,), torch.float32, dev, name="dw", skew=cfg["skew_out"])
    ws = Guarded(int(need), torch.uint8, dev, written="any", name="workspace")
    check(L.mink_gconv_wgrad(gx.ptr, n, Ci + pad, gdy.ptr, Co + pad, gn.ptr, n, K, G, ci, co, dw.ptr, ws.ptr, need, st))
    torch.cuda.synchronize()
    check_all(gx, gdy, gn, dw, ws)
    r["dw"] = _within(dw.t.cpu().reshape(K, G, ci, co), ref["dw"], bd["dw"], "dw")
    print(f"{layout}, (G, ci, co) = {(G, ci, co)}, n = {n}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))
