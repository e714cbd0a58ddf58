"""-m gpu: mink_kernel_map_cube, mink_conv_bigk_gather_gemm and mink_conv_bigk_wgrad (csrc/conv_bigk.hip) inside guard bands
(tests/guarded.py), by the rules of tests/test_gpu_guard_gconv.py: the entry points are called through the C ABI, every output
and table is a Guarded of EXACTLY the size include/mink_hip.h names, every input a Guarded.input with NaN bands and NaN pad
columns, the workspaces exactly what the *_workspace_bytes() queries return.  After each call: check() on every buffer (bands
untouched, every logical element written, pad columns and inputs bit for bit as they were), then every value finite and inside
the derived bound of tests/bigk_restate.py.

Layouts: exact size; pad columns on every matrix; the outputs 4 bytes behind a 16-byte boundary; the inputs 4 bytes behind one.
Rows: 1, one past the forward row tile, and a whole scene.  Nothing here is meant to fault: no buffer is smaller than the library
asks for."""
import functools

import numpy as np
import pytest
import torch

import bigk_restate as BR
from guarded import Guarded, assert_finite, check_all
from helpers import batch_scenes

pytestmark = pytest.mark.gpu

LAYOUTS = {"exact": dict(pad=0), "pads": dict(pad=4), "odd pads": dict(pad=3), "skewed output": dict(pad=0, skew_out=4),
           "skewed input": dict(pad=0, skew_in=4)}


@functools.lru_cache(maxsize=None)
def _coords():
    from oracle import maps

    maps.build()
    coords, _ = batch_scenes([11], grid=16, cin=1)
    inc = maps.quantize(coords.numpy())
    return inc[maps.unique(inc)[0]]


@functools.lru_cache(maxsize=None)
def reference(ks, n, cin, cout):
    from oracle import maps

    inc = _coords()
    n_in = inc.shape[0]
    nbr = maps.kernel_map_table(inc, inc, maps.kernel_offsets(ks, 1, 1))[: n if n > 0 else n_in]
    K = ks ** 3
    g = torch.Generator().manual_seed(ks + n + cin)
    x, w = torch.randn(n_in, cin, generator=g), torch.randn(K, cin, cout, generator=g) * (cin * K) ** -0.5
    dy, bias = torch.randn(nbr.shape[0], cout, generator=g), torch.randn(cout, generator=g)
    nbr_t = maps.transpose_table(nbr, n_in)
    return (x, w, dy, bias, nbr, nbr_t), (BR.forward(x, w, nbr, bias), BR.dgrad(dy, w, nbr, n_in), BR.wgrad(x, dy, nbr))


def _within(got, ref, what):
    assert_finite(got, what)
    r = BR.worst_ratio(got, *ref)
    assert r <= 1, (what, r)
    return r


@pytest.mark.parametrize("n", [1, 65, 0])  # 0 = every row of the scene
@pytest.mark.parametrize("ks,cin,cout", [(5, 3, 32), (7, 1, 32), (5, 28, 36), (5, 64, 64), (5, 70, 5)])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_bigk_convolution_inside_guard_bands(layout, ks, cin, cout, n):
    from nerf_downstream_amd._lib import check, lib

    L, K = lib(), ks ** 3
    cfg = dict(dict(pad=0, skew_out=0, skew_in=0), **LAYOUTS[layout])
    pad, dev, st = cfg["pad"], torch.device("cuda", 0), torch.cuda.current_stream().cuda_stream
    (x, w, dy, bias, nbr, nbr_t), ref = reference(ks, n, cin, cout)
    n_in, n_out = x.shape[0], nbr.shape[0]
    gx = Guarded.input(x.to(dev), ld=cin + pad, name="x", skew=cfg["skew_in"])
    gw = Guarded.input(w.to(dev), name="w", skew=cfg["skew_in"])
    gb = Guarded.input(bias.to(dev), name="bias")
    gn = Guarded.input(torch.from_numpy(nbr).to(dev), name="nbr")
    gt = Guarded.input(torch.from_numpy(nbr_t).to(dev), name="nbr_t")
    y = Guarded((n_out, cout + pad), torch.float32, dev, cols=cout, name="y", skew=cfg["skew_out"])
    check(L.mink_conv_bigk_gather_gemm(gx.ptr, n_in, cin + pad, cin, gw.ptr, 0, 0, gn.ptr, n_out, K, y.ptr, cout + pad, cout, gb.ptr, st))
    torch.cuda.synchronize()
    check_all(gx, gw, gb, gn, y)
    r = {"y": _within(y.logical().cpu(), ref[0], "y")}

    # the data gradient through the same entry point and the transposed table: dy in, the forward weights read transposed
    gdy = Guarded.input(dy.to(dev), ld=cout + pad, name="dy", skew=cfg["skew_in"])
    dx = Guarded((n_in, cin + pad), torch.float32, dev, cols=cin, name="dx", skew=cfg["skew_out"])
    check(L.mink_conv_bigk_gather_gemm(gdy.ptr, n_out, cout + pad, cout, gw.ptr, 1, 0, gt.ptr, n_in, K, dx.ptr, cin + pad, cin, None, st))
    torch.cuda.synchronize()
    check_all(gdy, gw, gt, dx)
    r["dx"] = _within(dx.logical().cpu(), ref[1], "dx")

    need = int(L.mink_conv_bigk_wgrad_workspace_bytes(n_out, K, cin, cout))
    dw = Guarded((K * cin * cout,), torch.float32, dev, name="dw", skew=cfg["skew_out"])
    ws = Guarded(need, torch.uint8, dev, written="any", name="workspace")
    check(L.mink_conv_bigk_wgrad(gx.ptr, n_in, cin + pad, cin, gdy.ptr, cout + pad, cout, gn.ptr, n_out, K, dw.ptr, ws.ptr, need, st))
    torch.cuda.synchronize()
    check_all(gx, gdy, gn, dw, ws)
    r["dw"] = _within(dw.t.cpu().reshape(K, cin, cout), ref[2], "dw")
    print(f"{layout}, ks {ks} {cin}->{cout}, rows {n_out}: error / bound " + " ".join(f"{k}={v:.3f}" for k, v in r.items()))


@pytest.mark.parametrize("ks,stride", [(5, 1), (7, 2)])
def test_cube_table_inside_guard_bands(oracle_maps, ks, stride):
    from nerf_downstream_amd._lib import check, lib

    L, K, dev = lib(), ks ** 3, torch.device("cuda", 0)
    inc = _coords()
    outc = inc if stride == 1 else oracle_maps.stride_map(inc, stride)[0]
    want = oracle_maps.kernel_map_table(inc, outc, oracle_maps.kernel_offsets(ks, 1, 1))
    gi = Guarded.input(torch.from_numpy(inc).to(dev), name="in_coords")
    go = Guarded.input(torch.from_numpy(np.ascontiguousarray(outc)).to(dev), name="out_coords")
    nbr = Guarded((outc.shape[0], K), torch.int32, dev, name="nbr")
    nbr_t = Guarded((inc.shape[0], K), torch.int32, dev, name="nbr_t")
    need = int(L.mink_kernel_map_cube_workspace_bytes(inc.shape[0]))
    ws = Guarded(need, torch.uint8, dev, written="any", name="workspace")
    check(L.mink_kernel_map_cube(gi.ptr, inc.shape[0], go.ptr, outc.shape[0], ks, 1, nbr.ptr, nbr_t.ptr, ws.ptr, need,
                                 torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    check_all(gi, go, nbr, nbr_t, ws)
    assert np.array_equal(nbr.t.cpu().numpy(), want)
    assert np.array_equal(nbr_t.t.cpu().numpy(), oracle_maps.transpose_table(want, inc.shape[0]))
