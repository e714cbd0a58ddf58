"""-m gpu: sparse convolution with 5^3 / 7^3 kernels (csrc/conv_bigk.hip).

1. Tables: mink_kernel_map_cube bit-equal to oracle.maps.kernel_map_table / transpose_table -- through the C ABI on edge-case
   coordinate sets, through CoordinateManager.kernel_table (on demand and prepared ahead) on two scenes.
2. Operators: forward, data gradient (stride 1 through the flipped forward table, stride 2 through the transposed table) and
   weight gradient against the float64 restatement tests/bigk_restate.py under its derived bound 2 (T + 2) 2^-24 S per element;
   row counts around the kernels' row tiles, pitched and misaligned operands, a lone last-row offset, bit-identical runs, the
   bf16 math mode changing nothing; non-finite footprints (tests/footprint.py).
3. Modules against oracle.me_cpu in the pattern of test_gpu_resunet.py::test_down_up_convolutions_kernel3_match_oracle.
4. Networks: ResUNetBN2C with a 5^3 / 7^3 stem under the criteria of test_gpu_resunet.py::test_resunet_matches_oracle;
   MinkowskiFCNN(kernel_size=5) under those of test_gpu_point.py::test_networks_match_float64_restatement (the float64
   restatement of tests/point_restate.py: the CPU oracle has no point modules)."""
import functools

import numpy as np
import pytest
import torch

import bigk_restate as BR
import footprint as FP
import point_restate as PT
from helpers import batch_scenes, misaligned

pytestmark = pytest.mark.gpu


def _consts():
    from nerf_downstream_amd._lib import CONSTANTS

    return CONSTANTS["MINK_BIGK_ROW_TILE"], CONSTANTS["MINK_BIGK_WGRAD_ROWS"]


def _note(line):
    """Printed (pytest -s shows it): the figures of profiles/bigk_kernels.txt."""
    print(line)


# ================================================================================================ 1. tables
def _block(n, lo=0, step=1, b=0):
    g = np.arange(n) * step + lo
    z, y, x = np.meshgrid(g, g, g, indexing="ij")
    return np.stack([np.full(x.size, b), x.ravel(), y.ravel(), z.ravel()], 1).astype(np.int32)


def _edge_sets():
    solid = _block(9)
    plane = _block(12)
    plane = plane[plane[:, 3] == 0]
    extremes = np.array([[0, 32767, 5, 5], [0, 32766, 5, 5], [0, 32764, 5, 5], [0, -32768, 5, 5], [0, -32767, 5, 5],
                         [0, 5, 32767, -32768], [0, 5, 32766, -32767], [0, 0, 0, 0],
                         [65534, 0, 0, 0], [65534, 1, 1, 1], [65534, 32767, 32767, 32767], [65534, -32768, -32768, -32768]], np.int32)
    return {
        "solid 9^3": solid,
        "solid 9^3 + isolated voxel": np.concatenate([solid, np.array([[0, 30, 30, 30]], np.int32)]),
        "plane": plane,
        "negative": _block(7, lo=-20),
        "key-range limits": extremes,
    }


def _cube_tables(inc, outc, ks, step):
    from nerf_downstream_amd._lib import check, lib

    L, K = lib(), ks ** 3
    ic, oc = torch.from_numpy(inc).cuda(), torch.from_numpy(outc).cuda()
    nbr = torch.full((outc.shape[0], K), 12345, dtype=torch.int32, device="cuda")
    nbr_t = torch.full((inc.shape[0], K), 12345, dtype=torch.int32, device="cuda")
    ws = torch.empty(int(L.mink_kernel_map_cube_workspace_bytes(inc.shape[0])), dtype=torch.uint8, device="cuda")
    check(L.mink_kernel_map_cube(ic.data_ptr(), inc.shape[0], oc.data_ptr(), outc.shape[0], ks, step, nbr.data_ptr(), nbr_t.data_ptr(),
                                 ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream))
    return nbr.cpu().numpy(), nbr_t.cpu().numpy()


@pytest.mark.parametrize("ks,stride,dil", [(5, 1, 1), (5, 2, 1), (7, 1, 1), (7, 2, 1), (5, 1, 2)])
def test_cube_tables_on_edge_cases(oracle_maps, ks, stride, dil):
    K, r = ks ** 3, (ks - 1) // 2
    for ts in (1, 2):  # at tensor stride 2 the coordinates are multiples of 2
        for name, inc in _edge_sets().items():
            if ts == 2:
                if name == "key-range limits":
                    continue
                inc = inc.copy()
                inc[:, 1:] *= 2
            outc = inc if stride == 1 else oracle_maps.stride_map(inc, ts * stride)[0]
            step = dil * ts
            want = oracle_maps.kernel_map_table(inc, outc, oracle_maps.kernel_offsets(ks, ts, dil))
            nbr, nbr_t = _cube_tables(inc, outc, ks, step)
            what = f"{name}, ks {ks} stride {stride} dilation {dil} ts {ts}"
            assert np.array_equal(nbr, want), what
            assert np.array_equal(nbr_t, oracle_maps.transpose_table(want, inc.shape[0])), what
            off = oracle_maps.kernel_offsets(ks, 1, 1)
            if name == "solid 9^3" and stride == 1 and dil == 1:
                centre = np.nonzero((inc[:, 1:] == 4 * ts).all(1))[0][0]
                assert (nbr[centre] >= 0).all()
                assert int((nbr >= 0).all(1).sum()) == (9 - 2 * r) ** 3  # the interior rows have every neighbour
            if name == "solid 9^3 + isolated voxel" and stride == 1:
                assert (nbr[-1] >= 0).sum() == 1 and nbr[-1, K // 2] == inc.shape[0] - 1  # only its centre
            if name == "plane" and stride == 1:
                assert (nbr[:, off[:, 2] != 0] == -1).all() and (nbr[:, off[:, 2] == 0] >= 0).any(0).all()
            if name == "key-range limits" and stride == 1 and dil == 1:
                # x = 32767 has nothing at +1 (the key would wrap onto x = -32768 of the same y, z) and x = -32768 nothing at -1
                kp, km = K // 2 + 1, K // 2 - 1
                assert nbr[0, kp] == -1 and nbr[0, km] == 1 and nbr[3, km] == -1 and nbr[3, kp] == 4
                assert (nbr[8:] < 8).sum() == (nbr[8:] == -1).sum()  # batch 65534 only sees its own rows
                assert nbr[8, off.tolist().index([1, 1, 1])] == 9


@functools.lru_cache(maxsize=None)
def _scene(grid=16, cin=4, seeds=(11, 12)):
    coords, feats = batch_scenes(list(seeds), grid=grid, cin=cin)
    return coords, feats


def _manager(coords, feats):
    from nerf_downstream_amd import minkowski as ME

    x = ME.TensorField(coordinates=coords.cuda(), features=feats.cuda()).sparse()
    return x, x.coordinate_manager


@pytest.mark.parametrize("grid", [16, 24])
def test_manager_tables_match_oracle(oracle_maps, grid):
    from nerf_downstream_amd.minkowski.coords import CoordinateMapKey

    coords, feats = _scene(grid)
    x, m = _manager(coords, feats)
    k1 = x.coordinate_map_key
    k2 = m.stride(k1, 2)
    c1, c2 = m.get_coordinates(k1).cpu().numpy(), m.get_coordinates(k2).cpu().numpy()
    assert 600 <= c1.shape[0] <= 2400 * 2
    cases = [(k1, k1, c1, c1, 5, 1), (k1, k1, c1, c1, 7, 1), (k1, k2, c1, c2, 5, 1), (k1, k2, c1, c2, 7, 1), (k1, k1, c1, c1, 5, 2),
             (k2, k2, c2, c2, 5, 1), (k2, k2, c2, c2, 7, 1)]
    for ki, ko, ci, co, ks, dil in cases:
        want = oracle_maps.kernel_map_table(ci, co, oracle_maps.kernel_offsets(ks, ki.ts, dil))
        nbr, nbr_t = m.kernel_table(ki, ko, ks, dil)
        assert nbr_t is None and np.array_equal(nbr.cpu().numpy(), want), (ki.ts, ko.ts, ks, dil)
        nbr2, nbr_t = m.kernel_table(ki, ko, ks, dil, transposed=True)
        assert np.array_equal(nbr2.cpu().numpy(), want)
        assert np.array_equal(nbr_t.cpu().numpy(), oracle_maps.transpose_table(want, ci.shape[0]))
        frac = float((want >= 0).mean())
        print(f"[bigk] grid {grid} ts {ki.ts}->{ko.ts} ks {ks} dil {dil}: {want.shape[0]} rows, {frac * ks ** 3:.1f} of {ks ** 3} neighbours per row")
    # stride 1, centred: the transposed table is the table with the offsets flipped (what the data gradient relies on)
    nbr, nbr_t = m.kernel_table(k1, k1, 7, 1, transposed=True)
    assert torch.equal(nbr_t, nbr.flip(1))
    # the ME-format lists of the diagnostic accessor
    lists = m.kernel_map(k1, k2, stride=2, kernel_size=5)
    want = oracle_maps.table_to_lists(oracle_maps.kernel_map_table(c1, c2, oracle_maps.kernel_offsets(5, 1, 1)))
    assert sorted(lists) == sorted(want)
    for k in want:
        assert lists[k].dtype == torch.int32 and np.array_equal(lists[k].cpu().numpy(), want[k]), k
    # the same tables from a prepared-ahead plan: a second manager replays the first one's trace
    plan = m.compile_plan(m.trace)
    assert any(op[0] == "ktable" and op[3] == 7 for op in plan)
    x2, m2 = _manager(coords, feats)
    m2.stride(x2.coordinate_map_key, 2)
    m2.replay(plan)
    for key, (a, b) in m.tables.items():
        if isinstance(key, tuple) and len(key) == 4 and key[2] in (5, 7):
            a2, b2 = m2.tables[key]
            assert torch.equal(a, a2) and (b is None or torch.equal(b, b2)), key
    assert isinstance(k2, CoordinateMapKey)


# ================================================================================================ 2. operators
CHANNELS = [(1, 32), (3, 32), (4, 32), (28, 36), (64, 64)]


@functools.lru_cache(maxsize=None)
def _tables(ks, stride, grid=16):
    from oracle import maps

    maps.build()
    coords, _ = _scene(grid)
    inc = maps.quantize(coords.numpy())
    inc = inc[maps.unique(inc)[0]]
    outc = inc if stride == 1 else maps.stride_map(inc, stride)[0]
    nbr = maps.kernel_map_table(inc, outc, maps.kernel_offsets(ks, 1, 1))
    return inc.shape[0], nbr, maps.transpose_table(nbr, inc.shape[0])


@functools.lru_cache(maxsize=None)
def _operands(n_in, n_out, K, cin, cout):
    g = torch.Generator().manual_seed(K + 7 * cin + cout)
    x = torch.randn(n_in, cin, generator=g)
    w = torch.randn(K, cin, cout, generator=g) * (cin * K) ** -0.5
    dy = torch.randn(n_out, cout, generator=g)
    bias = torch.randn(cout, generator=g)
    return x, w, dy, bias


def _three(x, w, dy, bias, nbr_np, nbr_t_np, stride):
    """forward, data gradient and weight gradient on the device -> cpu tensors."""
    from nerf_downstream_amd.minkowski import functional as Fn

    K, cin, cout = w.shape
    nbr = torch.from_numpy(np.ascontiguousarray(nbr_np)).cuda()
    xd, wd, dyd = x.cuda(), w.cuda(), dy.cuda()
    y = Fn.gather_gemm(xd, wd, nbr, cout, bias=None if bias is None else bias.cuda())
    if stride == 1:
        dx = Fn.gather_gemm(dyd, wd, nbr, cin, w_transposed=True, flip_k=True)
    else:
        dx = Fn.gather_gemm(dyd, wd, torch.from_numpy(np.ascontiguousarray(nbr_t_np)).cuda(), cin, w_transposed=True)
    dw = Fn.conv_wgrad(xd, dyd, nbr, (K, cin, cout))
    torch.cuda.synchronize()
    return y.cpu(), dx.cpu(), dw.cpu()


def _hold(got, ref, what):
    ratios = {}
    for name, g, (r, T, S) in zip(("y", "dx", "dw"), got, ref):
        assert tuple(g.shape) == r.shape, (what, name, tuple(g.shape), r.shape)
        assert bool(torch.isfinite(g).all()), (what, name)
        ratios[name] = BR.worst_ratio(g, r, T, S)
    _note(f"[bigk] {what}: largest |err| / bound " + " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, (what, ratios)
    return ratios


@pytest.mark.parametrize("cin,cout", CHANNELS)
@pytest.mark.parametrize("ks,stride", [(5, 1), (7, 1), (5, 2), (7, 2)])
def test_operators_within_the_derived_bound(ks, stride, cin, cout):
    n_in, nbr, nbr_t = _tables(ks, stride)
    x, w, dy, bias = _operands(n_in, nbr.shape[0], ks ** 3, cin, cout)
    got = _three(x, w, dy, bias, nbr, nbr_t, stride)
    ref = (BR.forward(x, w, nbr, bias), BR.dgrad(dy, w, nbr, n_in), BR.wgrad(x, dy, nbr))
    _hold(got, ref, f"ks {ks} stride {stride} {cin}->{cout}, {nbr.shape[0]} rows")
    # two runs give the same bits, and so does the bf16 math mode (these kernels are fp32 in every mode)
    from nerf_downstream_amd.minkowski import functional as Fn

    again = _three(x, w, dy, bias, nbr, nbr_t, stride)
    old = Fn.set_conv_math("bf16")
    try:
        b16 = _three(x, w, dy, bias, nbr, nbr_t, stride)
    finally:
        Fn.set_conv_math(old)
    for a, b, c in zip(got, again, b16):
        assert torch.equal(a, b) and torch.equal(a, c)


def _row_counts():
    tm, rt = _consts()
    return sorted({0, 1, rt - 1, rt, rt + 1, tm - 1, tm, tm + 1, 2 * tm + 1})


@pytest.mark.parametrize("cin,cout", [(3, 32), (28, 36), (64, 64)])
def test_row_counts_around_the_tiles(cin, cout):
    ks = 5
    n_in, nbr_full, _ = _tables(ks, 1)
    for n in _row_counts():
        nbr = nbr_full[:n]
        x, w, dy, bias = _operands(n_in, nbr_full.shape[0], ks ** 3, cin, cout)
        dy = dy[:n]
        from nerf_downstream_amd.minkowski import functional as Fn

        nd = torch.from_numpy(np.ascontiguousarray(nbr)).cuda().reshape(n, ks ** 3)
        y = Fn.gather_gemm(x.cuda(), w.cuda(), nd, cout, bias=bias.cuda())
        dw = Fn.conv_wgrad(x.cuda(), dy.cuda(), nd, tuple(w.shape))
        # the data gradient of the truncated table: the rows of x that the first n outputs reach, through its transpose
        from oracle import maps

        nt = torch.from_numpy(maps.transpose_table(nbr, n_in)).cuda()
        dx = Fn.gather_gemm(dy.cuda(), w.cuda(), nt, cin, w_transposed=True)
        torch.cuda.synchronize()
        assert y.shape == (n, cout) and dx.shape == (n_in, cin) and dw.shape == w.shape
        if n == 0:
            assert not bool(dw.any()) and not bool(dx.any())
        ref = (BR.forward(x, w, nbr, bias), BR.dgrad(dy, w, nbr, n_in), BR.wgrad(x, dy, nbr, cin, cout))
        _hold((y.cpu(), dx.cpu(), dw.cpu()), ref, f"rows {n}, ks 5 {cin}->{cout}")


@pytest.mark.parametrize("cin,cout", [(3, 32), (28, 36)])
def test_pitched_and_misaligned_operands(cin, cout):
    from nerf_downstream_amd.minkowski import functional as Fn

    ks = 7
    n_in, nbr, _ = _tables(ks, 1)
    x, w, dy, bias = _operands(n_in, nbr.shape[0], ks ** 3, cin, cout)
    ref = (BR.forward(x, w, nbr, bias), BR.dgrad(dy, w, nbr, n_in), BR.wgrad(x, dy, nbr))
    clean = _three(x, w, dy, bias, nbr, None, 1)
    nd = torch.from_numpy(nbr).cuda()
    # a row pitch above the channel count, the pad columns NaN
    xw = torch.full((n_in, cin + 3), float("nan"), device="cuda")
    xw[:, :cin] = x.cuda()
    dyw = torch.full((nbr.shape[0], cout + 5), float("nan"), device="cuda")
    dyw[:, :cout] = dy.cuda()
    xp, dyp = xw[:, :cin], dyw[:, :cout]
    assert xp.stride(0) == cin + 3 and dyp.stride(0) == cout + 5
    got = (Fn.gather_gemm(xp, w.cuda(), nd, cout, bias=bias.cuda()), Fn.gather_gemm(dyp, w.cuda(), nd, cin, w_transposed=True, flip_k=True),
           Fn.conv_wgrad(xp, dyp, nd, tuple(w.shape)))
    _hold([g.cpu() for g in got], ref, f"pitched, ks 7 {cin}->{cout}")
    for a, b in zip(got, clean):
        assert torch.equal(a.cpu(), b)
    # every operand 4 bytes behind a 16-byte boundary
    (_, xm), (_, dym) = misaligned(x), misaligned(dy)
    _, wm = misaligned(w.reshape(ks ** 3 * cin, cout))
    wm = wm.view(ks ** 3, cin, cout)
    got = (Fn.gather_gemm(xm, wm, nd, cout, bias=bias.cuda()), Fn.gather_gemm(dym, wm, nd, cin, w_transposed=True, flip_k=True),
           Fn.conv_wgrad(xm, dym, nd, tuple(w.shape)))
    for a, b in zip(got, clean):
        assert torch.equal(a.cpu(), b)


def test_offset_present_only_for_the_last_row_of_a_tile():
    from nerf_downstream_amd.minkowski import functional as Fn

    tm, rt = _consts()
    K, cin, cout, n = 125, 5, 20, 2 * tm
    nbr = np.full((n, K), -1, np.int32)
    nbr[tm - 1, 7] = 3          # last row of the first forward tile, an offset nobody else has
    nbr[2 * tm - 1, 100] = 9    # last row of the second
    nbr[rt - 1, 33] = 11        # last row of the first weight-gradient step
    nbr[tm, 124] = 0            # first row of a tile, last offset
    nbr[5, 62] = 5              # a centre
    x, w, dy, bias = _operands(16, n, K, cin, cout)
    ref = (BR.forward(x, w, nbr, None), BR.dgrad(dy, w, nbr, 16), BR.wgrad(x, dy, nbr))
    nd = torch.from_numpy(nbr).cuda()
    y = Fn.gather_gemm(x.cuda(), w.cuda(), nd, cout)
    dw = Fn.conv_wgrad(x.cuda(), dy.cuda(), nd, (K, cin, cout))
    from oracle import maps

    dx = Fn.gather_gemm(dy.cuda(), w.cuda(), torch.from_numpy(maps.transpose_table(nbr, 16)).cuda(), cin, w_transposed=True)
    _hold((y.cpu(), dx.cpu(), dw.cpu()), ref, "lone last-row offsets")
    rows = sorted({tm - 1, 2 * tm - 1, rt - 1, tm, 5})
    assert sorted(set(y.cpu().abs().sum(1).nonzero().flatten().tolist())) == rows  # every other row is exactly zero
    assert sorted(set(dw.cpu().abs().sum((1, 2)).nonzero().flatten().tolist())) == [7, 33, 62, 100, 124]


# ------------------------------------------------------------------------------------------------ non-finite footprints
@pytest.mark.parametrize("value", list(FP.POISONS))
@pytest.mark.parametrize("ks,stride,cin,cout", [(5, 1, 3, 32), (7, 2, 4, 32), (5, 2, 28, 36), (5, 1, 64, 64)])
def test_non_finite_footprints(ks, stride, cin, cout, value):
    """One poisoned value in rows of x (forward, weight gradient) or of the incoming gradient (data gradient, weight gradient)
    comes out in exactly the elements whose window -- or weight-gradient offset -- holds that row: a skipped empty offset loses
    none, a zero-filled absent neighbour creates none.  Weights are not poisoned."""
    v = FP.POISONS[value]
    n_in, nbr, nbr_t = _tables(ks, stride)
    n_out = nbr.shape[0]
    x, w, dy, bias = _operands(n_in, n_out, ks ** 3, cin, cout)
    unnamed = [int(i) for i in np.nonzero(~np.isin(np.arange(n_in), nbr[nbr >= 0]))[0][:1]]  # a row no window holds (stride 2: none)
    xp = FP.poison(x, v, FP.poison_rows(n_in, unnamed))
    dyp = FP.poison(dy, v, FP.poison_rows(n_out))
    with np.errstate(invalid="ignore", over="ignore"):
        rf = BR.forward(xp, w, nbr, bias)
        rd = BR.dgrad(dyp, w, nbr, n_in)
        rwx, rwy = BR.wgrad(xp, dy, nbr), BR.wgrad(x, dyp, nbr)
    t64 = lambda a: torch.from_numpy(a)  # noqa: E731
    FP.visible({"y": t64(rf[0]), "dx": t64(rd[0])}, f"bigk ks {ks} stride {stride} {cin}->{cout} {value}")
    FP.visible_reduction({"dw (x poisoned)": t64(rwx[0]), "dw (dy poisoned)": t64(rwy[0])}, "bigk dw")
    assert int(FP.footprint(t64(rwy[0])).sum()) < rwy[0].size  # some offset has no poisoned row: a leak would show
    y, _, dwx = _three(xp, w, dy, bias, nbr, nbr_t, stride)
    _, dx, dwy = _three(x, w, dyp, bias, nbr, nbr_t, stride)
    what = f"ks {ks} stride {stride} {cin}->{cout} {value}"
    with np.errstate(invalid="ignore"):
        for name, got, (r, T, S) in (("y", y, rf), ("dx", dx, rd), ("dw, x poisoned", dwx, rwx), ("dw, dy poisoned", dwy, rwy)):
            b = torch.from_numpy(np.nan_to_num(BR.bound(T, S), nan=0.0, posinf=0.0))
            FP.same_footprint(got, t64(r), b, f"{what}: {name}")


# ================================================================================================ 3. modules against the oracle
@pytest.mark.parametrize("cin,cmid,cout", [(3, 32, 20), (28, 16, 36)])
def test_k5_then_k7_stride2_chain_matches_oracle(oracle_maps, cin, cmid, cout):
    from nerf_downstream_amd import minkowski as ME
    from oracle import me_cpu as OME

    torch.manual_seed(0)
    coords, feats = batch_scenes([21, 22], grid=16, cin=cin)
    ra = OME.MinkowskiConvolution(cin, cmid, kernel_size=5, stride=1, bias=True, dimension=3)
    rb = OME.MinkowskiConvolution(cmid, cout, kernel_size=7, stride=2, bias=True, dimension=3)
    ha = ME.MinkowskiConvolution(cin, cmid, kernel_size=5, stride=1, bias=True, dimension=3).cuda()
    hb = ME.MinkowskiConvolution(cmid, cout, kernel_size=7, stride=2, bias=True, dimension=3).cuda()
    assert ha.kernel.shape == (125, cin, cmid) and hb.kernel.shape == (343, cmid, cout)
    ha.load_state_dict(ra.state_dict()), hb.load_state_dict(rb.state_dict())

    rx = OME.TensorField(coordinates=coords, features=feats).sparse()
    rF = rx.F.detach().clone().requires_grad_(True)
    ry = ra(OME.SparseTensor(rF, rx.coordinate_map_key, rx._manager))
    rz = rb(ry)
    hx = ME.TensorField(coordinates=coords.cuda(), features=feats.cuda()).sparse()
    hF = hx.F.detach().clone().requires_grad_(True)
    hy = ha(ME.SparseTensor(hF, hx.coordinate_map_key, hx.coordinate_manager), bn_stats=True)
    hz = hb(hy)
    # bn_stats=True is accepted and yields no partial: the norm that follows reduces on its own
    hc = ME.MinkowskiConvolution(cin, 8, kernel_size=5, dimension=3).cuda()
    hn = ME.MinkowskiBatchNorm(8).cuda()
    yc = hc(hx, bn_stats=True)
    assert getattr(yc, "_bn_partial", 0) is None
    with torch.no_grad():
        assert torch.allclose(hn(yc).F.mean(0), torch.zeros(8, device="cuda"), atol=1e-5)
    assert hy.tensor_stride[0] == 1 and hz.tensor_stride[0] == 2
    assert torch.equal(hx.C.cpu(), rx.C) and torch.equal(hz.C.cpu(), rz.C)
    print(f"[bigk] k5 s1 -> k7 s2 ({cin}, {cmid}, {cout}): y max|diff| {float((hy.F.cpu() - ry.F).abs().max()):.2e}, "
          f"z max|diff| {float((hz.F.cpu() - rz.F).abs().max()):.2e}")
    assert torch.allclose(hy.F.cpu(), ry.F, atol=2e-5, rtol=1e-5)
    assert torch.allclose(hz.F.cpu(), rz.F, atol=2e-5, rtol=1e-5)
    g = torch.randn_like(rz.F)
    rz.F.backward(g)
    hz.F.backward(g.cuda())
    assert torch.allclose(hF.grad.cpu(), rF.grad, atol=2e-5, rtol=1e-4)
    for h, r in ((ha, ra), (hb, rb)):
        scale = float(r.kernel.grad.abs().max())
        assert torch.allclose(h.kernel.grad.cpu(), r.kernel.grad, atol=2e-5 * max(scale, 1.0), rtol=1e-4)
        assert torch.allclose(h.bias.grad.cpu(), r.bias.grad, atol=1e-4, rtol=1e-5)


# ================================================================================================ 4. networks
@pytest.mark.parametrize("ks", [5, 7])
def test_resunet_with_a_cube_stem_matches_oracle(oracle_maps, ks):
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models import MODELS
    from oracle import me_cpu as OME

    torch.manual_seed(0)
    ref = MODELS["ResUNetBN2C"](3, 32, conv1_kernel_size=ks, ME=OME)
    hip = MODELS["ResUNetBN2C"](3, 32, conv1_kernel_size=ks).cuda()
    hip.load_state_dict(ref.state_dict())
    assert hip.conv1.kernel.shape == (ks ** 3, 3, 32)
    coords, feats = batch_scenes([31, 32], grid=24, cin=3)
    out = hip(hip.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
    oout = ref(ref.process_input({"coordinates": coords, "features": feats}))
    assert isinstance(out, ME.SparseTensor) and out.tensor_stride[0] == 1
    n = coords.shape[0]
    assert out.F.shape == (n, 32) == oout.F.shape and torch.equal(out.C.cpu(), oout.C)
    print(f"[bigk] ResUNetBN2C conv1_kernel_size={ks}: out max|diff| {float((out.F.detach().cpu() - oout.F.detach()).abs().max()):.2e}")
    assert torch.allclose(out.F.detach().cpu(), oout.F.detach(), atol=1e-3), (out.F.detach().cpu() - oout.F.detach()).abs().max()
    G = torch.randn(n, 32, generator=torch.Generator().manual_seed(1))
    ((out.F * G.cuda()).sum() / n).backward()
    ((oout.F * G).sum() / n).backward()
    hp, rp = dict(hip.named_parameters()), dict(ref.named_parameters())
    assert hp.keys() == rp.keys()
    rel = {k: float((hp[k].grad.cpu().double() - rp[k].grad.double()).norm() / rp[k].grad.double().norm().clamp_min(1e-12)) for k in hp}
    errs = sorted(rel.values())
    flat_g = torch.cat([hp[k].grad.cpu().double().flatten() for k in hp])
    flat_o = torch.cat([rp[k].grad.double().flatten() for k in hp])
    cos = float(torch.dot(flat_g, flat_o) / (flat_g.norm() * flat_o.norm()))
    print(f"[bigk] ResUNetBN2C conv1_kernel_size={ks}: gradient relative error max {errs[-1]:.3e} "
          f"({max(rel.items(), key=lambda kv: kv[1])[0]}), median {errs[len(errs) // 2]:.3e}, cosine {cos:.6f}, conv1.kernel {rel['conv1.kernel']:.3e}")
    assert max(rel.values()) < 0.15, max(rel.items(), key=lambda kv: kv[1])
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
    assert cos > 0.999
    hb, rb = dict(hip.named_buffers()), dict(ref.named_buffers())
    assert hb.keys() == rb.keys()
    for k in hb:
        assert torch.allclose(hb[k].float().cpu(), rb[k].float(), atol=1e-3, rtol=1e-3), k


def test_fcnn_with_kernel_size_5_matches_float64_restatement():
    from nerf_downstream_amd.co3d_3d.src.models.mink.fcnn import MinkowskiFCNN

    coords, feats = PT.two_clouds()
    torch.manual_seed(3)
    net = MinkowskiFCNN(3, 5, kernel_size=5, embedding_channel=32, channels=(8, 12, 16, 24, 32))
    for m in net.modules():
        if type(m).__name__ == "MinkowskiDropout":
            m.p = 0.0
    net = net.cuda().train()
    assert net.conv1[0].kernel.shape == (125, 8, 12) and net.conv2[0].stride == 2
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.named_parameters()}
    wts = torch.randn(2, 5, generator=torch.Generator().manual_seed(9))
    out = net(net.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
    ref = PT.fcnn_forward(params, coords, feats, kernel_size=5)
    assert out.shape == (2, 5) == ref.shape
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    print(f"[bigk] MinkowskiFCNN kernel_size=5: logits max |err| {err:.3e}")
    assert err <= 1e-3, err
    (out * wts.cuda()).sum().backward()
    (ref * wts.double()).sum().backward()
    hp = dict(net.named_parameters())
    assert all(p.grad is not None for p in hp.values())
    rel = {k: float((hp[k].grad.cpu().double() - params[k].grad).norm() / params[k].grad.norm().clamp_min(1e-12)) for k in hp}
    errs = sorted(rel.values())
    print(f"[bigk] MinkowskiFCNN kernel_size=5: parameter-gradient relative error median {errs[len(errs) // 2]:.3e}, max {errs[-1]:.3e} "
          f"({max(rel, key=rel.get)})")
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
