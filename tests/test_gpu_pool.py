"""-m gpu: the sparse pooling family (csrc/pool.hip) against the float64 restatement of tests/pool_restate.py on the same inputs.

Two inputs: a batch of four samples with [257, 0, 1, 130] voxels at coordinates in [-9, 14]^3 (negative coordinates, an empty
sample, a one-voxel sample, one sample longer than a multiple of a wave) and one sample of 4,100 voxels in [0, 40)^3 (the
segmented reductions then span several workgroups); channels 1, 3 (dword lanes), 32 (16-byte lanes) and 70 (dword lanes, more
column groups than a row lane holds); features from a normal distribution, so ties have probability zero (they have a test of
their own on {0, 1} inputs).

Bounds.  A maximum selects an input and the global-max gradient copies one: bitwise.  An fp32 sum of at most K = 27 terms is
within 27 x 2^-24 x sum |terms| of the exact one; the average adds one division per term or per sum: (K + 1) x 2^-24 x
sum |terms|, the terms taken after the division.  The global sum accumulates in double and rounds once: 2^-24 |ref| + 2^-149.
Every bound is computed from the restatement's own terms."""
import functools

import pytest
import torch

import layerwise as LW
import pool_restate as PR
from helpers import misaligned

pytestmark = pytest.mark.gpu

CASES = {"B4": dict(counts=[257, 0, 1, 130], lo=-9, hi=14, seed=11), "one4100": dict(counts=[4100], lo=0, hi=39, seed=12)}
CHANNELS = [1, 3, 32, 70]
KS = [(2, 2), (3, 2), (3, 1)]
K = 27
EPS = PR.EPS32
TINY = 2.0 ** -149


# ------------------------------------------------------------------------------------------------ inputs, built once
@functools.lru_cache(None)
def _coords(case):
    spec = CASES[case]
    g = torch.Generator().manual_seed(spec["seed"])
    side = spec["hi"] - spec["lo"] + 1
    rows = []
    for b, n in enumerate(spec["counts"]):
        cell = torch.randperm(side ** 3, generator=g)[:n]
        xyz = torch.stack([cell % side, cell // side % side, cell // (side * side)], 1) + spec["lo"]
        rows.append(torch.cat([torch.full((n, 1), b), xyz], 1))
    return torch.cat(rows).long()


def _offsets(case):
    return PR.offsets_of(_coords(case), len(CASES[case]["counts"]))


@functools.lru_cache(None)
def _ref_maps(case, k, s):
    return PR.pooling_maps(_coords(case), 1, k, s)


@functools.lru_cache(None)
def _randn(rows, C, seed):
    return torch.randn(rows, C, generator=torch.Generator().manual_seed(seed))


_MANAGERS = {}


def _manager(case):
    from nerf_downstream_amd import minkowski as ME

    if case not in _MANAGERS:
        c = _coords(case)
        st = ME.SparseTensor(torch.zeros(c.shape[0], 1, device="cuda"), coordinates=c.int().cuda())
        _MANAGERS[case] = st.coordinate_manager
    return _MANAGERS[case]


def _tables(case, k, s):
    from nerf_downstream_amd import minkowski as ME

    m = _manager(case)
    out_key = m.stride(ME.CoordinateMapKey(1), s)
    nbr, nbr_t = m.kernel_table(ME.CoordinateMapKey(1), out_key, k, 1, transposed=True)
    return m, out_key, nbr, nbr_t


def _run(fn, x, dy, *args):
    """One forward + backward of an autograd function -> (y, second output or None, dx) on the host."""
    xd = x.clone().cuda().requires_grad_(True)
    out = fn.apply(xd, *args)
    y, aux = out if isinstance(out, tuple) else (out, None)
    y.backward(dy.cuda())
    return y.detach().cpu(), None if aux is None else aux.cpu(), xd.grad.cpu()


def _within(got, ref, bound, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"[pool] {what}: max err / bound {ratio:.3f} (max |err| {float(err.max()) if err.numel() else 0.0:.2e})")
    assert bool((err <= bound).all()), (what, ratio, float(err.max()))


def _fns():
    from nerf_downstream_amd.minkowski import functional as Fn

    return Fn


# ------------------------------------------------------------------------------------------------ maps
@pytest.mark.parametrize("case", list(CASES))
def test_maps_and_window_counts_equal_the_restatement(case):
    for k, s in KS:
        m, out_key, nbr, nbr_t = _tables(case, k, s)
        ref_out, ref_table = _ref_maps(case, k, s)
        assert torch.equal(m.get_coordinates(out_key).cpu().long(), ref_out), (k, s)  # first-occurrence order on both sides
        t = nbr.cpu().long()
        assert torch.equal((t >= 0).sum(1), PR.counts(ref_table)), (k, s)
        assert torch.equal(t, ref_table), (k, s)
        assert int(PR.counts(ref_table).min()) >= 1
        # the transposed table holds exactly the same pairs: nbr_t[i][j] = o iff nbr[o][j] = i
        tt = nbr_t.cpu().long()
        o, j = torch.nonzero(t >= 0, as_tuple=True)
        assert torch.equal(tt[t[o, j], j], o) and int((tt >= 0).sum()) == o.numel(), (k, s)


# ------------------------------------------------------------------------------------------------ local pools
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C", CHANNELS)
def test_local_max_pooling(case, C):
    Fn = _fns()
    n = _coords(case).shape[0]
    x = _randn(n, C, 100 + C)
    for k, s in KS:
        _, _, nbr, nbr_t = _tables(case, k, s)
        _, table = _ref_maps(case, k, s)
        dy = _randn(table.shape[0], C, 200 + C)
        y, arg, dx = _run(Fn.SparseMaxPoolFunction, x, dy, nbr, nbr_t)
        ry, rarg = PR.max_fwd(x, table)
        what = f"max {case} C={C} k={k} s={s}"
        assert torch.equal(y, ry.float()) and torch.equal(y.double(), ry), what  # a maximum selects an input: bitwise
        assert torch.equal(arg.long(), rarg), what
        _within(dx, PR.max_bwd(dy, rarg, table, n), K * EPS * PR.max_bwd_abs(dy, rarg, table, n), what + " dx")


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C", CHANNELS)
def test_local_avg_and_overlapping_sum_pooling(case, C):
    Fn = _fns()
    n = _coords(case).shape[0]
    x = _randn(n, C, 300 + C)
    for k, s in KS:
        _, _, nbr, nbr_t = _tables(case, k, s)
        _, table = _ref_maps(case, k, s)
        dy = _randn(table.shape[0], C, 400 + C)
        for fn, avg, fwd, bwd in ((Fn.AvgPoolFunction, True, PR.avg_fwd, PR.avg_bwd), (Fn.OverlapSumPoolFunction, False, PR.sum_fwd, PR.sum_bwd)):
            y, cnt, dx = _run(fn, x, dy, nbr, nbr_t)
            what = f"{'avg' if avg else 'sum'} {case} C={C} k={k} s={s}"
            assert cnt.dtype == torch.int32 and torch.equal(cnt.long(), PR.counts(table)), what  # cnt is exact
            _within(y, fwd(x, table), (K + 1) * EPS * PR.sum_fwd_abs(x, table, avg), what + " y")
            _within(dx, bwd(dy, table, n), (K + 1) * EPS * PR.sum_bwd_abs(dy, table, n, avg), what + " dx")


# ------------------------------------------------------------------------------------------------ global pools
def _boff(case):
    from nerf_downstream_amd import minkowski as ME

    boff = _manager(case).batch_offsets(ME.CoordinateMapKey(1))
    assert boff.cpu().tolist() == _offsets(case)
    return boff


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C", CHANNELS)
def test_global_max_and_sum_pooling(case, C):
    Fn = _fns()
    off, boff = _offsets(case), _boff(case)
    n, B = off[-1], len(off) - 1
    x, dy = _randn(n, C, 500 + C), _randn(B, C, 600 + C)
    y, arg, dx = _run(Fn.GlobalMaxPoolFunction, x, dy, boff)
    ry, rarg = PR.global_max_fwd(x, off)
    what = f"global max {case} C={C}"
    assert torch.equal(y.double(), ry), what
    assert arg.dtype == torch.int32 and torch.equal(arg.long(), rarg), what
    assert torch.equal(dx.double(), PR.global_max_bwd(dy, rarg, n)), what  # every dx entry is one dy entry or 0
    for b in range(B):
        if off[b + 1] == off[b]:
            assert bool((y[b] == 0).all()) and bool((arg[b] == -1).all()), what  # an empty sample: 0 and arg = -1
    y, _, dx = _run(Fn.GlobalSumPoolFunction, x, dy, boff)
    ref = PR.global_sum_fwd(x, off)
    _within(y, ref, EPS * ref.abs() + TINY, f"global sum {case} C={C} y")
    assert torch.equal(dx.double(), PR.global_sum_bwd(dy, off)), f"global sum {case} C={C} dx"


# ------------------------------------------------------------------------------------------------ alignment fallback
def test_misaligned_features_take_the_dword_kernels():
    """C % 4 == 0 but x starts 4 bytes off a 16-byte boundary: the host side must launch the dword form of every kernel that
    reads x (a 16-byte access there faults or reads shifted columns).  Restatements and bounds of the aligned tests above."""
    Fn = _fns()
    case, C, (k, s) = "B4", 8, (3, 2)
    off, boff = _offsets(case), _boff(case)
    n, B = off[-1], len(off) - 1
    _, _, nbr, nbr_t = _tables(case, k, s)
    _, table = _ref_maps(case, k, s)
    x, dy, dyb = _randn(n, C, 1400), _randn(table.shape[0], C, 1401), _randn(B, C, 1402)

    def run(fn, g, *args):
        flat, xv = misaligned(x, requires_grad=True)
        assert xv.data_ptr() % 16 == 4
        out = fn.apply(xv, *args)
        y, aux = out if isinstance(out, tuple) else (out, None)
        y.backward(g.cuda())
        return y.detach().cpu(), None if aux is None else aux.cpu(), flat.grad[1:1 + n * C].view(n, C).cpu()

    y, arg, dx = run(Fn.SparseMaxPoolFunction, dy, nbr, nbr_t)
    ry, rarg = PR.max_fwd(x, table)
    assert torch.equal(y.double(), ry) and torch.equal(arg.long(), rarg)
    _within(dx, PR.max_bwd(dy, rarg, table, n), K * EPS * PR.max_bwd_abs(dy, rarg, table, n), "misaligned max dx")
    y, cnt, dx = run(Fn.AvgPoolFunction, dy, nbr, nbr_t)
    assert torch.equal(cnt.long(), PR.counts(table))
    _within(y, PR.avg_fwd(x, table), (K + 1) * EPS * PR.sum_fwd_abs(x, table, True), "misaligned avg y")
    _within(dx, PR.avg_bwd(dy, table, n), (K + 1) * EPS * PR.sum_bwd_abs(dy, table, n, True), "misaligned avg dx")
    y, arg, dx = run(Fn.GlobalMaxPoolFunction, dyb, boff)
    ry, rarg = PR.global_max_fwd(x, off)
    assert torch.equal(y.double(), ry) and torch.equal(arg.long(), rarg)
    assert torch.equal(dx.double(), PR.global_max_bwd(dyb, rarg, n))
    y, _, dx = run(Fn.GlobalSumPoolFunction, dyb, boff)
    ref = PR.global_sum_fwd(x, off)
    _within(y, ref, EPS * ref.abs() + TINY, "misaligned global sum y")
    assert torch.equal(dx.double(), PR.global_sum_bwd(dyb, off))


# ------------------------------------------------------------------------------------------------ ties
@pytest.mark.parametrize("C", [3, 32])
def test_ties_go_to_the_lowest_offset_and_the_lowest_row(C):
    """Inputs quantised to {0, 1}: most windows and every sample hold several rows attaining the maximum.  Only invariants."""
    Fn = _fns()
    case = "B4"
    n = _coords(case).shape[0]
    g = torch.Generator().manual_seed(700 + C)
    x = (torch.rand(n, C, generator=g) > 0.5).float()
    for k, s in KS:
        _, _, nbr, nbr_t = _tables(case, k, s)
        _, table = _ref_maps(case, k, s)
        dy = torch.rand(table.shape[0], C, generator=g) + 0.5  # non-zero: where a gradient lands is visible
        y, arg, dx = _run(Fn.SparseMaxPoolFunction, x, dy, nbr, nbr_t)
        ry, rarg = PR.max_fwd(x, table)
        assert torch.equal(y.double(), ry)  # the forward value is exact
        a = arg.long()
        cols = torch.arange(C)[None, :].expand_as(a)
        assert bool((a >= 0).all()) and bool((table[:, :, None] == a[:, None, :]).any(1).all())  # one row of the window ...
        assert torch.equal(x[a, cols], y)  # ... that attains the maximum ...
        assert torch.equal(a, rarg)  # ... and is the one at the lowest kernel offset
        assert int((PR.max_fwd(x, table)[1] != PR.max_fwd(x + 0.0, table.flip(1))[1]).sum()) > 0  # (the ties are there: order matters)
        ref_dx = PR.max_bwd(dy, a, table, n)
        bound = K * EPS * PR.max_bwd_abs(dy, a, table, n)
        _within(dx, ref_dx, bound, f"ties max C={C} k={k} s={s} dx")
        assert bool(((dx.double().sum(0) - dy.double().sum(0)).abs() <= bound.sum(0)).all())  # sum(dx) == sum(dy) per channel
    off, boff = _offsets(case), _boff(case)
    B = len(off) - 1
    dy = torch.rand(B, C, generator=g) + 0.5
    y, arg, dx = _run(Fn.GlobalMaxPoolFunction, x, dy, boff)
    ry, rarg = PR.global_max_fwd(x, off)
    assert torch.equal(y.double(), ry) and torch.equal(arg.long(), rarg)
    for b in range(B):
        seg = dx[off[b]:off[b + 1]]
        if seg.shape[0] == 0:
            continue
        assert bool(((seg != 0).sum(0) == 1).all())  # exactly one row per (sample, channel) ...
        hit = (seg != 0).float().argmax(0)
        attains = x[off[b]:off[b + 1]] == y[b][None]
        lowest = torch.where(attains, torch.arange(seg.shape[0])[:, None], seg.shape[0]).min(0).values
        assert torch.equal(hit, lowest)  # ... the lowest one attaining the maximum
        assert torch.equal(seg.sum(0), dy[b])  # (one non-zero entry per column: the sum is that entry)
    live = torch.tensor([off[b + 1] > off[b] for b in range(B)])
    assert bool(((dx.double().sum(0) - dy[live].double().sum(0)).abs() <= K * EPS * dy[live].double().abs().sum(0)).all())


# ------------------------------------------------------------------------------------------------ reproducibility
@pytest.mark.parametrize("case,C", [("B4", 70), ("one4100", 32)])
def test_two_runs_are_bitwise_equal(case, C):
    Fn = _fns()
    n = _coords(case).shape[0]
    x = _randn(n, C, 800 + C)
    boff = _boff(case)

    def same(a, b):
        return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))

    for k, s in KS:
        _, _, nbr, nbr_t = _tables(case, k, s)
        dy = _randn(nbr.shape[0], C, 900 + C)
        for fn in (Fn.SparseMaxPoolFunction, Fn.AvgPoolFunction, Fn.OverlapSumPoolFunction):
            assert same(_run(fn, x, dy, nbr, nbr_t), _run(fn, x, dy, nbr, nbr_t)), (fn.__name__, k, s)
    dy = _randn(boff.numel() - 1, C, 950 + C)
    for fn in (Fn.GlobalMaxPoolFunction, Fn.GlobalSumPoolFunction):
        assert same(_run(fn, x, dy, boff), _run(fn, x, dy, boff)), fn.__name__


# ------------------------------------------------------------------------------------------------ no host synchronisation
@pytest.mark.parametrize("C", [3, 32])
def test_global_pool_modules_match_float64_without_host_sync(C):
    from nerf_downstream_amd import minkowski as ME

    case = "B4"
    off = _offsets(case)
    n, B = off[-1], len(off) - 1
    x, dy = _randn(n, C, 1000 + C), _randn(B, C, 1100 + C)
    m = _manager(case)
    m.batch_offsets(ME.CoordinateMapKey(1))  # the offsets exist (their first build reads the sortedness flag back)
    gmax, gsum = ME.MinkowskiGlobalMaxPooling(), ME.MinkowskiGlobalSumPooling()
    xa, xb = (x.clone().cuda().requires_grad_(True) for _ in range(2))
    sa, sb = (ME.SparseTensor(t, ME.CoordinateMapKey(1), m) for t in (xa, xb))
    gmax(sa), gsum(sb)  # (first calls: scratch buffers are allocated)
    dyd = dy.cuda()  # (a copy from pageable host memory synchronises: made before the guarded region)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        oa, ob = gmax(sa), gsum(sb)
        oa.F.backward(dyd)
        ob.F.backward(dyd)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    for o in (oa, ob):
        assert o.coordinate_map_key == ME.CoordinateMapKey(0) and o.coordinate_manager is m and o.F.shape == (B, C)
    assert o.C.cpu().tolist() == [[b, 0, 0, 0] for b in range(B)]  # row b is batch index b
    ry, rarg = PR.global_max_fwd(x, off)
    assert torch.equal(oa.F.detach().cpu().double(), ry)
    assert torch.equal(xa.grad.cpu().double(), PR.global_max_bwd(dy, rarg, n))
    ref = PR.global_sum_fwd(x, off)
    _within(ob.F.detach().cpu(), ref, EPS * ref.abs() + TINY, f"global sum module C={C}")
    assert torch.equal(xb.grad.cpu().double(), PR.global_sum_bwd(dy, off))


# ------------------------------------------------------------------------------------------------ modules
def test_local_pool_modules_and_sum_pooling_dispatch():
    """MinkowskiSumPooling(3, 2), the newly legal case, against the restatement; MinkowskiSumPooling(2, 2) still runs
    mink_pool_sum_fwd (bitwise equal to a direct SumPoolFunction call); stride 1 pools onto the input map."""
    from nerf_downstream_amd import minkowski as ME

    Fn = _fns()
    case, C = "B4", 32
    m = _manager(case)
    n = _coords(case).shape[0]
    x = _randn(n, C, 1200)
    key1 = ME.CoordinateMapKey(1)
    # (3, 2): overlapping windows
    _, table = _ref_maps(case, 3, 2)
    dy = _randn(table.shape[0], C, 1201)
    xd = x.clone().cuda().requires_grad_(True)
    out = ME.MinkowskiSumPooling(3, 2, dimension=3)(ME.SparseTensor(xd, key1, m))
    assert out.coordinate_map_key == ME.CoordinateMapKey(2) and type(out.F.grad_fn).__name__ == "OverlapSumPoolFunctionBackward"
    out.F.backward(dy.cuda())
    _within(out.F.detach().cpu(), PR.sum_fwd(x, table), (K + 1) * EPS * PR.sum_fwd_abs(x, table), "MinkowskiSumPooling(3, 2) y")
    _within(xd.grad.cpu(), PR.sum_bwd(dy, table, n), (K + 1) * EPS * PR.sum_bwd_abs(dy, table, n), "MinkowskiSumPooling(3, 2) dx")
    # (2, 2): the non-overlapping kernels, as before
    xd = x.clone().cuda().requires_grad_(True)
    out = ME.MinkowskiSumPooling(2, 2, dimension=3)(ME.SparseTensor(xd, key1, m))
    assert type(out.F.grad_fn).__name__ == "SumPoolFunctionBackward"
    nbr8, _ = m.kernel_table(key1, ME.CoordinateMapKey(2), 2, 1)
    direct = Fn.SumPoolFunction.apply(x.cuda(), nbr8, m.stride_map(key1, ME.CoordinateMapKey(2)))
    assert torch.equal(out.F.detach(), direct)
    _, table8 = _ref_maps(case, 2, 2)
    _within(direct.cpu(), PR.sum_fwd(x, table8), 8 * EPS * PR.sum_fwd_abs(x, table8), "MinkowskiSumPooling(2, 2) y")
    out.F.backward(dy.cuda())
    assert torch.equal(xd.grad.cpu().double(), PR.sum_bwd(dy, table8, n))  # one window per row: a copy
    # avg / max through the modules, stride 1 onto the input map
    _, table1 = _ref_maps(case, 3, 1)
    for cls, ref in ((ME.MinkowskiAvgPooling, PR.avg_fwd(x, table1)), (ME.MinkowskiMaxPooling, PR.max_fwd(x, table1)[0])):
        o = cls(3, 1, dimension=3)(ME.SparseTensor(x.cuda(), key1, m))
        assert o.coordinate_map_key == key1 and o.coordinate_manager is m
        _within(o.F.cpu(), ref, (K + 1) * EPS * PR.sum_fwd_abs(x, table1, True), cls.__name__ + "(3, 1)")


def test_modules_end_to_end_against_float64(oracle_maps):
    """conv(3 -> 32, k=3) -> MinkowskiMaxPooling(3, 2) -> MinkowskiAvgPooling(2, 2) -> cat(global max, global avg) -> linear,
    against the same chain in float64: the oracle's convolution, this file's restatement of the pools, under the HIP run's own
    max decisions (teacher forcing, as tests/layerwise.py does for ReLU).  Logits within 1e-3; parameter gradients (and the
    input gradient) within layerwise.check_conv's bounds, as tests/test_gpu_layerwise.py holds them."""
    from nerf_downstream_amd import minkowski as ME
    from oracle import me_cpu as OME

    Fn = _fns()
    case, ncls = "B4", 10
    coords, off = _coords(case), _offsets(case)
    n, B = off[-1], len(off) - 1
    feats, gl = _randn(n, 3, 1300), _randn(B, ncls, 1301)
    torch.manual_seed(0)
    conv = ME.MinkowskiConvolution(3, 32, kernel_size=3, dimension=3).cuda()
    lin = ME.MinkowskiLinear(64, ncls).cuda()
    xs = feats.clone().cuda().requires_grad_(True)
    st = ME.SparseTensor(xs, coordinates=coords.int().cuda())
    m = st.coordinate_manager
    h0 = conv(st)
    h1 = ME.MinkowskiMaxPooling(3, 2, dimension=3)(h0)
    h2 = ME.MinkowskiAvgPooling(2, 2, dimension=3)(h1)
    head = ME.cat(ME.MinkowskiGlobalMaxPooling()(h2), ME.MinkowskiGlobalAvgPooling()(h2))  # the head of the reference's fcnn
    out = lin(head)
    assert h1.tensor_stride == [2, 2, 2] and h2.tensor_stride == [4, 4, 4]
    assert head.coordinate_map_key == ME.CoordinateMapKey(0) and head.F.shape == (B, 64) and out.F.shape == (B, ncls)
    out.F.backward(gl.cuda())
    # the HIP run's max decisions: the same kernels on the same stored inputs
    nbr, nbr_t = m.kernel_table(ME.CoordinateMapKey(1), ME.CoordinateMapKey(2), 3, 1, transposed=True)
    y1, arg1 = Fn.SparseMaxPoolFunction.apply(h0.F.detach(), nbr, nbr_t)
    y3, arg3 = Fn.GlobalMaxPoolFunction.apply(h2.F.detach(), m.batch_offsets(ME.CoordinateMapKey(4)))
    assert torch.equal(y1, h1.F.detach()) and torch.equal(y3, head.F.detach()[:, :32])
    arg1, arg3 = arg1.cpu().long(), arg3.cpu().long()
    # float64
    oconv = OME.MinkowskiConvolution(3, 32, kernel_size=3, dimension=3).double()
    with torch.no_grad():
        oconv.kernel.copy_(conv.kernel.detach().cpu().double())
    W = lin.linear.weight.detach().cpu().double().requires_grad_(True)
    bias = lin.linear.bias.detach().cpu().double().requires_grad_(True)
    ox = feats.double().requires_grad_(True)
    r0 = oconv(OME.TensorField(coordinates=coords.float(), features=ox).sparse()).F
    _, t1 = _ref_maps(case, 3, 2)
    assert bool((t1[:, :, None] == arg1[:, None, :]).any(1).all())  # every decision is a row of its window
    r1 = PR.max_fwd_forced(r0, arg1)
    c2 = PR.strided_coords(coords, 1, 2)[0]
    c4, t2 = PR.pooling_maps(c2, 2, 2, 2)
    assert torch.equal(h2.C.cpu().long(), c4)
    r2 = PR.avg_fwd(r1, t2)
    off4 = PR.offsets_of(c4, B)
    r3 = torch.cat([PR.max_fwd_forced(r2, arg3), PR.global_avg_fwd(r2, off4)], 1)
    rout = r3 @ W.t() + bias
    rout.backward(gl.double())
    err = float((out.F.detach().cpu().double() - rout.detach()).abs().max())
    print(f"[pool chain] logits: max |err| {err:.2e} against float64 (max |logit| {float(rout.detach().abs().max()):.2f})")
    assert err <= 1e-3
    # the forced decisions are float64's own except where two candidates are equal to fp32 rounding
    own = PR.max_fwd(r0.detach(), t1)[1]
    flips = own != arg1
    cols = torch.arange(32)[None, :].expand_as(arg1)
    gap = (r0.detach()[own, cols] - r0.detach()[arg1, cols]).abs()
    assert not bool(flips.any()) or float(gap[flips].max()) <= 1e-5 * float(r0.detach().abs().max())
    recs = LW.check_conv("chain", "conv wgrad", conv.kernel.grad.cpu(), oconv.kernel.grad)
    recs += LW.check_conv("chain", "linear weight", lin.linear.weight.grad.cpu(), W.grad)
    recs += LW.check_conv("chain", "linear bias", lin.linear.bias.grad.cpu(), bias.grad)
    recs += LW.check_conv("chain", "input gradient", xs.grad.cpu(), ox.grad)
    for r in recs:
        print("[pool chain] " + r.line())
    assert all(r.ok for r in recs), [r.line() for r in recs if not r.ok]
