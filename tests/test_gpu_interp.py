"""-m gpu: trilinear interpolation and splat (csrc/interp.hip) against the float64 restatement of tests/interp_restate.py on the
same inputs.

Maps: the `B4` case of tests/test_gpu_pool.py (voxel counts [257, 0, 1, 130] in [-9, 14]^3, with holes) and one sample of 4,100
voxels in [0, 40)^3, each at tensor strides 1, 2 and 4 (CoordinateManager.stride).  Queries of B4, 697 rows: 4 integer points
that are voxels, 388 uniform in [-10.5, 15.5)^3 over batches 0..3 (batch 1 is empty; some find no corner), 300 inside one
occupied cell (its corner rows receive more than 256 pairs: the workgroup path of mink_interp_segsum), 3 with batch index 7, 2
with a coordinate exactly on a cell face.  4,100 uniform queries for the second map (several workgroups).  Channels 1, 3
(dword lanes), 32 (16-byte lanes), 70 (dword lanes, more column groups than a team's column lanes).

Bounds, u = 2^-24, all computed from the restatement's own terms:
  imap  equal.
  w     4 u absolute: three factors with at most one rounding each in d and in 1 - d, two products, all factors <= 1.
  y     16 u sum_found |x_c| + 2^-149: the weight error gives 4 u |x_c| per term; the product and an eight-term fp32 sum in any
        order give at most 9 u |w x| with w <= 1.
  dx    (n_i + 5) u sum_pairs |dy_q| + 2^-149, n_i the pair count of the row: holds for any summation order.
The splat's features take the dx bound and its gradient the y bound (splat is the transpose)."""
import functools

import pytest
import torch

import interp_restate as IR
import pool_restate as PR
from helpers import misaligned

pytestmark = pytest.mark.gpu

CASES = {"B4": dict(counts=[257, 0, 1, 130], lo=-9, hi=14, seed=11), "one4100": dict(counts=[4100], lo=0, hi=39, seed=12)}
CHANNELS = [1, 3, 32, 70]
STRIDES = [1, 2, 4]
U = IR.EPS32
TINY = 2.0 ** -149


# ------------------------------------------------------------------------------------------------ inputs, built once
@functools.lru_cache(None)
def _coords(case):
    """The voxels of tests/test_gpu_pool.py's cases (the same generator calls)."""
    spec = CASES[case]
    g = torch.Generator().manual_seed(spec["seed"])
    side = spec["hi"] - spec["lo"] + 1
    rows = []
    for b, n in enumerate(spec["counts"]):
        cell = torch.randperm(side ** 3, generator=g)[:n]
        xyz = torch.stack([cell % side, cell // side % side, cell // (side * side)], 1) + spec["lo"]
        rows.append(torch.cat([torch.full((n, 1), b), xyz], 1))
    return torch.cat(rows).long()


@functools.lru_cache(None)
def _level_coords(case, ts):
    """The map at tensor stride ts, restated: floor to the stride, unique, first-occurrence order."""
    return _coords(case) if ts == 1 else PR.strided_coords(_level_coords(case, ts // 2), ts // 2, 2)[0]


@functools.lru_cache(None)
def _queries(case):
    c = _coords(case)
    g = torch.Generator().manual_seed(21)
    if case == "one4100":
        q = torch.cat([torch.zeros(4100, 1), torch.rand(4100, 3, generator=g) * 41 - 0.5], 1)
        return q.float()
    exact = c[[0, 100, 257, 300]].float()  # voxels of batches 0, 0, 2, 3
    uni = torch.cat([torch.randint(0, 4, (388, 1), generator=g).float(), torch.rand(388, 3, generator=g) * 26 - 10.5], 1)
    cell = torch.cat([torch.zeros(300, 1), c[5, 1:].float()[None] + torch.rand(300, 3, generator=g)], 1)
    far = torch.cat([torch.full((3, 1), 7.0), c[:3, 1:].float() + 0.25], 1)
    face = c[[7, 290]].float() + torch.tensor([[0, 0.5, 0, 0.25], [0, 0.75, 0.5, 0]])  # y (then z) exactly on a cell face
    q = torch.cat([exact, uni, cell, far, face]).float()
    assert q.shape == (697, 4)
    return q


@functools.lru_cache(None)
def _ref_map(case, ts):
    return IR.map_weight(_level_coords(case, ts), ts, _queries(case))


@functools.lru_cache(None)
def _randn(rows, C, seed):
    return torch.randn(rows, C, generator=torch.Generator().manual_seed(seed))


_MANAGERS = {}


def _manager(case):
    from nerf_downstream_amd import minkowski as ME

    if case not in _MANAGERS:
        c = _coords(case)
        m = ME.SparseTensor(torch.zeros(c.shape[0], 1, device="cuda"), coordinates=c.int().cuda()).coordinate_manager
        k2 = m.stride(ME.CoordinateMapKey(1), 2)
        m.stride(k2, 2)
        _MANAGERS[case] = m
    return _MANAGERS[case]


def _within(got, ref, bound, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    err = (got.double() - ref).abs()
    live = bound > 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    print(f"[interp] {what}: max err / bound {ratio:.3f} (max |err| {float(err.max()) if err.numel() else 0.0:.2e})")
    assert bool((err <= bound).all()), (what, ratio, float(err.max()))


def _fwd_bound(x, imap):
    return 16 * U * IR.interp_fwd_abs(x, imap) + TINY


def _bwd_bound(dy, imap, n_in):
    s, cnt = IR.interp_bwd_abs(dy, imap, n_in)
    return (cnt[:, None] + 5).double() * U * s + TINY


def _tensor(case, ts, x):
    from nerf_downstream_amd import minkowski as ME

    return ME.SparseTensor(x, ME.CoordinateMapKey(ts), _manager(case))


# ------------------------------------------------------------------------------------------------ map and weights
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("ts", STRIDES)
def test_map_and_weights_equal_the_restatement(case, ts):
    from nerf_downstream_amd import minkowski as ME

    m = _manager(case)
    assert torch.equal(m.get_coordinates(ME.CoordinateMapKey(ts)).cpu().long(), _level_coords(case, ts))
    imap, w = m.interpolation_map_weight(ME.CoordinateMapKey(ts), _queries(case).cuda())
    rimap, rw = _ref_map(case, ts)
    assert imap.dtype == torch.int32 and w.dtype == torch.float32 and imap.shape == w.shape == rimap.shape
    assert torch.equal(imap.cpu().long(), rimap)
    _within(w.cpu(), rw, torch.full_like(rw, 4 * U), f"w {case} ts={ts}")
    if case == "B4":
        absent = (rimap < 0).all(1)
        assert bool(absent[-5:-2].all()) and int(absent.sum()) > 3  # batch index 7, and uniform points that find nothing
        if ts == 1:
            assert bool((rimap[:4, 0] >= 0).all()) and bool((rw[:4, 0] == 1).all())  # the integer points that are voxels
            # a present corner of weight 0 keeps its row: the integer point one step below voxel 3 on x
            v = _coords(case)[3].float() - torch.tensor([0.0, 1, 0, 0])
            i1, w1 = m.interpolation_map_weight(ME.CoordinateMapKey(1), v[None].cuda())
            assert int(i1[0, 1]) == 3 and float(w1[0, 1]) == 0.0 and float(w1[0, 0]) == 1.0
        cnt = torch.bincount(rimap[rimap >= 0], minlength=_level_coords(case, ts).shape[0])
        assert int(cnt.max()) > 256  # a segment longer than four waves


# ------------------------------------------------------------------------------------------------ forward and backward
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("C", CHANNELS)
def test_interpolation_forward_and_backward(case, C):
    q = _queries(case)
    qd = q.cuda()
    dy = _randn(q.shape[0], C, 200 + C)
    for ts in STRIDES:
        n = _level_coords(case, ts).shape[0]
        x = _randn(n, C, 100 + C + ts)
        rimap, rw = _ref_map(case, ts)
        xd = x.clone().cuda().requires_grad_(True)
        y = _tensor(case, ts, xd).features_at_coordinates(qd)
        assert type(y.grad_fn).__name__ == "InterpolationFunctionBackward" and y.shape == (q.shape[0], C)
        y.backward(dy.cuda())
        what = f"{case} C={C} ts={ts}"
        _within(y.detach().cpu(), IR.interp_fwd(x, rimap, rw), _fwd_bound(x, rimap), what + " y")
        _within(xd.grad.cpu(), IR.interp_bwd(dy, rimap, rw, n), _bwd_bound(dy, rimap, n), what + " dx")
        absent = (rimap < 0).all(1)
        assert bool((y.detach().cpu()[absent] == 0).all()), what  # an all-absent query row is exactly zero
        untouched = torch.bincount(rimap[rimap >= 0], minlength=n) == 0
        assert bool((xd.grad.cpu()[untouched] == 0).all()), what


def test_misaligned_rows_take_the_dword_kernels():
    """C % 4 == 0 but x (the gather) and dy (the segmented sum) start 4 bytes off a 16-byte boundary: both must run their
    dword form.  Bounds of test_interpolation_forward_and_backward."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.minkowski import functional as Fn

    case, C = "B4", 32
    q = _queries(case)
    dy = _randn(q.shape[0], C, 250)
    for ts in STRIDES:
        n = _level_coords(case, ts).shape[0]
        x = _randn(n, C, 150 + ts)
        rimap, rw = _ref_map(case, ts)
        imap, w = _manager(case).interpolation_map_weight(ME.CoordinateMapKey(ts), q.cuda())
        flat, xv = misaligned(x, requires_grad=True)
        _, dyv = misaligned(dy)
        assert xv.data_ptr() % 16 == 4 and dyv.data_ptr() % 16 == 4
        y = Fn.InterpolationFunction.apply(xv, imap, w, Fn.lazy_csr(imap, n))
        seen = []
        y.register_hook(lambda g: seen.append(g.data_ptr()))
        y.backward(dyv)
        assert seen == [dyv.data_ptr()]  # the segmented sum was handed the misaligned rows themselves
        what = f"misaligned {case} C={C} ts={ts}"
        _within(y.detach().cpu(), IR.interp_fwd(x, rimap, rw), _fwd_bound(x, rimap), what + " y")
        _within(flat.grad[1:1 + n * C].view(n, C).cpu(), IR.interp_bwd(dy, rimap, rw, n), _bwd_bound(dy, rimap, n), what + " dx")


def test_interpolate_and_the_module_take_the_same_path():
    from nerf_downstream_amd import minkowski as ME

    case, C, ts = "B4", 32, 2
    q = _queries(case)
    x = _randn(_level_coords(case, ts).shape[0], C, 300).cuda()
    st = _tensor(case, ts, x)
    y = st.features_at_coordinates(q.cuda())
    field = ME.TensorField(features=torch.zeros(q.shape[0] - 3, 1, device="cuda"), coordinates=torch.cat([q[:-5], q[-2:]]).cuda())
    out = st.interpolate(field)  # (a field of its own: not the one the tensor was quantised from; batch 7 left out)
    assert isinstance(out, ME.TensorField) and out.coordinate_manager is field.coordinate_manager and out.C is field.C
    assert torch.equal(out.F, torch.cat([y[:-5], y[-2:]]))
    assert torch.equal(ME.MinkowskiInterpolation()(st, q.cuda()), y)
    # ME's kernel-map lists: the found entries in (query, corner) order
    rimap, rw = _ref_map(case, ts)
    o, in_map, out_map, weights = ME.MinkowskiInterpolation(return_kernel_map=True)(st, q.cuda())
    assert torch.equal(o, y)
    found = torch.nonzero(rimap.reshape(-1) >= 0).reshape(-1)
    assert torch.equal(in_map.cpu().long(), rimap.reshape(-1)[found]) and torch.equal(out_map.cpu().long(), found // 8)
    imap, w = _manager(case).interpolation_map_weight(ME.CoordinateMapKey(ts), q.cuda())
    assert torch.equal(weights, w.reshape(-1)[found.cuda()]) and weights.shape == in_map.shape == out_map.shape


@pytest.mark.parametrize("case,C", [("B4", 70), ("B4", 32), ("one4100", 3)])
def test_two_backward_runs_are_bitwise_equal(case, C):
    q = _queries(case).cuda()
    dy = _randn(q.shape[0], C, 400 + C).cuda()
    for ts in STRIDES:
        x = _randn(_level_coords(case, ts).shape[0], C, 500 + C)
        grads = []
        for _ in range(2):
            xd = x.clone().cuda().requires_grad_(True)
            _tensor(case, ts, xd).features_at_coordinates(q).backward(dy)
            grads.append(xd.grad)
        assert torch.equal(grads[0], grads[1]), (case, C, ts)


def test_out_of_range_and_nan_queries_are_refused():
    from nerf_downstream_amd import minkowski as ME

    st = _tensor("B4", 1, _randn(_coords("B4").shape[0], 3, 600).cuda())
    for bad in ([0, 32767.5, 0, 0], [0, 0, float("nan"), 0], [0, 0, 0, float("inf")], [0, -32768.5, 0, 0]):
        with pytest.raises(ValueError):
            st.features_at_coordinates(torch.tensor([[0, 1.5, 2.5, 3.5], bad]).float().cuda())
    # a field whose floor map is legal (32767) but whose upper corners are not
    field = ME.TensorField(features=torch.zeros(2, 1, device="cuda"), coordinates=torch.tensor([[0, 1.5, 2.5, 3.5], [0, 1, 32767.5, 1]]).float().cuda())
    with pytest.raises(ValueError):
        field.splat()


# ------------------------------------------------------------------------------------------------ splat
@functools.lru_cache(None)
def _field():
    g = torch.Generator().manual_seed(31)
    xyz = torch.rand(257, 3, generator=g) * 23 - 9
    xyz[40:50] = xyz[:10]  # duplicates
    xyz[60:70] = torch.floor(xyz[60:70])  # integer points
    xyz[70:80, 1] = torch.floor(xyz[70:80, 1])  # one coordinate on a face
    xyz[100:180] = xyz[100].floor()[None] + torch.rand(80, 3, generator=g)  # 80 points of one cell: long segments
    b = torch.cat([torch.zeros(200, 1), torch.ones(57, 1)])
    return torch.cat([b, xyz], 1).float()


@pytest.mark.parametrize("C", CHANNELS)
def test_splat_against_the_restatement(C):
    from nerf_downstream_amd import minkowski as ME

    fc = _field()
    coords, rimap, rw = IR.splat_coords(fc)
    nv = coords.shape[0]
    F, g = _randn(257, C, 700 + C), _randn(nv, C, 800 + C)
    Fd = F.clone().cuda().requires_grad_(True)
    st = ME.TensorField(features=Fd, coordinates=fc.cuda()).splat()
    assert isinstance(st, ME.SparseTensor) and st.tensor_stride == [1, 1, 1]
    assert torch.equal(st.C.cpu().long(), coords)  # first-occurrence order
    assert type(st.F.grad_fn).__name__ == "SplatFunctionBackward"
    st.F.backward(g.cuda())
    _within(st.F.detach().cpu(), IR.splat_fwd(F, rimap, rw, nv), _bwd_bound(F, rimap, nv), f"splat C={C} F_s")
    _within(Fd.grad.cpu(), IR.interp_fwd(g, rimap, rw), _fwd_bound(g, rimap), f"splat C={C} dF")
    again = ME.TensorField(features=F.cuda(), coordinates=fc.cuda()).splat()
    assert torch.equal(again.F, st.F.detach())  # bitwise reproducible


def test_strided_levels_and_pooling_on_the_splat_manager_read_back_at_the_field():
    from nerf_downstream_amd import minkowski as ME

    C = 32
    fc = _field()
    coords, _, _ = IR.splat_coords(fc)
    field = ME.TensorField(features=_randn(257, C, 900).cuda(), coordinates=fc.cuda())
    st = field.splat()
    m = st.coordinate_manager
    assert m is not field.coordinate_manager  # the field's manager holds its floor map at stride 1 already
    k2 = m.stride(st.coordinate_map_key, 2)
    c2 = PR.strided_coords(coords, 1, 2)[0]
    assert torch.equal(m.get_coordinates(k2).cpu().long(), c2)
    pooled = ME.MinkowskiMaxPooling(3, 2, dimension=3)(st)
    assert pooled.coordinate_map_key == k2 and pooled.coordinate_manager is m
    out2, table = PR.pooling_maps(coords, 1, 3, 2)
    assert torch.equal(out2, c2)
    assert torch.equal(pooled.F.cpu().double(), PR.max_fwd(st.F.cpu(), table)[0])  # a maximum selects an input: bitwise
    back = pooled.interpolate(field)
    assert back.coordinate_manager is field.coordinate_manager and back.F.shape == (257, C)
    rimap, rw = IR.map_weight(c2, 2, fc)
    x = pooled.F.cpu()
    _within(back.F.cpu(), IR.interp_fwd(x, rimap, rw), _fwd_bound(x, rimap), "splat -> max pool (3, 2) -> interpolate")
    # the tensor-stride-1 splat read back at its own field finds all eight corners of every point
    imap, w = m.interpolation_map_weight(st.coordinate_map_key, fc.cuda())
    assert bool((imap >= 0).all()) and float((w.sum(1) - 1).abs().max()) <= 8 * U


# ------------------------------------------------------------------------------------------------ PerlinNoise
def test_perlin_noise_against_the_float64_recipe():
    """One octave at a time on 500 points in [-20, 28)^3 with the node noise supplied as a function of the node's coordinates:
    out = coords + std * interp(smooth(noise)) against the same recipe in float64 (lattice = splat coordinates of coords / q,
    smooth = a 3 -> 3 channel 3^3 convolution with EVERY entry of its [27, 3, 3] kernel 1/27: each output channel is the sum
    over the 27-neighbourhood, absent nodes counting as zero, AND over the three input channels, divided by 27 -- the three
    output channels are equal), within std x (16 u sum_found |s_c| + 2^-149), s = the float64 smoothed lattice values.  The
    bound is the interpolation's own: the fp32 rounding of the 81-term smoothing sum and of the final multiply-add (u |out|,
    |out| < 32 here) are not terms of it, so the printed ratio is the figure to watch if this ever fails."""
    from nerf_downstream_amd.co3d_3d.src.data.perlin import PerlinNoise

    g = torch.Generator().manual_seed(41)
    coords = (torch.rand(500, 3, generator=g) * 48 - 20).float()
    table = torch.randn(4096, 3, generator=g)

    def node_noise(C):
        c = C.cpu().long()
        return table[((c[:, 1] * 73 + c[:, 2] * 179 + c[:, 3] * 283) % 4096 + 4096) % 4096]

    p = PerlinNoise(application_ratio=1.0)
    assert list(map(tuple, p.noise_params)) == [(4, 4), (16, 16)]
    for q, std in p.noise_params:
        out = p.perlin_noise(coords.cuda(), q, std, node_noise=node_noise)
        assert out.is_cuda and out.shape == coords.shape and out.dtype == torch.float32
        bq = torch.cat([torch.zeros(500, 1), coords / q], 1)  # (a division by a power of two: exact on either side)
        nodes, rimap, rw = IR.splat_coords(bq)
        s = PR.sum_fwd(node_noise(nodes).double(), PR.window_table(nodes, nodes, 1, 3)).sum(1, keepdim=True).expand(-1, 3) / 27
        ref = coords.double() + std * IR.interp_fwd(s, rimap, rw)
        _within(out.cpu(), ref, std * _fwd_bound(s, rimap), f"PerlinNoise q={q} std={std}")
        assert float((out.cpu() - coords).abs().max()) > 0.01 * std  # it moved the points
    # the whole transform is the octaves chained, and never applied it returns its input
    both = p(coords.cuda(), node_noise=node_noise)
    step = coords.cuda()
    for q, std in p.noise_params:
        step = p.perlin_noise(step, q, std, node_noise=node_noise)
    assert torch.equal(both, step)
    cd = coords.cuda()
    assert PerlinNoise(application_ratio=0)(cd) is cd
    # drawn on the device from a generator: reproducible from its seed
    a = p(cd, generator=torch.Generator(device="cuda").manual_seed(5))
    b = p(cd, generator=torch.Generator(device="cuda").manual_seed(5))
    assert torch.equal(a, b) and not torch.equal(a, cd)
