"""CPU: tests/interp_restate.py, the float64 restatement the interpolation / splat kernels are held to, pinned by itself:
partition of unity, exactness on linear functions, a dense torch.nn.functional.grid_sample as an independent implementation,
adjointness of forward and backward, floor (not truncation) below zero -- and the host logic of PerlinNoise."""
import inspect

import torch

import interp_restate as IR

F64 = torch.float64


def _lattice(nx, ny, nz, lo=0, ts=1, b=0):
    """Every (b, x, y, z) of a full box, x fastest; coordinates lo + ts * index."""
    z, y, x = torch.meshgrid(torch.arange(nz), torch.arange(ny), torch.arange(nx), indexing="ij")
    xyz = torch.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1) * ts + lo
    return torch.cat([torch.full((xyz.shape[0], 1), b), xyz], 1).long()


def _queries(n, lo, hi, seed, b=0):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 3, generator=g) * (hi - lo) + lo
    return torch.cat([torch.full((n, 1), float(b)), xyz], 1).float()


def test_weights_of_a_fully_present_cell_sum_to_one():
    coords = _lattice(6, 6, 6, lo=-3)
    q = _queries(200, -3.0, 2.0, 1)
    imap, w = IR.map_weight(coords, 1, q)
    assert bool((imap >= 0).all())
    assert float((w.sum(1) - 1).abs().max()) <= 1e-12
    assert bool((w >= 0).all())


def test_a_linear_function_is_reproduced_at_tensor_strides_1_and_2():
    for ts in (1, 2):
        coords = _lattice(7, 6, 5, lo=-4, ts=ts)
        A = torch.tensor([[0.5, -1.25], [2.0, 0.75], [-0.375, 1.5]], dtype=F64)
        f = lambda p: p.to(F64) @ A + torch.tensor([0.25, -3.0], dtype=F64)  # noqa: E731
        x = f(coords[:, 1:])
        q = _queries(300, -4.0, -4.0 + 4 * ts, 2 + ts)  # inside the box on every axis
        imap, w = IR.map_weight(coords, ts, q)
        assert bool((imap >= 0).all())
        y = IR.interp_fwd(x, imap, w)
        assert float((y - f(q[:, 1:].double())).abs().max()) <= 1e-12, ts


def test_against_grid_sample_on_a_dense_grid_interior_and_border():
    nx, ny, nz, C = 6, 7, 5, 3
    coords = _lattice(nx, ny, nz)
    g = torch.Generator().manual_seed(5)
    vol = torch.randn(1, C, nz, ny, nx, generator=g, dtype=F64)
    x = vol[0].permute(1, 2, 3, 0).reshape(-1, C)  # row order of _lattice: x fastest, z slowest
    q = torch.cat([_queries(300, 0.0, 4.0, 6),  # interior on every axis
                   _queries(300, -1.0, 7.0, 7),  # border: cells with absent corners, and points outside
                   torch.tensor([[0, 0, 0, 0], [0, 5, 6, 4], [0, 2.5, 0, 4], [0, -0.5, 3, 2], [0, 5.25, 6.5, 4.75]]).float()])
    imap, w = IR.map_weight(coords, 1, q)
    assert bool((imap < 0).any()) and bool((imap >= 0).all(1).any())
    y = IR.interp_fwd(x, imap, w)
    size = torch.tensor([nx, ny, nz], dtype=F64)
    grid = (2 * q[:, 1:].double() / (size - 1) - 1).reshape(1, -1, 1, 1, 3)
    ref = torch.nn.functional.grid_sample(vol, grid, mode="bilinear", align_corners=True, padding_mode="zeros")
    ref = ref[0, :, :, 0, 0].t()
    assert float((y - ref).abs().max()) <= 1e-12


def test_forward_and_backward_are_adjoint():
    g = torch.Generator().manual_seed(8)
    cell = torch.randperm(10 ** 3, generator=g)[:400]
    coords = torch.stack([torch.zeros_like(cell), cell % 10 - 4, cell // 10 % 10 - 4, cell // 100 - 4], 1).long()
    for ts in (1, 2):
        cm = coords.clone()
        cm[:, 1:] *= ts
        q = _queries(500, -5.0 * ts, 6.0 * ts, 9 + ts)
        imap, w = IR.map_weight(cm, ts, q)
        assert bool((imap < 0).any())
        x = torch.randn(400, 4, generator=g, dtype=F64)
        dy = torch.randn(500, 4, generator=g, dtype=F64)
        lhs = float((IR.interp_fwd(x, imap, w) * dy).sum())
        rhs = float((x * IR.interp_bwd(dy, imap, w, 400)).sum())
        assert abs(lhs - rhs) <= 1e-10 * max(abs(lhs), abs(rhs)), (ts, lhs, rhs)
        s, cnt = IR.interp_bwd_abs(dy, imap, 400)
        assert int(cnt.sum()) == int((imap >= 0).sum()) and bool((s >= IR.interp_bwd(dy, imap, w, 400).abs() - 1e-12).all())


def test_splat_keeps_the_feature_sum_and_lists_corners_in_first_occurrence_order():
    q = _queries(120, -3.0, 3.0, 12)
    q = torch.cat([q, q[:5], torch.tensor([[0, 1, -2, 0], [0, 1, -2, 0]]).float()])  # duplicates and integer points
    coords, imap, w = IR.splat_coords(q)
    assert torch.equal(coords[:8, 1:], coords[0, 1:] + torch.tensor([[c & 1, c >> 1 & 1, c >> 2 & 1] for c in range(8)]))
    assert imap[0].tolist() == list(range(8))
    assert len({tuple(c) for c in coords.tolist()}) == coords.shape[0] and int(imap.max()) == coords.shape[0] - 1
    first = [int((imap.reshape(-1) == v).nonzero()[0]) for v in range(coords.shape[0])]
    assert first == sorted(first)  # rows are numbered by first occurrence
    F = torch.randn(q.shape[0], 3, generator=torch.Generator().manual_seed(13), dtype=F64)
    Fs = IR.splat_fwd(F, imap, w, coords.shape[0])
    assert float((Fs.sum(0) - F.sum(0)).abs().max()) <= 1e-10  # partition of unity
    # the splat is the interpolation backward over its own map, and the map is what map_weight finds
    imap2, w2 = IR.map_weight(coords, 1, q)
    assert torch.equal(imap2, imap) and torch.equal(w2, w)


def test_negative_coordinates_floor():
    q = torch.tensor([[0, -0.25, -1.0, -2.5]]).float()
    b, lo, d = IR.cells(q, 1)
    assert lo.tolist() == [[-1, -1, -3]] and d.tolist() == [[0.75, 0.0, 0.5]]
    b, lo, d = IR.cells(q, 2)
    assert lo.tolist() == [[-2, -2, -4]] and d.tolist() == [[0.875, 0.5, 0.75]]
    coords = torch.tensor([[0, -1, -1, -3], [0, 0, -1, -3]])
    imap, w = IR.map_weight(coords, 1, q)
    assert imap[0].tolist() == [0, 1, -1, -1, -1, -1, -1, -1]
    assert w[0].tolist() == [0.125, 0.375, 0.0, 0.0, 0.125, 0.375, 0.0, 0.0]


def test_perlin_noise_host_logic():
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.data.perlin import PerlinNoise

    sig = inspect.signature(PerlinNoise.__init__).parameters
    assert [k for k in sig if k != "self"] == ["noise_params", "application_ratio", "device"]  # the reference's arguments
    p = PerlinNoise()
    assert list(map(tuple, p.noise_params)) == [(4, 4), (16, 16)] and p.application_ratio == 0.9 and p.device == "cpu"
    coords = torch.rand(10, 3)
    assert PerlinNoise(application_ratio=0)(coords) is coords  # never applied: the input, untouched
    assert PerlinNoise(noise_params=None, application_ratio=1.0)(coords) is coords
    assert ME.MinkowskiInterpolation().return_kernel_map is False and hasattr(ME.TensorField, "splat")
    assert hasattr(ME.SparseTensor, "interpolate") and hasattr(ME.SparseTensor, "features_at_coordinates")


def test_native_arguments_are_validated_before_any_launch():
    """NULL pointers, C < 1 and negative counts give -1 and a message (dummy non-NULL pointers are never dereferenced: the
    checks come before the first launch, so this runs without a GPU)."""
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000
    assert L.mink_interp_map_weight(None, 10, 1, None, None, 64, 5, None, None, None, None) == -1
    assert b"NULL" in L.mink_last_error()
    assert L.mink_interp_map_weight(P, -1, 1, P, P, 64, 5, P, P, P, None) == -1
    assert L.mink_interp_map_weight(P, 10, 0, P, P, 64, 5, P, P, P, None) == -1
    assert L.mink_interp_map_weight(P, 10, 1, P, P, 100, 5, P, P, P, None) == -1 and b"power of two" in L.mink_last_error()
    assert L.mink_interp_map_weight(P + 4, 10, 1, P, P, 64, 5, P, P, P, None) == -1 and b"aligned" in L.mink_last_error()
    assert L.mink_splat_coords(None, 10, None, None, None, None) == -1 and b"NULL" in L.mink_last_error()
    assert L.mink_splat_coords(P, -3, P, P, P, None) == -1
    assert L.mink_interp_gather(P, 0, 5, 0, P, P, 10, P, None) == -1 and b"C=0" in L.mink_last_error()
    assert L.mink_interp_gather(P, 3, 5, 4, P, P, 10, P, None) == -1  # row pitch below C
    assert L.mink_interp_gather(P, 4, 5, 4, None, P, 10, P, None) == -1 and b"NULL" in L.mink_last_error()
    assert L.mink_interp_gather(P, 4, 5, 4, P, P, -1, P, None) == -1
    assert L.mink_interp_segsum(P, 4, 10, 4, P, P, None, 5, 80, P, None) == -1 and b"NULL" in L.mink_last_error()
    assert L.mink_interp_segsum(P, 4, 10, 0, P, P, P, 5, 80, P, None) == -1
    assert L.mink_interp_segsum(P, 4, 10, 4, P, P, P, 5, 81, P, None) == -1  # more pairs than 8 per query
    assert L.mink_interp_segsum(P, 4, 10, 4, P, P, P, -5, 80, P, None) == -1
    # nothing to do is not an error
    assert L.mink_interp_gather(None, 4, 0, 4, None, None, 0, None, None) == 0
    assert L.mink_interp_segsum(None, 4, 0, 4, None, None, None, 0, 0, None, None) == 0
