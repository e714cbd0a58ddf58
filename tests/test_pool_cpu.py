"""CPU: the float64 restatement of the sparse pooling family (tests/pool_restate.py) against torch autograd and hand cases, and
the public surface of the feature -- the four new layers exported from nerf_downstream_amd.minkowski with ME's signatures,
their argument checks, and the new C entry points in libmink_hip.so."""
import ctypes
import inspect

import pytest
import torch

import pool_restate as PR

F64 = torch.float64


def _coords(counts, lo, hi, seed):
    """Integer (b, x, y, z) rows without duplicates within a sample, x, y, z in [lo, hi], sorted by sample."""
    g = torch.Generator().manual_seed(seed)
    side = hi - lo + 1
    rows = []
    for b, n in enumerate(counts):
        cell = torch.randperm(side ** 3, generator=g)[:n]
        xyz = torch.stack([cell % side, cell // side % side, cell // (side * side)], 1) + lo
        rows.append(torch.cat([torch.full((n, 1), b), xyz], 1))
    return torch.cat(rows).long()


def _rand(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


# ------------------------------------------------------------------------------------------------ backward formulas
@pytest.mark.parametrize("k,s", [(2, 2), (3, 2), (3, 1)])
def test_local_backward_formulas_match_autograd(k, s):
    coords = _coords([60, 0, 1, 45], -4, 5, 1)
    out, table = PR.pooling_maps(coords, 1, k, s)
    n, C = coords.shape[0], 5
    x, dy = _rand((n, C), 2), _rand((out.shape[0], C), 3)
    for fwd, bwd in ((PR.sum_fwd, PR.sum_bwd), (PR.avg_fwd, PR.avg_bwd)):
        xa = x.clone().requires_grad_(True)
        fwd(xa, table).backward(dy)
        assert torch.allclose(xa.grad, bwd(dy, table, n), rtol=0, atol=1e-13)
    # max: a dense rewrite -- the windows as a [m, K, C] tensor with -inf in the empty places, torch's amax (no ties: continuous x)
    y, arg = PR.max_fwd(x, table)
    xa = x.clone().requires_grad_(True)
    xp = torch.cat([xa, torch.full((1, C), -float("inf"), dtype=F64)], 0)
    dense = xp[table].amax(1)
    assert torch.equal(dense.detach(), y)
    dense.backward(dy)
    assert torch.allclose(xa.grad, PR.max_bwd(dy, arg, table, n), rtol=0, atol=1e-13)
    assert torch.equal(PR.max_fwd_forced(x, arg), y)
    # every window of a strided map holds at least one input, and the sum of the gradient is kept
    assert int(PR.counts(table).min()) >= 1
    assert torch.allclose(PR.max_bwd(dy, arg, table, n).sum(0), dy.sum(0), atol=1e-12)
    assert torch.allclose(PR.avg_bwd(dy, table, n).sum(0), dy.sum(0), atol=1e-12)


def test_global_backward_formulas_match_autograd():
    coords = _coords([60, 0, 1, 45], -4, 5, 4)
    off = PR.offsets_of(coords, 4)
    assert off == [0, 60, 60, 61, 106]
    n, C = coords.shape[0], 5
    x, dy = _rand((n, C), 5), _rand((4, C), 6)
    y, arg = PR.global_max_fwd(x, off)
    xa = x.clone().requires_grad_(True)
    dense = torch.stack([xa[off[b]:off[b + 1]].amax(0) if off[b + 1] > off[b] else torch.zeros(C, dtype=F64) for b in range(4)])
    assert torch.equal(dense.detach(), y)
    dense.backward(dy)
    assert torch.equal(xa.grad, PR.global_max_bwd(dy, arg, n))
    assert torch.equal(PR.max_fwd_forced(x, arg), y)
    xa = x.clone().requires_grad_(True)
    PR.global_sum_fwd(xa, off).backward(dy)
    assert torch.equal(xa.grad, PR.global_sum_bwd(dy, off))


# ------------------------------------------------------------------------------------------------ hand cases
def test_hand_cases():
    # two voxels that share a 2^3 cell and a third alone in its cell, at negative coordinates
    coords = torch.tensor([[0, -1, -1, -1], [0, -2, -1, -1], [0, -3, 5, 0]])
    out, i2o = PR.strided_coords(coords, 1, 2)
    assert out.tolist() == [[0, -2, -2, -2], [0, -4, 4, 0]] and i2o.tolist() == [0, 0, 1]  # floor, not truncation towards zero
    table = PR.window_table(coords, out, 1, 2)
    assert PR.counts(table).tolist() == [2, 1]
    # offsets of kernel 2 are {0, 1}^3 with x fastest: (-1,-1,-1) = base + (1,1,1) is entry 7, (-2,-1,-1) = base + (0,1,1) entry 6
    # (-3, 5, 0) = (-4, 4, 0) + (1, 1, 0): entry 3
    assert table[0].tolist() == [-1, -1, -1, -1, -1, -1, 1, 0] and table[1].tolist() == [-1, -1, -1, 2, -1, -1, -1, -1]
    x = torch.tensor([[1.0, -8.0], [3.0, -2.0], [5.0, 7.0]], dtype=F64)
    assert PR.avg_fwd(x, table).tolist() == [[2.0, -5.0], [5.0, 7.0]]  # a window with one present voxel averages to that voxel
    assert PR.sum_fwd(x, table).tolist() == [[4.0, -10.0], [5.0, 7.0]]
    y, arg = PR.max_fwd(x, table)
    assert y.tolist() == [[3.0, -2.0], [5.0, 7.0]] and arg.tolist() == [[1, 1], [2, 2]]
    dy = torch.tensor([[10.0, 20.0], [30.0, 40.0]], dtype=F64)
    assert PR.avg_bwd(dy, table, 3).tolist() == [[5.0, 10.0], [5.0, 10.0], [30.0, 40.0]]
    assert PR.max_bwd(dy, arg, table, 3).tolist() == [[0.0, 0.0], [10.0, 20.0], [30.0, 40.0]]
    # a tie goes to the lowest kernel offset: row 1 sits at entry 6, row 0 at entry 7
    yt, argt = PR.max_fwd(torch.ones(3, 1, dtype=F64), table)
    assert yt.tolist() == [[1.0], [1.0]] and argt.tolist() == [[1], [2]]
    # an isolated voxel under k=3 s=1 returns itself (every pool), through the centre entry 13
    _, t3 = PR.pooling_maps(coords[2:], 1, 3, 1)
    assert t3.tolist() == [[-1] * 13 + [0] + [-1] * 13]
    for f in (PR.avg_fwd, PR.sum_fwd, lambda a, t: PR.max_fwd(a, t)[0]):
        assert torch.equal(f(x[2:], t3), x[2:])


def test_global_max_empty_sample_and_ties():
    x = torch.tensor([[1.0, 4.0], [2.0, 4.0], [2.0, 3.0], [-5.0, -6.0]], dtype=F64)
    off = [0, 3, 3, 4]  # the middle sample is empty
    y, arg = PR.global_max_fwd(x, off)
    assert y.tolist() == [[2.0, 4.0], [0.0, 0.0], [-5.0, -6.0]]
    assert arg.tolist() == [[1, 0], [-1, -1], [3, 3]]  # the lowest row attaining the maximum; -1 for the empty sample
    dy = torch.tensor([[1.0, 2.0], [3.0, 4.0], [5.0, 6.0]], dtype=F64)
    assert PR.global_max_bwd(dy, arg, 4).tolist() == [[0.0, 2.0], [1.0, 0.0], [0.0, 0.0], [5.0, 6.0]]  # the empty sample's dy lands nowhere
    assert PR.global_sum_fwd(x, off).tolist() == [[5.0, 11.0], [0.0, 0.0], [-5.0, -6.0]]
    assert PR.global_sum_bwd(dy, off).tolist() == [[1.0, 2.0]] * 3 + [[5.0, 6.0]]
    assert PR.global_avg_fwd(x, off)[1].tolist() == [0.0, 0.0]


# ------------------------------------------------------------------------------------------------ public surface
def test_new_layers_are_exported_with_me_signatures():
    import nerf_downstream_amd.minkowski as ME

    local = ["kernel_size", "stride", "dilation", "kernel_generator", "dimension"]
    for name in ("MinkowskiAvgPooling", "MinkowskiMaxPooling", "MinkowskiSumPooling"):
        cls = getattr(ME, name)
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters)[1:] == local, (name, sig)
        assert sig.parameters["kernel_size"].default is inspect.Parameter.empty
        assert [sig.parameters[p].default for p in local[1:]] == [1, 1, None, None], (name, sig)
        layer = cls(kernel_size=3, stride=2, dimension=3)
        assert isinstance(layer, torch.nn.Module) and (layer.kernel_size, layer.stride) == (3, 2) and not list(layer.parameters())
    for name in ("MinkowskiGlobalMaxPooling", "MinkowskiGlobalSumPooling"):
        cls = getattr(ME, name)
        assert list(inspect.signature(cls).parameters) == [], name
        assert isinstance(cls(), torch.nn.Module) and not list(cls().parameters())
    assert ME.MinkowskiSumPooling(2, 2, dimension=3).overlapping is False and ME.MinkowskiSumPooling(3, 2, dimension=3).overlapping is True
    from nerf_downstream_amd.minkowski import functional as Fn

    for name in ("AvgPoolFunction", "GlobalMaxPoolFunction", "GlobalSumPoolFunction", "SparseMaxPoolFunction", "OverlapSumPoolFunction"):
        assert issubclass(getattr(Fn, name), torch.autograd.Function), name


@pytest.mark.parametrize("layer", ["MinkowskiAvgPooling", "MinkowskiMaxPooling", "MinkowskiSumPooling"])
def test_bad_arguments_raise_value_error(layer):
    import nerf_downstream_amd.minkowski as ME

    cls = getattr(ME, layer)
    for k, s in ((1, 1), (2, 2), (3, 1), (3, 2), (3, 3), ([3, 3, 3], [2, 2, 2])):
        cls(k, s, dimension=3)
    with pytest.raises(ValueError, match="dimension"):
        cls(2, 2)
    with pytest.raises(ValueError, match="dimension"):
        cls(2, 2, dimension=2)
    with pytest.raises(ValueError, match="dilation"):
        cls(3, 2, dilation=2, dimension=3)
    with pytest.raises(ValueError, match="27"):
        cls(4, 4, dimension=3)
    with pytest.raises(ValueError, match="27"):
        cls(5, 2, dimension=3)
    with pytest.raises(ValueError, match="odd or equal to the stride"):
        cls(2, 1, dimension=3)
    with pytest.raises(ValueError, match="kernel_generator"):
        cls(3, 2, kernel_generator=object(), dimension=3)
    with pytest.raises(ValueError, match="anisotropic"):
        cls([3, 3, 2], 2, dimension=3)
    with pytest.raises(ValueError, match=">= 1"):
        cls(3, 0, dimension=3)


NEW_SYMBOLS = ["mink_pool_local_fwd", "mink_pool_local_bwd", "mink_pool_local_max_fwd", "mink_pool_local_max_bwd",
               "mink_global_pool_workspace_bytes", "mink_global_max_fwd", "mink_global_max_bwd", "mink_global_sum_fwd",
               "mink_global_sum_bwd"]


def test_new_symbols_exported_and_arguments_checked_without_gpu():
    from nerf_downstream_amd import _lib

    _lib.build()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(raw, name), f"{name} not exported by libmink_hip.so"
        assert name in _lib.SIGNATURES, name
    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced: every check below comes before the first launch
    # partials: B x G x C doubles, G = min(ceil(n / 256), 2048 / B) row chunks per sample
    assert L.mink_global_pool_workspace_bytes(4100, 32, 1) == 17 * 32 * 8
    assert L.mink_global_pool_workspace_bytes(388, 70, 4) == 4 * 2 * 70 * 8
    assert L.mink_global_pool_workspace_bytes(10 ** 6, 8, 65535) == 65535 * 8 * 8
    assert L.mink_pool_local_fwd(None, 4, 4, None, 10, 27, 1, None, None, None) == -1 and b"NULL" in L.mink_last_error()
    assert L.mink_pool_local_fwd(P, 4, 4, P, 10, 27, 1, P, None, None) == -1 and b"NULL" in L.mink_last_error()  # the average needs cnt
    assert L.mink_pool_local_fwd(P, 4, 4, P, 10, 27, 2, P, P, None) == -1 and b"mode" in L.mink_last_error()
    assert L.mink_pool_local_fwd(P, 3, 4, P, 10, 27, 0, P, P, None) == -1 and b"ldx" in L.mink_last_error()
    assert L.mink_pool_local_bwd(P, 5000, P, 10, 27, 0, None, P, None) == -1 and b"4096" in L.mink_last_error()
    assert L.mink_pool_local_max_fwd(P, 4, 4, P, 10, 0, P, P, None) == -1 and b"K=0" in L.mink_last_error()
    assert L.mink_pool_local_max_bwd(P, None, 4, P, 10, 27, P, None) == -1 and b"NULL" in L.mink_last_error()
    need = L.mink_global_pool_workspace_bytes(1000, 8, 2)
    assert L.mink_global_max_fwd(P, 1000, 8, 8, P, 2, P, P, P, need - 1, None) == -1 and b"workspace" in L.mink_last_error()
    assert L.mink_global_sum_fwd(P, 1000, 8, 8, P, 2, P, P, need - 1, None) == -1 and b"workspace" in L.mink_last_error()
    assert L.mink_global_max_fwd(P, 1000, 8, 8, P, 65536, P, P, P, 1 << 30, None) == -1 and b"65535" in L.mink_last_error()
    assert L.mink_global_max_bwd(P, P, 1000, 0, P, 2, P, None) == -1 and b"bad shape" in L.mink_last_error()
    assert L.mink_global_sum_bwd(None, 1000, 8, P, 2, P, None) == -1 and b"NULL" in L.mink_last_error()
    # empty inputs are accepted without a launch
    assert L.mink_pool_local_fwd(None, 4, 4, None, 0, 27, 1, None, None, None) == 0
    assert L.mink_global_sum_bwd(None, 0, 8, None, 2, None, None) == 0
