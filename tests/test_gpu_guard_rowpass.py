"""-m gpu: the row-pass kernels of csrc/norm.hip, pool.hip, interp.hip and field.hip (the 16-byte / dword lane choice and the
chunked per-sample reduction of csrc/rowpass.h) inside guard bands (tests/guarded.py).

Rules of tests/test_gpu_guard.py: every entry point is called through the C ABI, every output, workspace and statistics
buffer is a Guarded of EXACTLY the size include/mink_hip.h or the matching *_workspace_bytes() names, every input (offset,
table, members and seg arrays included) a Guarded.input with NaN bands and, where the header gives the matrix a row pitch,
NaN pad columns.  After the call: check() on every buffer, then every written element finite and within the bound the
existing test of the same entry point uses (test_gpu_norm, test_gpu_pool, test_gpu_interp, test_gpu_point -- imported or
restated beside the use), of the float64 restatement computed from the logical operands on the CPU; integer-valued results
(tables, arguments, counts, gathers) are equal.

Which lanes a case reaches is restated from the host code (`_vec`): 16 bytes when C % 4 == 0, every pitch % 4 == 0 and
every pointer is 16-byte aligned, dwords otherwise -- through an odd C, through a pitch (ld % 4 != 0 at a C that is a
multiple of 4) or through one pointer that Guarded(skew=4) puts 4 bytes behind a 16-byte boundary.  Nothing here is meant
to fault: no buffer is smaller than the library asks for and no index leaves what the header says is tolerated."""
import ctypes
import functools

import pytest
import torch

import interp_restate as IR
import norm_restate as NR
import point_restate as PT
import pool_restate as PR
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23   # PR.EPS32 / IR.EPS32: one ulp of a float in [1, 2)
TINY = 2.0 ** -149
K_BOUND = 27       # test_gpu_pool.K: its bounds are (K + 1) EPS sum |terms| and K EPS sum |terms| with this K, whatever the table's K
FWD_TOL = dict(atol=2e-5, rtol=1e-5)   # test_gpu_norm.FWD_TOL / GRAD_TOL
GRAD_TOL = dict(atol=2e-4, rtol=1e-4)
MINK_STATUS_RANGE = 1  # include/mink_hip.h


def _dev():
    return torch.device("cuda", 0)


def _st():
    return torch.cuda.current_stream().cuda_stream


def _ptr(g):
    return None if g is None else g.ptr


def _gin(t, ld=None, name="input", skew=0):
    return Guarded.input(t.to(_dev()), ld=ld, name=name, skew=skew)


def _gout(shape, dtype=torch.float32, name="output", **kw):
    return Guarded(shape, dtype, _dev(), name=name, **kw)


def _ws(nbytes, name="workspace"):
    return Guarded(int(nbytes), torch.uint8, _dev(), written="any", name=name)


def _lib():
    from nerf_downstream_amd._lib import check, lib

    return lib(), check


def _done(*bufs):
    torch.cuda.synchronize()
    check_all(*bufs)


def _vec(C, *bufs, lds=()):
    """The host's lane decision, restated: 16-byte lanes iff C % 4 == 0, every pitch % 4 == 0, every pointer 16-byte aligned."""
    return C % 4 == 0 and all(ld % 4 == 0 for ld in lds) and all(g is None or g.ptr % 16 == 0 for g in bufs)


def _cpu(g):
    return g.logical().cpu()


def _within(got, ref, bound, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert_finite(got, what)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (what, float(err.max()), float((err - bound).max()))


def _close(got, ref, tol, what):
    assert got.shape == ref.shape, what
    assert_finite(got, what)
    assert torch.allclose(got.double(), ref, **tol), (what, float((got.double() - ref).abs().max()))


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _sample_chunks(n, B):
    """rowpass.h sample_chunks: the G row chunks every sample is cut into."""
    return max(1, min(-(-n // 256), max(1, 2048 // max(B, 1))))


def _offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + int(s))
    return off


@functools.lru_cache(None)
def _samples(n, B):
    """Offsets of the three (n, B) shapes: (300, 1) and (20000, 3) are B samples of uneven size with an empty sample first, in
    the middle and last (B + 3 samples in all: G = 2, and G = 79 > 64, where the finalize wave takes a second trip over the
    chunks); (600, 2500) is 2500 samples of 0, 1, 2 or 3 rows, most of them empty (G = 1)."""
    g = torch.Generator().manual_seed(n + B)
    if B == 2500:
        sizes = torch.zeros(B, dtype=torch.int64)
        live = torch.randperm(B, generator=g)[:400]
        sizes[live[:250]], sizes[live[250:350]], sizes[live[350:]] = 1, 2, 3
        assert int(sizes.sum()) == n
        off = _offsets(sizes.tolist())
    else:
        cuts = sorted((torch.randperm(n - 1, generator=g)[: B - 1] + 1).tolist())
        parts = [b - a for a, b in zip([0] + cuts, cuts + [n])]
        sizes = [0] + parts[: (B + 1) // 2] + [0] + parts[(B + 1) // 2 :] + [0]
        off = _offsets(sizes)
    assert off[-1] == n
    G = _sample_chunks(n, len(off) - 1)
    assert G == {300: 2, 20000: 79, 600: 1}[n], G
    return tuple(off)


NB_SHAPES = [(300, 1), (20000, 3), (600, 2500)]


# ================================================================================================ instance norm
def _run_instance_norm(n, C, off, relu, residual, dres, seed, skew_out=0, skew_in=0, expect_vec=None):
    L, check = _lib()
    B = len(off) - 1
    eps = 1e-8
    x, dy, res = _randn((n, C), seed) * 1.5 + 0.2, _randn((n, C), seed + 1), _randn((n, C), seed + 2)
    if B > 1000:
        # samples of two and three rows: with eps = 1e-8 two rows that happen to lie close together have an invstd of up to
        # 1e4, and the centred tolerances of test_gpu_norm are for samples whose spread is of order one.  Rows of one sample
        # are put 2 apart with a jitter of 0.25, so that every sample of more than one row has a standard deviation near 1.
        j = torch.arange(n) - torch.tensor(off)[NR.sample_of_rows(off, n)]
        x = 0.2 + 2.0 * j[:, None].float() + 0.25 * _randn((n, C), seed)
    gamma, beta = torch.linspace(0.5, 1.5, C), torch.linspace(-0.2, 0.2, C)
    gx, gdy = _gin(x, name="x", skew=skew_in), _gin(dy, name="dy")
    gres = _gin(res, name="residual") if residual else None
    gga, gbe = _gin(gamma, name="gamma"), _gin(beta, name="beta")
    goff = _gin(torch.tensor(off, dtype=torch.int32), name="batch_offsets")
    gy = _gout((n, C), name="y", skew=skew_out)
    gmean, ginv = _gout((B, C), name="mean"), _gout((B, C), name="invstd")
    need = L.mink_in_workspace_bytes(n, C, B)
    assert need == (B * _sample_chunks(n, B) * 2 * C + B * 2 * C) * 8 + 2 * B * C * 4
    ws = _ws(need, "in_fwd workspace")
    if expect_vec is not None:
        assert _vec(C, gx, gy, gres, gmean, ginv, gga, gbe) == expect_vec
    check(L.mink_in_fwd(gx.ptr, n, C, goff.ptr, B, eps, gga.ptr, gbe.ptr, _ptr(gres), int(relu), gy.ptr, gmean.ptr, ginv.ptr, ws.ptr,
                        ws.nbytes, _st()))
    _done(gx, gres, gga, gbe, goff, gy, gmean, ginv, ws)
    what = f"IN n={n} B={B} C={C} relu={relu} res={residual}"
    rmean, rinv, _ = NR.instance_stats(x, off, eps)
    empty = torch.tensor([off[b + 1] == off[b] for b in range(B)])
    mean, inv = _cpu(gmean), _cpu(ginv)
    assert bool((mean[empty] == 0).all()) and bool((inv[empty] == 0).all()), what + ": an empty sample holds (0, 0)"
    _close(mean, rmean, FWD_TOL, what + " mean")
    _close(inv, rinv, FWD_TOL, what + " invstd")
    # backward, from the forward's own y, mean and invstd (guarded inputs now)
    y = _cpu(gy)
    gyin, gmin, giin = _gin(y, name="y (in)", skew=skew_out), _gin(mean, name="mean (in)"), _gin(inv, name="invstd (in)")
    gdx = _gout((n, C), name="dx")
    gdres = _gout((n, C), name="dresidual") if dres else None
    gdga, gdbe = _gout((C,), name="dgamma"), _gout((C,), name="dbeta")
    ws2 = _ws(need, "in_bwd workspace")
    check(L.mink_in_bwd(gdy.ptr, gx.ptr, gyin.ptr, n, C, goff.ptr, B, gmin.ptr, giin.ptr, gga.ptr, int(relu), gdx.ptr, _ptr(gdres), gdga.ptr,
                        gdbe.ptr, ws2.ptr, ws2.nbytes, _st()))
    _done(gdy, gx, gyin, goff, gmin, giin, gga, gdx, gdres, gdga, gdbe, ws2)
    import test_gpu_norm as TN

    assert TN.FWD_TOL == FWD_TOL and TN.GRAD_TOL == GRAD_TOL
    r = res if residual else None
    z = NR.instance_norm_fwd(x, off, gamma, beta, eps, r, False)
    got = (y, _cpu(gdx), _cpu(gdga), _cpu(gdbe), _cpu(gdres) if dres else None)
    for t in got:
        if t is not None:
            assert_finite(t, what)
    TN._check_centred(got, z.clamp_min(0) if relu else z, lambda mask: NR.instance_norm_bwd(dy, x, off, gamma, beta, eps, r, relu, mask),
                      z, relu, dres, what)


@pytest.mark.parametrize("n,B", NB_SHAPES)
@pytest.mark.parametrize("C", [3, 4, 257, 1028])  # 257: dword lanes, tprb 256, a second slab with one live lane; 1028: 257 16-byte groups
def test_instance_norm_stays_inside_its_buffers(C, n, B):
    off = _samples(n, B)
    i = [3, 4, 257, 1028].index(C) + NB_SHAPES.index((n, B))  # every (relu, residual, dresidual) combination turns up
    relu, residual, dres = bool(i & 1), bool(i & 2), not bool(i & 1) or C == 4
    _run_instance_norm(n, C, off, relu, residual, dres, 1000 + C + n, expect_vec=C % 4 == 0)


@pytest.mark.parametrize("which", ["output y", "input x"])
def test_instance_norm_with_one_pointer_off_16_bytes_takes_dword_lanes(which):
    off = _samples(300, 1)
    _run_instance_norm(300, 8, off, True, True, True, 1100, skew_out=4 if which == "output y" else 0, skew_in=4 if which == "input x" else 0,
                       expect_vec=False)


# ================================================================================================ layer norm
def _ln_group(ncg):
    gs = 1
    while gs < ncg and gs < 64:
        gs <<= 1
    return gs


def _ln_grid(n, gs, cap):
    """norm.hip ln_grid: a wave holds 64 / gs rows, a workgroup four waves."""
    return max(1, min(-(-n // (4 * (64 // gs))), cap))


def _run_layer_norm(n, C, relu, residual, dres, seed, skew_out=0, skew_in=0, expect_vec=None, bwd_blocks=None):
    L, check = _lib()
    eps = 1e-5
    x, dy, res = _randn((n, C), seed) * 1.5 + 0.2, _randn((n, C), seed + 1), _randn((n, C), seed + 2)
    gamma, beta = torch.linspace(0.5, 1.5, C), torch.linspace(-0.2, 0.2, C)
    gx, gdy = _gin(x, name="x", skew=skew_in), _gin(dy, name="dy")
    gres = _gin(res, name="residual") if residual else None
    gga, gbe = _gin(gamma, name="gamma"), _gin(beta, name="beta")
    gy = _gout((n, C), name="y", skew=skew_out)
    gmean, ginv = _gout((n,), name="mean"), _gout((n,), name="invstd")
    if expect_vec is not None:
        assert _vec(C, gx, gy, gres, gga, gbe) == expect_vec
    check(L.mink_ln_fwd(gx.ptr, n, C, eps, gga.ptr, gbe.ptr, _ptr(gres), int(relu), gy.ptr, gmean.ptr, ginv.ptr, _st()))
    _done(gx, gres, gga, gbe, gy, gmean, ginv)
    what = f"LN n={n} C={C} relu={relu} res={residual}"
    rmean, rinv, _ = NR.layer_stats(x, eps)
    y, mean, inv = _cpu(gy), _cpu(gmean), _cpu(ginv)
    _close(mean, rmean[:, 0], FWD_TOL, what + " mean")
    _close(inv, rinv[:, 0], FWD_TOL, what + " invstd")
    gyin, gmin, giin = _gin(y, name="y (in)", skew=skew_out), _gin(mean, name="mean (in)"), _gin(inv, name="invstd (in)")
    gdx = _gout((n, C), name="dx")
    gdres = _gout((n, C), name="dresidual") if dres else None
    gdga, gdbe = _gout((C,), name="dgamma"), _gout((C,), name="dbeta")
    need = L.mink_ln_workspace_bytes(n, C)
    assert need == 1024 * 2 * C * 8
    if bwd_blocks is not None:
        vec = _vec(C, gdy, gx, gyin if relu else None, gdx, gdres, gga)
        assert _ln_grid(n, _ln_group(C // 4 if vec else C), 1024) == bwd_blocks
    ws = _ws(need, "ln_bwd workspace")
    check(L.mink_ln_bwd(gdy.ptr, gx.ptr, gyin.ptr, n, C, gmin.ptr, giin.ptr, gga.ptr, int(relu), gdx.ptr, _ptr(gdres), gdga.ptr, gdbe.ptr,
                        ws.ptr, ws.nbytes, _st()))
    _done(gdy, gx, gyin, gmin, giin, gga, gdx, gdres, gdga, gdbe, ws)
    import test_gpu_norm as TN

    r = res if residual else None
    z = NR.layer_norm_fwd(x, gamma, beta, eps, r, False)
    got = (y, _cpu(gdx), _cpu(gdga), _cpu(gdbe), _cpu(gdres) if dres else None)
    for t in got:
        if t is not None:
            assert_finite(t, what)
    TN._check_centred(got, z.clamp_min(0) if relu else z, lambda mask: NR.layer_norm_bwd(dy, x, gamma, beta, eps, r, relu, mask), z, relu, dres,
                      what)


@pytest.mark.parametrize("C", [1, 3, 4, 5, 256, 260, 509, 512])
def test_layer_norm_stays_inside_its_buffers(C):
    for i, n in enumerate((1, 63, 65, 1025)):
        j = i + C
        _run_layer_norm(n, C, bool(j & 1), bool(j & 2), i != 1, 2000 + 10 * C + n, expect_vec=C % 4 == 0)


@pytest.mark.parametrize("which", ["output y", "input x"])
def test_layer_norm_with_one_pointer_off_16_bytes_takes_dword_lanes(which):
    _run_layer_norm(65, 8, True, True, True, 2100, skew_out=4 if which == "output y" else 0, skew_in=4 if which == "input x" else 0,
                    expect_vec=False)


def test_layer_norm_backward_at_the_cap_of_its_grid():
    """C = 1: a workgroup holds 256 rows, so n = 1024 x 256 + 1 asks for 1025 workgroups and gets kLnRedBlocks = 1024: every
    partial row of the workspace is written and the first workgroup takes a second trip for the last row."""
    n = 1024 * 256 + 1
    assert _ln_grid(n - 1, 1, 1 << 30) == 1024 and _ln_grid(n, 1, 1 << 30) == 1025
    _run_layer_norm(n, 1, False, False, True, 2200, expect_vec=False, bwd_blocks=1024)


# ================================================================================================ local pools
@functools.lru_cache(None)
def _window_table(n_out, n_in, K, seed):
    """nbr[n_out][K] (int64, -1 = empty) with an exact transpose (every column is an injection of the present rows into the
    inputs): about 45 % empty, rows 5, 64 and the last entirely empty, one column empty everywhere; and nbr_t[n_in][K]."""
    g = torch.Generator().manual_seed(seed)
    assert n_out <= n_in
    nbr = torch.stack([torch.randperm(n_in, generator=g)[:n_out] for _ in range(K)], 1)
    nbr[torch.rand(n_out, K, generator=g) < 0.45] = -1
    if K > 1:
        nbr[:, K // 2 - 1] = -1
    for r in (5, 64, n_out - 1):
        nbr[r] = -1
    nbr_t = torch.full((n_in, K), -1, dtype=torch.int64)
    o, j = torch.nonzero(nbr >= 0, as_tuple=True)
    nbr_t[nbr[o, j], j] = o
    return nbr, nbr_t


POOL_N_OUT, POOL_N_IN = 203, 301  # several workgroups of 256 threads at every C; no multiple of anything


def _run_local_pools(K, C, ldx, seed, skew_x=0, skew_y=0, skew_dy=0, skew_dx=0):
    L, check = _lib()
    n_out, n_in = POOL_N_OUT, POOL_N_IN
    table, table_t = _window_table(n_out, n_in, K, 7 * K)
    x, dy = _randn((n_in, C), seed), _randn((n_out, C), seed + 1)
    gx = _gin(x, ld=ldx, name="x", skew=skew_x)
    gnbr, gnbrt = _gin(table.int(), name="nbr"), _gin(table_t.int(), name="nbr_t")
    gdy = _gin(dy, name="dy", skew=skew_dy)
    cnt_ref = PR.counts(table)
    expect_fwd = _vec(C, gx, lds=(ldx,)) and skew_y == 0
    expect_bwd = C % 4 == 0 and skew_dy == 0 and skew_dx == 0
    for mode, with_cnt in ((0, False), (0, True), (1, True)):
        what = f"local pool mode {mode} K={K} C={C} ldx={ldx}"
        gy = _gout((n_out, C), name="y", skew=skew_y)
        gcnt = _gout((n_out,), torch.int32, name="cnt") if with_cnt else None
        assert _vec(C, gx, gy, lds=(ldx,)) == expect_fwd
        check(L.mink_pool_local_fwd(gx.ptr, ldx, C, gnbr.ptr, n_out, K, mode, gy.ptr, _ptr(gcnt), _st()))
        _done(gx, gnbr, gy, gcnt)
        if with_cnt:
            assert torch.equal(gcnt.t.cpu().long(), cnt_ref), what
        ref = PR.avg_fwd(x, table) if mode else PR.sum_fwd(x, table)
        _within(_cpu(gy), ref, (K_BOUND + 1) * EPS * PR.sum_fwd_abs(x, table, bool(mode)), what + " y")
        assert bool((_cpu(gy)[cnt_ref == 0] == 0).all()), what + ": a row with no present entry gets 0"
        if not with_cnt:
            continue
        gcin = _gin(cnt_ref.int(), name="cnt (in)")
        gdx = _gout((n_in, C), name="dx", skew=skew_dx)
        assert _vec(C, gdy, gdx) == expect_bwd
        check(L.mink_pool_local_bwd(gdy.ptr, C, gnbrt.ptr, n_in, K, mode, gcin.ptr if mode else None, gdx.ptr, _st()))
        _done(gdy, gnbrt, gcin, gdx)
        ref = PR.avg_bwd(dy, table, n_in) if mode else PR.sum_bwd(dy, table, n_in)
        _within(_cpu(gdx), ref, (K_BOUND + 1) * EPS * PR.sum_bwd_abs(dy, table, n_in, bool(mode)), what + " dx")
    # max pooling
    what = f"local max pool K={K} C={C} ldx={ldx}"
    gy, garg = _gout((n_out, C), name="y", skew=skew_y), _gout((n_out, C), torch.int32, name="arg")
    assert _vec(C, gx, gy, garg, lds=(ldx,)) == expect_fwd
    check(L.mink_pool_local_max_fwd(gx.ptr, ldx, C, gnbr.ptr, n_out, K, gy.ptr, garg.ptr, _st()))
    _done(gx, gnbr, gy, garg)
    ry, rarg = PR.max_fwd(x, table)
    assert_finite(_cpu(gy), what)
    assert torch.equal(_cpu(gy).double(), ry) and torch.equal(_cpu(garg).long(), rarg), what
    gain = _gin(rarg.int(), name="arg (in)")
    gdx = _gout((n_in, C), name="dx", skew=skew_dx)
    assert _vec(C, gdy, gain, gdx) == expect_bwd
    check(L.mink_pool_local_max_bwd(gdy.ptr, gain.ptr, C, gnbrt.ptr, n_in, K, gdx.ptr, _st()))
    _done(gdy, gain, gnbrt, gdx)
    _within(_cpu(gdx), PR.max_bwd(dy, rarg, table, n_in), K_BOUND * EPS * PR.max_bwd_abs(dy, rarg, table, n_in), what + " dx")


@pytest.mark.parametrize("K", [1, 27, 81])
@pytest.mark.parametrize("C", [3, 4, 36])
def test_local_pools_stay_inside_their_buffers(C, K):
    for ldx in (C, C + 4, C + 1):  # contiguous; padded, 16-byte lanes where C % 4 == 0; a pitch that forces dwords at any C
        _run_local_pools(K, C, ldx, 3000 + 100 * C + K)


@pytest.mark.parametrize("which", ["x", "y", "dy", "dx"])
def test_local_pools_with_one_pointer_off_16_bytes_take_dword_lanes(which):
    _run_local_pools(27, 8, 12, 3100, **{"skew_" + which: 4})


# ================================================================================================ global pools
def _run_global_pools(n, C, off, ldx, seed, skew_x=0, skew_dx=0):
    L, check = _lib()
    B = len(off) - 1
    x, dy = _randn((n, C), seed), _randn((B, C), seed + 1)
    gx = _gin(x, ld=ldx, name="x", skew=skew_x)
    goff = _gin(torch.tensor(off, dtype=torch.int32), name="batch_offsets")
    gdy = _gin(dy, name="dy")
    need = L.mink_global_pool_workspace_bytes(n, C, B)
    assert need == B * _sample_chunks(n, B) * C * 8
    what = f"global pool n={n} B={B} C={C} ldx={ldx}"
    empty = torch.tensor([off[b + 1] == off[b] for b in range(B)])
    # the backward restatements walk the samples one by one: they are handed the samples that own rows (an empty one owns no
    # row of dx), which for 2500 samples of which 2100 are empty is the difference between 10 s and a tenth of one
    live = ~empty
    off_live = [0] + [off[b + 1] for b in range(B) if off[b + 1] > off[b]]
    # max
    gy, garg, ws = _gout((B, C), name="y"), _gout((B, C), torch.int32, name="arg"), _ws(need, "global_max workspace")
    check(L.mink_global_max_fwd(gx.ptr, n, ldx, C, goff.ptr, B, gy.ptr, garg.ptr, ws.ptr, ws.nbytes, _st()))
    _done(gx, goff, gy, garg, ws)
    ry, rarg = PR.global_max_fwd(x, off)
    y, arg = _cpu(gy), _cpu(garg)
    assert_finite(y, what)
    assert torch.equal(y.double(), ry) and torch.equal(arg.long(), rarg), what + " max"
    assert bool((y[empty] == 0).all()) and bool((arg[empty] == -1).all()), what
    gain, gdx = _gin(rarg.int(), name="arg (in)"), _gout((n, C), name="dx", skew=skew_dx)
    check(L.mink_global_max_bwd(gdy.ptr, gain.ptr, n, C, goff.ptr, B, gdx.ptr, _st()))
    _done(gdy, gain, goff, gdx)
    assert torch.equal(_cpu(gdx).double(), PR.global_max_bwd(dy[live], rarg[live], n)), what + " max dx"
    # sum
    gy, ws = _gout((B, C), name="y"), _ws(need, "global_sum workspace")
    check(L.mink_global_sum_fwd(gx.ptr, n, ldx, C, goff.ptr, B, gy.ptr, ws.ptr, ws.nbytes, _st()))
    _done(gx, goff, gy, ws)
    ref = PR.global_sum_fwd(x, off)
    _within(_cpu(gy), ref, EPS * ref.abs() + TINY, what + " sum y")
    gdx = _gout((n, C), name="dx", skew=skew_dx)
    check(L.mink_global_sum_bwd(gdy.ptr, n, C, goff.ptr, B, gdx.ptr, _st()))
    _done(gdy, goff, gdx)
    assert torch.equal(_cpu(gdx).double(), PR.global_sum_bwd(dy[live], off_live)), what + " sum dx"


@pytest.mark.parametrize("n,B", NB_SHAPES)
@pytest.mark.parametrize("C", [3, 4, 257, 1028])
def test_global_pools_stay_inside_their_buffers(C, n, B):
    _run_global_pools(n, C, _samples(n, B), C + 4, 4000 + C + n)  # 16-byte lanes where C % 4 == 0


@pytest.mark.parametrize("how", ["pitch", "x", "dx"])
def test_global_pools_at_a_multiple_of_four_channels_on_dword_lanes(how):
    """C % 4 == 0 and still dwords: through a pitch that is no multiple of 4, or through one pointer 4 bytes off."""
    n, B = 300, 1
    _run_global_pools(n, 8, _samples(n, B), 13 if how == "pitch" else 12, 4100, skew_x=4 if how == "x" else 0, skew_dx=4 if how == "dx" else 0)


def test_global_pool_backward_second_trip_of_the_capped_grid():
    """pool.hip caps its flat grids at 65536 workgroups of 256 threads: n x C just above 2^24 on dword lanes (C odd) sends the
    first workgroups round a second time.  The float64 reference is torch's, on the GPU, from the logical operands."""
    L, check = _lib()
    C, B = 257, 3
    n = (1 << 24) // C + 40
    assert n * C > 65536 * 256 and (n - 40) * C <= 65536 * 256
    off = [0, 0, n // 3, n]
    dy = _randn((B, C), 4200)
    goff, gdy = _gin(torch.tensor(off, dtype=torch.int32), name="batch_offsets"), _gin(dy, name="dy")
    gdx = _gout((n, C), name="dx")
    check(L.mink_global_sum_bwd(gdy.ptr, n, C, goff.ptr, B, gdx.ptr, _st()))
    _done(gdy, goff, gdx)
    rows = torch.repeat_interleave(torch.arange(B, device=_dev()), torch.tensor(off, device=_dev()).diff())
    assert torch.equal(gdx.t.double(), dy.to(_dev()).double()[rows])
    arg = torch.stack([torch.full((C,), -1), torch.randint(off[1], off[2], (C,), generator=torch.Generator().manual_seed(1)),
                       torch.randint(off[2], off[3], (C,), generator=torch.Generator().manual_seed(2))]).int()
    gain, gdx = _gin(arg, name="arg"), _gout((n, C), name="dx")
    check(L.mink_global_max_bwd(gdy.ptr, gain.ptr, n, C, goff.ptr, B, gdx.ptr, _st()))
    _done(gdy, gain, goff, gdx)
    ref = torch.zeros(n, C, dtype=torch.float64, device=_dev())
    cols = torch.arange(C, device=_dev())
    for b in (1, 2):
        ref[arg[b].long().to(_dev()), cols] = dy[b].double().to(_dev())
    assert torch.equal(gdx.t.double(), ref)


# ================================================================================================ interpolation
def _hash_table(m, ts):
    """The hash map of level ts of a coordinate manager, copied into guarded inputs of exactly `cap` entries."""
    tkeys, tvals, cap = m.hash_map(ts)
    m._sync_lazy()
    torch.cuda.synchronize()
    assert tkeys.numel() == cap and tvals.numel() == cap
    return _gin(tkeys.clone(), name="table_keys"), _gin(tvals.clone(), name="table_vals"), cap


def _status(expect_written=False):
    """The device status word, zeroed by the caller: an input for in-range queries, written where one is out of range."""
    return Guarded((1,), torch.int32, _dev(), written=expect_written, init=torch.zeros(1, dtype=torch.int32), name="status")


BAD_QUERIES = ([0.0, 1.5, float("nan"), 2.0], [0.0, 32767.5, 0.0, 0.0])


@pytest.mark.parametrize("ts", [1, 2, 4])
def test_interp_map_weight_stays_inside_its_buffers(ts):
    import test_gpu_interp as TI

    L, check = _lib()
    m = TI._manager("B4")
    q = TI._queries("B4")
    n, n_rows = q.shape[0], TI._level_coords("B4", ts).shape[0]
    assert n % 32 != 0  # eight threads per query: the last workgroup is partial
    gk, gv, cap = _hash_table(m, ts)
    rimap, rw = TI._ref_map("B4", ts)
    gq, gimap, gw, gs = _gin(q, name="tfield"), _gout((n, 8), torch.int32, name="imap"), _gout((n, 8), name="w"), _status()
    check(L.mink_interp_map_weight(gq.ptr, n, ts, gk.ptr, gv.ptr, cap, n_rows, gimap.ptr, gw.ptr, gs.ptr, _st()))
    _done(gq, gk, gv, gimap, gw, gs)
    assert torch.equal(gimap.t.cpu().long(), rimap)
    _within(gw.t.cpu(), rw, torch.full_like(rw, 4 * TI.U), f"w ts={ts}")
    # one NaN and one out-of-range row in the middle: the status word is raised, the other rows are what they were
    for bad in BAD_QUERIES:
        qb = torch.cat([q[:40], torch.tensor([bad]), q[40:]])
        gq, gimap2, gw2, gs = _gin(qb, name="tfield"), _gout((n + 1, 8), torch.int32, name="imap"), _gout((n + 1, 8), name="w"), _status(True)
        check(L.mink_interp_map_weight(gq.ptr, n + 1, ts, gk.ptr, gv.ptr, cap, n_rows, gimap2.ptr, gw2.ptr, gs.ptr, _st()))
        _done(gq, gk, gv, gimap2, gw2, gs)
        assert int(gs.t[0]) == MINK_STATUS_RANGE
        keep = torch.arange(n + 1) != 40
        assert torch.equal(gimap2.t.cpu()[keep], gimap.t.cpu()) and torch.equal(gw2.t.cpu()[keep], gw.t.cpu())
        assert_finite(gw2.t.cpu(), "w beside a bad query")


@pytest.mark.parametrize("with_w", [False, True])
def test_splat_coords_stays_inside_its_buffers(with_w):
    import test_gpu_interp as TI

    L, check = _lib()
    q = TI._queries("B4")
    n = q.shape[0]
    b, lo, d = IR.cells(q, 1)
    rc, rw = IR.corner_coords(b, lo, 1).reshape(-1, 4), IR.corner_weights(d).reshape(-1)
    gq, gc, gs = _gin(q, name="tfield"), _gout((8 * n, 4), torch.int32, name="corners"), _status()
    gw = _gout((8 * n,), name="w") if with_w else None
    check(L.mink_splat_coords(gq.ptr, n, gc.ptr, _ptr(gw), gs.ptr, _st()))
    _done(gq, gc, gw, gs)
    assert torch.equal(gc.t.cpu().long(), rc)
    if with_w:
        _within(gw.t.cpu(), rw, torch.full_like(rw, 4 * TI.U), "splat w")
    for bad in BAD_QUERIES:
        qb = torch.cat([q[:40], torch.tensor([bad]), q[40:]])
        gq, gc2, gs = _gin(qb, name="tfield"), _gout((8 * (n + 1), 4), torch.int32, name="corners"), _status(True)
        gw2 = _gout((8 * (n + 1),), name="w") if with_w else None
        check(L.mink_splat_coords(gq.ptr, n + 1, gc2.ptr, _ptr(gw2), gs.ptr, _st()))
        _done(gq, gc2, gw2, gs)
        assert int(gs.t[0]) == MINK_STATUS_RANGE
        keep = torch.arange(8 * (n + 1)) // 8 != 40
        assert torch.equal(gc2.t.cpu()[keep], gc.t.cpu())
        if with_w:
            assert torch.equal(gw2.t.cpu()[keep], gw.t.cpu())
            assert_finite(gw2.t.cpu(), "splat w beside a bad query")


def _run_interp_gather(C, ldx, seed, skew_x=0, skew_y=0, expect_vec=None):
    import test_gpu_interp as TI

    L, check = _lib()
    q = TI._queries("B4")
    n_q, n_x = q.shape[0], TI._level_coords("B4", 2).shape[0]
    rimap, rw = TI._ref_map("B4", 2)
    w32 = rw.float()  # the weights the kernel is handed; the reference multiplies by exactly these
    x = _randn((n_x, C), seed)
    gx, gimap, gw = _gin(x, ld=ldx, name="x", skew=skew_x), _gin(rimap.int(), name="imap"), _gin(w32, name="w")
    gy = _gout((n_q, C), name="y", skew=skew_y)
    if expect_vec is not None:
        assert _vec(C, gx, gy, lds=(ldx,)) == expect_vec
    check(L.mink_interp_gather(gx.ptr, ldx, n_x, C, gimap.ptr, gw.ptr, n_q, gy.ptr, _st()))
    _done(gx, gimap, gw, gy)
    _within(_cpu(gy), IR.interp_fwd(x, rimap, w32.double()), TI._fwd_bound(x, rimap), f"interp gather C={C} ldx={ldx}")
    assert bool((_cpu(gy)[(rimap < 0).all(1)] == 0).all())


@pytest.mark.parametrize("C", [3, 4, 17, 68])
def test_interp_gather_stays_inside_its_buffers(C):
    _run_interp_gather(C, C + 4, 5000 + C, expect_vec=C % 4 == 0)
    _run_interp_gather(C, C + 1, 5001 + C, expect_vec=False)  # a pitch that is no multiple of 4: dwords at any C


@pytest.mark.parametrize("which", ["x", "y"])
def test_interp_gather_with_one_pointer_off_16_bytes_takes_dword_lanes(which):
    _run_interp_gather(8, 12, 5100, expect_vec=False, **{"skew_" + which: 4})


def _pairs_csr(lengths, n_q, seed):
    """(members int64 [P], seg int64 [rows + 1], imap int64 [n_q, 8]): distinct pairs q * 8 + c dealt to segments of the given
    lengths, ascending inside each."""
    g = torch.Generator().manual_seed(seed)
    P = sum(lengths)
    assert P <= 8 * n_q
    pool = torch.randperm(8 * n_q, generator=g)[:P]
    seg = torch.tensor(_offsets(lengths))
    members = torch.cat([pool[seg[r]:seg[r + 1]].sort().values for r in range(len(lengths))]) if P else pool
    imap = torch.full((8 * n_q,), -1, dtype=torch.int64)
    imap[members] = torch.repeat_interleave(torch.arange(len(lengths)), seg.diff())
    return members, seg, imap.reshape(n_q, 8)


SEG_LONG = [0, 1, 256, 257, 600] + [3] * 30 + [0, 7]   # a wave's share ends at 256 pairs: both launches run
SEG_SHORT = [0, 1, 100, 150, 0, 5]                     # 256 pairs in all: the workgroup launch is skipped


def _run_interp_segsum(C, ldy, lengths, seed, skew_dy=0, skew_dx=0, expect_vec=None):
    import test_gpu_interp as TI

    L, check = _lib()
    n_q, n_rows = 203, len(lengths)
    members, seg, imap = _pairs_csr(tuple(lengths), n_q, seed)
    P = members.numel()
    dy = _randn((n_q, C), seed + 1)
    w = torch.rand(n_q, 8, generator=torch.Generator().manual_seed(seed + 2))
    gdy, gw = _gin(dy, ld=ldy, name="dy", skew=skew_dy), _gin(w, name="w")
    gm, gs = _gin(members.int(), name="members"), _gin(seg.int(), name="seg")
    gdx = _gout((n_rows, C), name="dx", skew=skew_dx)
    if expect_vec is not None:
        assert _vec(C, gdy, gdx, lds=(ldy,)) == expect_vec
    check(L.mink_interp_segsum(gdy.ptr, ldy, n_q, C, gw.ptr, gm.ptr, gs.ptr, n_rows, P, gdx.ptr, _st()))
    _done(gdy, gw, gm, gs, gdx)
    what = f"interp segsum C={C} ldy={ldy} pairs={P}"
    _within(_cpu(gdx), IR.interp_bwd(dy, imap, w.double(), n_rows), TI._bwd_bound(dy, imap, n_rows), what)
    assert bool((_cpu(gdx)[torch.tensor(lengths) == 0] == 0).all()), what


@pytest.mark.parametrize("C", [3, 4, 17, 68])  # one slab, one slab, two dword slabs, two 16-byte slabs of kColLanes
def test_interp_segsum_stays_inside_its_buffers(C):
    assert sum(SEG_LONG) > 256 and sum(SEG_SHORT) == 256
    _run_interp_segsum(C, C + 4, SEG_LONG, 5200 + C, expect_vec=C % 4 == 0)
    _run_interp_segsum(C, C + 4, SEG_SHORT, 5300 + C, expect_vec=C % 4 == 0)
    _run_interp_segsum(C, C + 1, SEG_LONG, 5400 + C, expect_vec=False)


@pytest.mark.parametrize("which", ["dy", "dx"])
def test_interp_segsum_with_one_pointer_off_16_bytes_takes_dword_lanes(which):
    _run_interp_segsum(8, 12, SEG_LONG, 5500, expect_vec=False, **{"skew_" + which: 4})


def test_interp_gather_second_trip_of_the_capped_grid():
    """interp.hip caps the flat grid of the gather at 65536 workgroups of 256 threads; n_q x C just above 2^24 on dword lanes."""
    import test_gpu_interp as TI

    L, check = _lib()
    C, n_x = 257, 100
    n_q = (1 << 24) // C + 40
    assert n_q * C > 65536 * 256
    g = torch.Generator().manual_seed(5600)
    x, w = _randn((n_x, C), 5601), torch.rand(n_q, 8, generator=g)
    imap = torch.randint(-1, n_x, (n_q, 8), generator=g)
    gx, gimap, gw, gy = _gin(x, ld=C + 3, name="x"), _gin(imap.int(), name="imap"), _gin(w, name="w"), _gout((n_q, C), name="y")
    check(L.mink_interp_gather(gx.ptr, C + 3, n_x, C, gimap.ptr, gw.ptr, n_q, gy.ptr, _st()))
    _done(gx, gimap, gw, gy)
    xd = torch.cat([x.double(), torch.zeros(1, C, dtype=torch.float64)]).to(_dev())
    imd, wd = torch.where(imap < 0, n_x, imap).to(_dev()), w.double().to(_dev())
    ref, absum = torch.zeros(n_q, C, dtype=torch.float64, device=_dev()), torch.zeros(n_q, C, dtype=torch.float64, device=_dev())
    for k in range(8):
        rows = xd[imd[:, k]]
        ref += wd[:, k, None] * rows
        absum += rows.abs()
    assert bool(torch.isfinite(gy.t).all())
    assert bool(((gy.t.double() - ref).abs() <= 16 * TI.U * absum + TINY).all())


# ================================================================================================ field
@pytest.mark.parametrize("ts", [1, 2, 8, 128])
def test_field_map_stays_inside_its_buffers(ts):
    import test_gpu_point as TP

    L, check = _lib()
    ME, tf, m = TP._field()
    coords = TP._case()[0]
    n = coords.shape[0]
    assert n % 256 != 0 and n > 256
    vox = m.get_coordinates(ME.CoordinateMapKey(ts)).cpu().long()
    gk, gv, cap = _hash_table(m, ts)
    ref = PT.field_map(coords, vox, ts)
    gq, gidx, gs = _gin(coords, name="tfield"), _gout((n,), torch.int32, name="idx"), _status()
    check(L.mink_field_map(gq.ptr, n, ts, gk.ptr, gv.ptr, cap, vox.shape[0], gidx.ptr, gs.ptr, _st()))
    _done(gq, gk, gv, gidx, gs)
    assert torch.equal(gidx.t.cpu().long(), ref) and int(ref.min()) >= 0
    # (32767.5 is in range here: only the floor is looked up, not the corner above it)
    for bad in (BAD_QUERIES[0], [0.0, 0.0, 0.0, 40000.0], [0.0, -40000.5, 0.0, 0.0], [0.0, float("inf"), 0.0, 0.0]):
        qb = torch.cat([coords[:40], torch.tensor([bad]), coords[40:], torch.tensor([[7.0, 1.0, 1.0, 1.0]])])
        gq, gidx2, gs = _gin(qb, name="tfield"), _gout((n + 2,), torch.int32, name="idx"), _status(True)
        check(L.mink_field_map(gq.ptr, n + 2, ts, gk.ptr, gv.ptr, cap, vox.shape[0], gidx2.ptr, gs.ptr, _st()))
        _done(gq, gk, gv, gidx2, gs)
        assert int(gs.t[0]) == MINK_STATUS_RANGE
        got = gidx2.t.cpu().long()
        assert torch.equal(torch.cat([got[:40], got[41:-1]]), ref) and int(got[-1]) == -1  # (a batch index without voxels finds nothing)


def _host_array(ctype, values):
    return (ctype * len(values))(*values)


def _run_field_gather_cat(widths, pads, ldy_extra, seed, skew_src=None, skew_y=0, expect_vec=None):
    L, check = _lib()
    n = 301
    g = torch.Generator().manual_seed(seed)
    rows = [40 + 13 * s for s in range(len(widths))]
    xs = [_randn((r, c), seed + 1 + s) for s, (r, c) in enumerate(zip(rows, widths))]
    idxs = [torch.randint(-2, r + 2, (n,), generator=g) for r in rows]  # -2, -1 and rows, rows + 1: zeros in that source's columns
    ldxs = [c + p for c, p in zip(widths, pads)]
    gxs = [_gin(x, ld=ld, name=f"x[{s}]", skew=4 if s == skew_src else 0) for s, (x, ld) in enumerate(zip(xs, ldxs))]
    gis = [_gin(i.int(), name=f"idx[{s}]") for s, i in enumerate(idxs)]
    total = sum(widths)
    ldy = total + ldy_extra
    gy = _gout((n, ldy), cols=total, name="y", skew=skew_y)  # the pad columns of y stay untouched
    if expect_vec is not None:
        assert (all(c % 4 == 0 for c in widths) and _vec(4, gy, *gxs, lds=[ldy] + ldxs)) == expect_vec
    check(L.mink_field_gather_cat(len(widths), _host_array(ctypes.c_void_p, [g_.ptr for g_ in gxs]), _host_array(ctypes.c_int32, ldxs),
                                  _host_array(ctypes.c_int64, rows), _host_array(ctypes.c_int32, widths),
                                  _host_array(ctypes.c_void_p, [g_.ptr for g_ in gis]), n, gy.ptr, ldy, _st()))
    _done(gy, *gxs, *gis)
    ref = torch.cat([PT.gather_fwd(x, torch.where((i >= 0) & (i < r), i, -1)) for x, i, r in zip(xs, idxs, rows)], 1)
    assert_finite(_cpu(gy), "field_gather_cat")
    assert torch.equal(_cpu(gy).double(), ref), (widths, ldxs, ldy)


@pytest.mark.parametrize("n_src", [1, 4, 8])
def test_field_gather_cat_stays_inside_its_buffers(n_src):
    widths = [12, 16, 4, 32, 8, 24, 4, 20][:n_src]
    _run_field_gather_cat(widths, [4] * n_src, 4, 6000 + n_src, expect_vec=True)
    odd = list(widths)
    odd[n_src // 2] += 1  # one odd width: everything falls to dwords
    _run_field_gather_cat(odd, [4] * n_src, 4, 6010 + n_src, expect_vec=False)
    _run_field_gather_cat(widths, [4] * n_src, 5, 6020 + n_src, expect_vec=False)  # ldy % 4 != 0
    _run_field_gather_cat(widths, [4] * (n_src - 1) + [1], 4, 6030 + n_src, expect_vec=False)  # one source pitch % 4 != 0


@pytest.mark.parametrize("which", ["y", "last source"])
def test_field_gather_cat_with_one_pointer_off_16_bytes_takes_dword_lanes(which):
    _run_field_gather_cat([12, 16, 4, 32], [4] * 4, 4, 6100, skew_src=3 if which == "last source" else None, skew_y=4 if which == "y" else 0,
                          expect_vec=False)


def _run_segment_mean_bwd(C, ldy, lddx, seed, skew_dy=0, skew_dx=0, expect_vec=None):
    L, check = _lib()
    n_in, n_out, named, behind = 301, 50, 220, 11
    g = torch.Generator().manual_seed(seed)
    perm = torch.randperm(n_in, generator=g)
    cuts = torch.cat([torch.tensor([0, 0]), torch.randint(0, named + 1, (n_out - 3,), generator=g).sort().values, torch.tensor([named, named])])
    members = torch.cat([perm[cuts[u]:cuts[u + 1]].sort().values for u in range(n_out)] + [perm[named:named + behind]])
    assert cuts.numel() == n_out + 1 and members.numel() == named + behind and int((cuts.diff() == 0).sum()) >= 2
    dy = _randn((n_out, C), seed + 1)
    gdy = _gin(dy, ld=ldy, name="dy", skew=skew_dy)
    gm, gs = _gin(members.int(), name="members"), _gin(cuts.int(), name="seg")
    hit = torch.zeros(n_in, dtype=torch.bool)
    hit[perm[:named]] = True
    # rows of dx that no segment names (the members behind seg[n_out] among them) and the pad columns keep the sentinel
    gdx = _gout((n_in, lddx), cols=C, written=hit[:, None].expand(n_in, C), name="dx", skew=skew_dx)
    if expect_vec is not None:
        assert _vec(C, gdy, gdx, lds=(ldy, lddx)) == expect_vec
    check(L.mink_segment_mean_bwd(gdy.ptr, ldy, C, gm.ptr, gs.ptr, n_out, members.numel(), n_in, gdx.ptr, lddx, _st()))
    _done(gdy, gm, gs, gdx)
    inverse = torch.repeat_interleave(torch.arange(n_out), cuts.diff())
    ref = PT.mean_bwd(dy, inverse, n_out)  # row j of ref belongs to dx[members[j]]
    got = _cpu(gdx)[members[:named]]
    assert_finite(got, "segment_mean_bwd")
    assert bool(((got.double() - ref).abs() <= 2.0 ** -23 * ref.abs()).all())  # one rounding of the division (test_gpu_point)


@pytest.mark.parametrize("C", [3, 4, 36])
def test_segment_mean_bwd_stays_inside_its_buffers(C):
    _run_segment_mean_bwd(C, C + 4, C + 8, 6200 + C, expect_vec=C % 4 == 0)
    _run_segment_mean_bwd(C, C + 4, C + 1, 6210 + C, expect_vec=False)
    _run_segment_mean_bwd(C, C + 1, C + 4, 6220 + C, expect_vec=False)


@pytest.mark.parametrize("which", ["dy", "dx"])
def test_segment_mean_bwd_with_one_pointer_off_16_bytes_takes_dword_lanes(which):
    _run_segment_mean_bwd(8, 12, 12, 6300, expect_vec=False, **{"skew_" + which: 4})


@pytest.mark.parametrize("C", [1, 3, 4, 20, 65])
def test_rows_gather_stays_inside_its_buffers(C):
    L, check = _lib()
    n_src, n = 57, 301
    for ldx, skew in ((C + 4, 0), (C + 1, 0), (C + 4, 4)):
        g = torch.Generator().manual_seed(6400 + C + ldx)
        x = _randn((n_src, C), 6401 + C)
        idx = torch.randint(-2, n_src + 2, (n,), generator=g)
        gx, gi, gy = _gin(x, ld=ldx, name="x", skew=skew), _gin(idx.int(), name="idx"), _gout((n, C), name="y", skew=skew)
        check(L.mink_rows_gather(gx.ptr, ldx, n_src, C, gi.ptr, n, gy.ptr, _st()))
        _done(gx, gi, gy)
        assert_finite(_cpu(gy), "rows_gather")
        assert torch.equal(_cpu(gy).double(), PT.gather_fwd(x, torch.where((idx >= 0) & (idx < n_src), idx, -1)))


def test_field_gather_cat_second_trip_of_the_capped_grid():
    """field.hip caps its flat grids at 65536 workgroups of 256 threads; n x width just above 2^24 on dword lanes."""
    L, check = _lib()
    C, rows = 257, 100
    n = (1 << 24) // C + 40
    assert n * C > 65536 * 256
    x = _randn((rows, C), 6500)
    idx = torch.randint(-1, rows + 1, (n,), generator=torch.Generator().manual_seed(6501))
    gx, gi, gy = _gin(x, ld=C + 3, name="x"), _gin(idx.int(), name="idx"), _gout((n, C + 2), cols=C, name="y")
    check(L.mink_field_gather_cat(1, _host_array(ctypes.c_void_p, [gx.ptr]), _host_array(ctypes.c_int32, [C + 3]), _host_array(ctypes.c_int64, [rows]),
                                  _host_array(ctypes.c_int32, [C]), _host_array(ctypes.c_void_p, [gi.ptr]), n, gy.ptr, C + 2, _st()))
    _done(gx, gi, gy)
    xd = torch.cat([x, torch.zeros(1, C)]).to(_dev())
    ref = xd[torch.where((idx >= 0) & (idx < rows), idx, rows).to(_dev())]
    assert torch.equal(gy.logical().double(), ref.double())


def test_rows_gather_second_trip_of_the_capped_grid():
    """mink_rows_gather caps its grid at 8192 workgroups of 256 threads: n x C just above 2^21."""
    L, check = _lib()
    C, n_src = 3, 100
    n = (1 << 21) // C + 40
    assert n * C > 8192 * 256
    x = _randn((n_src, C), 6600)
    idx = torch.randint(-1, n_src + 1, (n,), generator=torch.Generator().manual_seed(6601))
    gx, gi, gy = _gin(x, ld=C + 2, name="x"), _gin(idx.int(), name="idx"), _gout((n, C), name="y")
    check(L.mink_rows_gather(gx.ptr, C + 2, n_src, C, gi.ptr, n, gy.ptr, _st()))
    _done(gx, gi, gy)
    xd = torch.cat([x, torch.zeros(1, C)]).to(_dev())
    ref = xd[torch.where((idx >= 0) & (idx < n_src), idx, n_src).to(_dev())]
    assert torch.equal(gy.t.double(), ref.double())
