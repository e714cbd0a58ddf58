"""No GPU: the footprint helper (tests/footprint.py) on torch itself, and every float64 restatement that
tests/test_gpu_nonfinite.py uses as a reference held to torch's rules for non-finite values -- ReLU keeps a NaN, a maximum
returns it with the first NaN in scan order as the arg, a masked gradient is 0 whatever the incoming gradient holds, a row an
operator leaves out contributes nothing whatever it holds."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dgcnn_restate as DR
import footprint as FP
import interp_restate as IR
import norm_restate as NR
import pool_restate as PR
import seghead_restate as SH

VALUES = list(FP.POISONS)
F64 = torch.float64


def _x(n, C, seed):
    return torch.randn(n, C, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ the helper itself
def test_poison_pattern():
    assert FP.poison_rows(130) == [0, 63, 64, 129] and FP.poison_rows(64) == [0, 63] and FP.poison_rows(1) == [0]
    assert FP.poison_rows(10, extra=[7]) == [0, 7, 9]
    assert FP.poison_channels(64) == [0, 3, 63] and FP.poison_channels(3) == [0] and FP.poison_channels(1) == [0]
    assert FP.poison_channels(4) == [0, 3] and FP.poison_channels(7) == [0, 3, 6]
    for C in range(1, 80):
        assert 1 <= len(FP.poison_channels(C)) <= max(1, C // 2)
    x = _x(130, 8, 0)
    p = FP.poison(x, float("nan"), FP.poison_rows(130))
    assert int(FP.footprint(p).sum()) == 4 * 3 and bool(torch.isfinite(x).all())
    assert torch.equal(FP.footprint(p).nonzero()[:, 0].unique(), torch.tensor([0, 63, 64, 129]))


@pytest.mark.parametrize("value", VALUES)
def test_helper_on_torch_pointwise_and_maxima(value):
    v = FP.POISONS[value]
    x = FP.poison(_x(130, 8, 1), v, FP.poison_rows(130))
    for name, fn in (("relu", torch.relu), ("leaky_relu", lambda t: F.leaky_relu(t, 0.2)), ("gelu", F.gelu)):
        ref = fn(x.double())
        if value != "-inf" or name == "leaky_relu":
            FP.visible({name: ref}, name)
        # (torch's vectorised fp32 gelu on the CPU returns NaN at +inf where x * cdf is inf: its float64 form rounded is `got`)
        got = ref.float() if name == "gelu" else fn(x)
        FP.same_footprint(got, ref, dict(atol=1e-6, rtol=1e-6), name)
    # maxima over the rows, over windows of 4 rows, and with indices: NaN wins, the first NaN is the arg
    ref = x.double().amax(0)
    FP.same_footprint(x.amax(0), ref, None, "amax")
    win, idx = F.max_pool1d(x.double().t()[None], 4, return_indices=True)
    win32, idx32 = F.max_pool1d(x.t()[None], 4, return_indices=True)
    FP.same_footprint(win32[0], win[0], None, "max_pool1d")
    assert torch.equal(idx, idx32)
    if FP.is_nan(v):
        assert bool(torch.isnan(ref[FP.poison_channels(8)]).all()) and bool(torch.isfinite(ref[[1, 2, 4]]).all())
        assert int(x.double().max(0).indices[0]) == 0  # the first NaN of column 0 is row 0
        assert bool(torch.isnan(win[0, 0, 0])) and int(idx[0, 0, 0]) == 0 and int(idx[0, 0, 16]) == 64
        y = x.clone()
        y[0, 0] = 0.0  # ... and with row 0 clean it is row 63, not the largest number before it
        assert int(y.double().max(0).indices[0]) == 63 and int(F.max_pool1d(y.double().t()[None], 64, return_indices=True)[1][0, 0, 0]) == 63


@pytest.mark.parametrize("value", VALUES)
def test_helper_on_torch_batch_norm(value):
    x = FP.poison(_x(130, 8, 2), FP.POISONS[value], FP.poison_rows(130))
    bn64, bn32 = torch.nn.BatchNorm1d(8).double(), torch.nn.BatchNorm1d(8)
    ref, got = torch.relu(bn64(x.double())), torch.relu(bn32(x))
    FP.visible({"y": ref.detach()}, "batch norm")
    assert torch.equal(FP.footprint(ref.detach()).all(0), torch.tensor([c in (0, 3, 7) for c in range(8)]))  # the whole column, no other
    FP.same_footprint(got, ref, dict(atol=1e-5, rtol=1e-5), "batch norm", behind="batch norm")
    FP.same_footprint(bn32.running_mean, bn64.running_mean, dict(atol=1e-6, rtol=0), "running_mean", behind="batch norm")
    FP.same_footprint(bn32.running_var, bn64.running_var, dict(atol=1e-5, rtol=0), "running_var", behind="batch norm")


def test_helper_fails_for_a_swallowed_a_leaked_and_a_changed_value():
    x = FP.poison(_x(130, 8, 3), float("nan"), FP.poison_rows(130))
    ref = torch.relu(x.double())
    with pytest.raises(AssertionError, match="swallowed"):
        FP.same_footprint(torch.fmax(x, torch.zeros(())), ref, None, "a ReLU that drops NaN")  # (fmax: the number wins)
    with pytest.raises(AssertionError):
        FP.no_swallow(torch.fmax(x, torch.zeros(())), ref, "a ReLU that drops NaN")
    leak = torch.relu(x)
    leak[5, 5] = float("nan")
    with pytest.raises(AssertionError, match="1 leaked"):
        FP.same_footprint(leak, ref, None, "a leak")
    FP.no_swallow(leak, ref, "a leak is not a swallow")
    off = torch.relu(x)
    off[5, 5] += 1e-3
    with pytest.raises(AssertionError, match="finite elements"):
        FP.same_footprint(off, ref, dict(atol=1e-6, rtol=1e-6), "a wrong number")
    xi = FP.poison(_x(130, 8, 3), float("inf"), FP.poison_rows(130))
    with pytest.raises(AssertionError, match="another non-finite"):
        FP.same_footprint(torch.where(torch.isinf(xi), torch.full_like(xi, float("nan")), xi), xi.double(), None, "inf -> nan")
    FP.same_footprint(torch.where(torch.isinf(xi), torch.full_like(xi, float("nan")), xi), xi.double(), None, "inf -> nan", behind="bf16x3")
    with pytest.raises(AssertionError, match="exception classes"):
        FP.same_footprint(xi, xi.double(), None, "free flag", behind="because")
    with pytest.raises(AssertionError, match="no reference footprint"):
        FP.visible({"clean": _x(4, 4, 0).double()}, "nothing poisoned")
    with pytest.raises(AssertionError, match="no reference footprint"):
        FP.visible({"all": torch.full((4, 4), float("nan"), dtype=F64)}, "everything poisoned")
    with pytest.raises(AssertionError, match="is empty"):
        FP.visible_reduction({"clean": _x(4, 4, 0).double()}, "nothing poisoned")
    r = FP.Reached(["a", "b"])
    r.reach("a")
    with pytest.raises(AssertionError, match="not reached"):
        r.finish("forms")
    with pytest.raises(AssertionError):
        FP.untouched(leak, torch.relu(x), torch.isfinite(ref), "leak")


# ------------------------------------------------------------------------------------------------ pool_restate
def _table(m, K, n_in, seed, unnamed):
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, n_in, (m, K), generator=g)
    t[torch.rand(m, K, generator=g) < 0.4] = -1
    t[t == unnamed] = -1
    t[5] = -1  # a window without entries
    return t


@pytest.mark.parametrize("value", VALUES)
def test_pool_restatement_follows_torch(value):
    v = FP.POISONS[value]
    n, C, K, unnamed = 130, 8, 8, 77
    table = _table(90, K, n, 4, unnamed)
    rows = FP.poison_rows(n, extra=[unnamed])
    x = FP.poison(_x(n, C, 5), v, rows)
    y, arg = PR.max_fwd(x, table)
    # torch: max_pool1d over the window's present rows, absent ones filled with -inf (they never win against a present row)
    filled = torch.cat([x.double(), torch.full((1, C), -float("inf"), dtype=F64)])[table]  # [m, K, C]
    ty = F.max_pool1d(filled.permute(0, 2, 1), K)[:, :, 0]
    tmax = filled.max(1)  # (max(dim) gives the FIRST NaN's index, the rule here; max_pool1d's own index is the last NaN's)
    assert bool(((tmax.values == ty) | (torch.isnan(tmax.values) & torch.isnan(ty))).all())
    tj = tmax.indices
    live = PR.counts(table) > 0
    assert torch.equal(FP.footprint(y), FP.footprint(torch.where(live[:, None], ty, torch.zeros_like(ty)))) or value == "-inf"
    eq = (y == ty) | (torch.isnan(y) & torch.isnan(ty))
    assert bool(eq[live].all())
    if value != "-inf":  # (an absent -inf filler ties with a poisoned -inf: torch's index may then be the filler's)
        assert torch.equal(arg[live], torch.gather(table, 1, tj)[live])
    assert bool((y[~live] == 0).all()) and bool((arg[~live] == -1).all())
    named = (table[:, :, None] == arg[:, None, :]).any(1)
    assert bool(named[live].all())  # the arg is always a row of the window
    if FP.is_nan(v):
        FP.visible({"y": y}, "max pool")
        pc = FP.poison_channels(C)
        expect = torch.zeros(90, C, dtype=torch.bool)
        expect[:, pc] = torch.isin(table, torch.tensor([r for r in rows if r != unnamed])).any(1)[:, None]
        assert torch.equal(FP.footprint(y), expect)  # exactly the windows that name a poisoned row; the unnamed row nowhere
    dy = FP.poison(_x(90, C, 6), v, FP.poison_rows(90))
    clean = PR.max_fwd(_x(n, C, 5), table)[1]
    xa = _x(n, C, 5).double().requires_grad_(True)
    PR.max_fwd_forced(xa, clean).backward(dy.double())
    dx = PR.max_bwd(dy, clean, table, n)
    assert torch.equal(FP.footprint(dx), FP.footprint(xa.grad))
    # sums and averages: torch's own index_add / sum, checked for where the poison goes
    for fn in (PR.sum_fwd, PR.avg_fwd):
        s = fn(x, table)
        expect = torch.zeros(90, C, dtype=torch.bool)
        expect[:, FP.poison_channels(C)] = torch.isin(table, torch.tensor([r for r in rows if r != unnamed])).any(1)[:, None]
        assert torch.equal(FP.footprint(s), expect)
    for fn in (PR.sum_bwd, PR.avg_bwd):
        d = fn(dy, table, n)
        expect = torch.zeros(n, C, dtype=torch.bool)
        hit = torch.zeros(n, dtype=torch.bool)
        for o in FP.poison_rows(90):
            hit[table[o][table[o] >= 0]] = True
        expect[:, FP.poison_channels(C)] = hit[:, None]
        assert torch.equal(FP.footprint(d), expect)


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("where", ["first", "middle", "last"])
def test_global_max_restatement_follows_torch(value, where):
    v = FP.POISONS[value]
    off = [0, 257, 257, 258, 388]
    x = _x(388, 8, 7)
    row = {"first": 0, "middle": 100, "last": 256}[where]
    x[row, 2] = v
    x[300, 5] = v
    x[320, 5] = v  # two in one column: the first is the arg
    y, arg = PR.global_max_fwd(x, off)
    for b in range(4):
        seg = x[off[b]:off[b + 1]].double()
        if seg.shape[0] == 0:
            assert bool((y[b] == 0).all()) and bool((arg[b] == -1).all())
            continue
        t = seg.max(0)
        assert bool(((y[b] == t.values) | (torch.isnan(y[b]) & torch.isnan(t.values))).all())
        assert torch.equal(arg[b], t.indices + off[b])
    if FP.is_nan(v):
        assert bool(torch.isnan(y[0, 2])) and int(arg[0, 2]) == row and bool(torch.isnan(y[3, 5])) and int(arg[3, 5]) == 300
        assert int(FP.footprint(y).sum()) == 2
    for fn in (PR.global_sum_fwd, PR.global_avg_fwd):
        s = fn(x, off)
        assert FP.footprint(s).nonzero().tolist() == [[0, 2], [3, 5]]


# ------------------------------------------------------------------------------------------------ norm_restate
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("relu,residual", [(False, False), (True, False), (True, True)])
def test_norm_restatement_follows_torch(value, relu, residual):
    v = FP.POISONS[value]
    sizes = [0, 70, 1, 0, 41, 64, 65]
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    n, C, eps = off[-1], 8, 1e-5
    g = torch.Generator().manual_seed(8)
    x, dy, res = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g), torch.randn(n, C, generator=g)
    gamma, beta = torch.linspace(0.5, 1.5, C), torch.linspace(-0.2, 0.2, C)
    s1 = slice(off[1], off[2])  # the poisoned sample
    xp = x.clone()
    xp[s1] = FP.poison(x[s1], v, FP.poison_rows(70))
    r = res if residual else None

    def torch_in(xx):
        out = torch.empty_like(xx)
        for b in range(len(sizes)):
            seg = xx[off[b]:off[b + 1]]
            if seg.shape[0] == 1:  # (torch refuses one row; variance 0, xhat 0)
                out[off[b]:off[b + 1]] = seg - seg
            elif seg.shape[0]:
                out[off[b]:off[b + 1]] = F.instance_norm(seg.t()[None], eps=eps)[0].t()
        z = out * gamma.double() + beta.double()
        z = z + r.double() if residual else z
        return torch.relu(z) if relu else z

    def torch_ln(xx):
        z = F.layer_norm(xx, (C,), gamma.double(), beta.double(), eps)
        z = z + r.double() if residual else z
        return torch.relu(z) if relu else z

    # (a) poisoned input, forward
    y = NR.instance_norm_fwd(xp, off, gamma, beta, eps, r, relu)
    ty = torch_in(xp.double())
    assert torch.equal(FP.footprint(y), FP.footprint(ty))
    FP.visible({"y": y}, "instance norm")
    expect = torch.zeros(n, C, dtype=torch.bool)
    expect[s1, :] = torch.tensor([c in FP.poison_channels(C) for c in range(C)])
    assert torch.equal(FP.footprint(y), expect)  # the sample's column; every other sample and column finite
    yl = NR.layer_norm_fwd(xp, gamma, beta, eps, r, relu)
    assert torch.equal(FP.footprint(yl), FP.footprint(torch_ln(xp.double())))
    assert torch.equal(FP.footprint(yl).all(1), FP.footprint(yl).any(1)) and int(FP.footprint(yl).any(1).sum()) == 4  # whole rows
    # (b) clean forward, poisoned gradient
    dyp = dy.clone()
    dyp[s1] = FP.poison(dy[s1], v, FP.poison_rows(70))
    for fwd, bwd in ((torch_in, lambda: NR.instance_norm_bwd(dyp, x, off, gamma, beta, eps, r, relu)),
                     (torch_ln, lambda: NR.layer_norm_bwd(dyp, x, gamma, beta, eps, r, relu))):
        xa = x.double().requires_grad_(True)
        fwd(xa).backward(dyp.double())
        dx, dga, dbe, dres = bwd()
        assert torch.equal(FP.footprint(dx), FP.footprint(xa.grad))
        if relu:  # a masked element's gradient is 0 whatever arrives (torch's threshold_backward), not 0 x NaN
            masked = fwd(x.double()) <= 0
            assert bool((dres[masked] == 0).all())


# ------------------------------------------------------------------------------------------------ interp_restate
@pytest.mark.parametrize("value", VALUES)
def test_interp_restatement_lets_the_poison_through_the_named_pairs_only(value):
    v = FP.POISONS[value]
    g = torch.Generator().manual_seed(9)
    side = 6
    cell = torch.randperm(side ** 3, generator=g)[:150]
    coords = torch.stack([torch.zeros(150, dtype=torch.long), cell % side, cell // side % side, cell // (side * side)], 1)
    q = torch.cat([torch.zeros(90, 1), torch.rand(90, 3, generator=g) * (side - 1)], 1)
    q[:10, 1:] = q[:10, 1:].floor()  # queries on a voxel: seven corners of weight 0
    imap, w = IR.map_weight(coords, 1, q)
    named = torch.zeros(150, dtype=torch.bool)
    named[imap[imap >= 0]] = True
    unnamed = [int(i) for i in (~named).nonzero().flatten()[:1]]
    rows = FP.poison_rows(150, extra=unnamed)
    x = FP.poison(_x(150, 8, 10), v, rows)
    y = IR.interp_fwd(x, imap, w)
    hit = torch.isin(imap, torch.tensor([r for r in rows if bool(named[r])])).any(1)
    expect = torch.zeros(90, 8, dtype=torch.bool)
    expect[:, FP.poison_channels(8)] = hit[:, None]
    assert torch.equal(FP.footprint(y), expect)  # also through a present corner of weight 0: 0 x NaN, as the kernels multiply
    xa = _x(150, 8, 10).double().requires_grad_(True)
    dy = FP.poison(_x(90, 8, 11), v, FP.poison_rows(90))
    IR.interp_fwd(xa, imap, w).backward(dy.double())
    assert torch.equal(FP.footprint(IR.interp_bwd(dy, imap, w, 150)), FP.footprint(xa.grad))
    assert torch.equal(FP.footprint(IR.splat_fwd(dy, imap, w, 150)), FP.footprint(xa.grad))


# ------------------------------------------------------------------------------------------------ seghead_restate
@pytest.mark.parametrize("value", VALUES)
def test_seghead_restatement_follows_torch(value):
    v = FP.POISONS[value]
    z, labels, w = SH.make_case(130, 7, 12, ignore=255, weighted=True)
    labels[[0, 64]] = 255
    labels[[63, 129]] = [2, 3]
    wt = torch.from_numpy(w).double()

    def torch_ce(zz):
        zt = torch.from_numpy(zz).double().requires_grad_(True)
        loss = F.cross_entropy(zt, torch.from_numpy(labels), weight=wt, ignore_index=255)
        loss.backward()
        return float(loss), zt.grad.numpy()

    for rows, finite in (([0, 64], True), ([63], False), ([129], False)):
        zp = z.copy()
        zp[rows, 3] = v
        got = SH.ce(zp, labels, w, 255)
        tl, tg = torch_ce(zp)
        if finite:  # an ignored row: the loss does not see it, its gradient is 0
            assert np.isfinite(got["loss"]) and np.isfinite(tl) and abs(got["loss"] - tl) < 1e-12
            assert np.isfinite(got["grad"]).all() and (got["grad"][rows] == 0).all()
        else:
            assert not np.isfinite(got["loss"]) or value == "-inf"
            assert np.isfinite(got["loss"]) == np.isfinite(tl)
        if not finite:  # (for a row it leaves out torch writes 0 x NaN; the restatement and the kernels write 0)
            assert np.array_equal(np.isfinite(got["grad"]), np.isfinite(tg))
        pred = SH.argmax_first(zp)
        assert ((pred >= 0) & (pred < 7)).all()
        assert np.array_equal(pred, torch.from_numpy(zp).double().argmax(1).numpy())


# ------------------------------------------------------------------------------------------------ dgcnn_restate (edge maximum)
@pytest.mark.parametrize("value", VALUES)
def test_edge_maximum_restatement_follows_torch(value):
    v = FP.POISONS[value]
    z = _x(40, 6 * 5, 13).reshape(40, 6, 5).double()
    z[0, 2, 1] = z[0, 4, 1] = v
    z[39, 0, 4] = v
    z[7, 5, 0] = v
    arg = DR.first_argmax(z)
    t = z.max(1)
    assert torch.equal(arg, t.indices)
    if FP.is_nan(v):
        assert int(arg[0, 1]) == 2 and int(arg[39, 4]) == 0 and int(arg[7, 0]) == 5
    assert bool(((arg >= 0) & (arg < 6)).all())
    y = DR.lrelu(z.gather(1, arg[:, None, :])[:, 0, :])
    assert torch.equal(FP.footprint(y), FP.footprint(F.leaky_relu(t.values, 0.2)))
    # the whole layer: a poisoned feature row reaches every edge that uses it and, through the batch statistics, its columns
    g = torch.Generator().manual_seed(14)
    x = torch.randn(30, 4, generator=g).double()
    W = torch.randn(8, 8, generator=g).double()
    idx = DR.knn(x, [0, 30], 5)
    mean, var = torch.zeros(8, dtype=F64), torch.ones(8, dtype=F64)
    xp = x.clone()
    xp[3, 1] = v
    y, arg, _ = DR.edge_conv(xp, W, torch.ones(8, dtype=F64), torch.zeros(8, dtype=F64), idx, stats=(mean, var))
    uses = (idx == 3).any(1)
    uses[3] = True
    assert torch.equal(FP.footprint(y).any(1), uses) and bool(((arg >= 0) & (arg < 5)).all())


# ------------------------------------------------------------------------------------------------ _gather64 / _wgrad64
@pytest.mark.parametrize("value", VALUES)
def test_conv_restatements_let_the_poison_through_the_named_rows_only(value):
    import test_gpu_reduced_math as RM

    v = FP.POISONS[value]
    g = torch.Generator().manual_seed(15)
    n_out, K, cin, cout = 130, 8, 8, 6
    n_in = n_out + 17
    nbr = RM._table(n_out, K, n_in, g)
    unnamed = 100
    nbr[nbr == unnamed] = -1
    rows = FP.poison_rows(n_in, extra=[unnamed])
    x = FP.poison(torch.randn(n_in, cin, generator=g), v, rows).double()
    w = torch.randn(K, cin, cout, generator=g).double()
    y = RM._gather64(x, w, nbr)
    hit = torch.isin(nbr, torch.tensor([r for r in rows if r != unnamed])).any(1)
    assert torch.equal(FP.footprint(y), hit[:, None].expand(-1, cout))  # whole rows, of the outputs that name a poisoned row
    FP.visible({"y": y}, "gather")
    # an explicit pair-by-pair sum agrees on the footprint (absent pairs are skipped, not multiplied by zero)
    ref = torch.zeros(n_out, cout, dtype=F64)
    for o in range(n_out):
        for k in range(K):
            if nbr[o, k] >= 0:
                ref[o] += x[nbr[o, k]] @ w[k]
    assert torch.equal(FP.footprint(ref), FP.footprint(y))
    gy = torch.randn(n_out, cout, generator=g).double()
    dw = RM._wgrad64(x, gy, nbr)
    assert K > 1 and bool((nbr[:, K // 2 - 1] == -1).all()) and bool((dw[K // 2 - 1] == 0).all())  # the offset no row has: exactly 0
    expect = torch.zeros(K, cin, cout, dtype=torch.bool)
    for k in range(K):
        if bool(torch.isin(nbr[:, k], torch.tensor([r for r in rows if r != unnamed])).any()):
            expect[k, FP.poison_channels(cin), :] = True
    assert torch.equal(FP.footprint(dw), expect)
    FP.visible_reduction({"dW": dw}, "wgrad")
    gyp = FP.poison(gy.float(), v, FP.poison_rows(n_out)).double()
    dw = RM._wgrad64(torch.randn(n_in, cin, generator=g).double(), gyp, nbr)
    expect = torch.zeros(K, cin, cout, dtype=torch.bool)
    for k in range(K):
        if bool((nbr[FP.poison_rows(n_out), k] >= 0).any()):
            expect[k, :, FP.poison_channels(cout)] = True
    assert torch.equal(FP.footprint(dw), expect)
