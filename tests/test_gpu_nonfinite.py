"""-m gpu: one NaN, +inf or -inf enters an operator; where it comes out is held to the float64 reference (tests/footprint.py).

Two experiments per operator family: (a) the forward input is poisoned and every forward output checked; (b) the forward runs
clean, the incoming gradient is poisoned at the same row / channel pattern and every gradient output checked.  What is checked:
  * a value the reference lets through comes through (fmaxf(x, 0) as ReLU and `v > m` as a maximum drop a NaN: the training
    loops' finite-loss guard then never fires);
  * a value in a row the operator's table does not name, in a pad column, in another sample or another column appears nowhere
    (0 x NaN is NaN: a clamped re-read of row 0, a `live ? o : n - 1` row or a zero-weight multiply would show);
  * the finite elements still meet the tolerance of the operator's existing test, imported from it (where that test states its
    tolerance as a literal, the literal is repeated here beside the test's name).
A case is one operator form under one poison value, both experiments: before a kernel's result is looked at, at least one of
the case's reference outputs must show the poison in less than half of its elements (a maximum or a ReLU absorbs -inf, so
there the gradient experiment is the visible one).
Weights and query coordinates are never poisoned, and nothing that turns data into an address by comparing it (kNN selection,
coordinate / voxel / augmentation kernels) is run poisoned.  The three kernels that do derive an index from a comparison of
features start from a valid entry and only ever replace it by another valid one (pool arg: -1 or a row of the window; edge
`at`: slot 0 .. k - 1; segmentation `pred`: column 0 .. C - 1), so the index stays in range when every comparison is false."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dgcnn_restate as DR
import footprint as FP
import interp_restate as IR
import layerwise as LW
import norm_restate as NR
import pool_restate as PR
import seghead_restate as SH
from helpers import batch_scenes, trunk_node

pytestmark = pytest.mark.gpu

VALUES = list(FP.POISONS)
F64 = torch.float64


def _randn(n, C, seed):
    return torch.randn(n, C, generator=torch.Generator().manual_seed(seed))


def _st():
    return torch.cuda.current_stream().cuda_stream


def _cols(C, poisoned):
    """bool [C]: the columns the poison cannot reach."""
    keep = torch.ones(C, dtype=torch.bool)
    keep[list(poisoned)] = False
    return keep


# ================================================================================================ ReLU, add, activations
COUNTS = [1, 5, 1027]  # scalar tail only, tail only with a second poisoned element, vector body + tail


def _flat_poison(t, v):
    out = t.clone()
    for i in (0, 3, 63, 64, t.numel() - 1):
        if i < t.numel():
            out[i] = v
    return out


@pytest.mark.parametrize("value", VALUES)
def test_relu_masked_gradient_and_add(value):
    """mink_eltwise modes 0 (ReLU), 1 (its gradient: gy where y > 0) and 2 (add) at counts 1, 5, 1027."""
    from nerf_downstream_amd.minkowski.eltwise import _eltwise

    v = FP.POISONS[value]
    reached = FP.Reached([f"mode {m} count {c}" for m in (0, 1, 2) for c in COUNTS])
    refs = {}
    for count in COUNTS:
        a, b = _randn(count, 1, 10 + count)[:, 0], _randn(count, 1, 20 + count)[:, 0]
        ap = _flat_poison(a, v)
        # (a) poisoned activation through ReLU and the add
        ref = torch.relu(ap.double())
        refs[f"relu {count}"] = ref
        y = _eltwise(ap.cuda(), None, 0)
        FP.same_footprint(y, ref, None, f"relu count {count}")
        reached.reach(f"mode 0 count {count}")
        ref = ap.double() + b.double()  # (the sum of two floats is exact in double)
        refs[f"add {count}"] = ref
        FP.same_footprint(_eltwise(ap.cuda(), b.cuda(), 2), ref.float(), None, f"add count {count}")
        FP.same_footprint(_eltwise(b.cuda(), ap.cuda(), 2), ref.float(), None, f"add (second operand) count {count}")
        reached.reach(f"mode 2 count {count}")
        # (b) clean forward, poisoned gradient; and the mask of a poisoned activation is 0, as torch's threshold_backward has it
        yc = torch.relu(a)
        ref = torch.where(yc.double() > 0, ap.double(), torch.zeros((), dtype=F64))
        refs[f"relu gradient {count}"] = ref
        FP.same_footprint(_eltwise(ap.cuda(), yc.cuda(), 1), ref, None, f"relu gradient count {count}")
        ref = torch.where(y.cpu().double() > 0, b.double(), torch.zeros((), dtype=F64))
        FP.same_footprint(_eltwise(b.cuda(), y, 1), ref, None, f"relu gradient under a poisoned activation, count {count}")
        reached.reach(f"mode 1 count {count}")
    FP.visible(refs, f"eltwise {value}")
    reached.finish(f"eltwise {value}")


ACT_TOL = dict(atol=2e-6, rtol=1e-5)  # tests/test_gpu_compat.py, the activation modules against torch
ACTS = [("leaky_relu", 0.2, lambda x, w: F.leaky_relu(x, 0.2)), ("elu", 0.7, lambda x, w: F.elu(x, 0.7)),
        ("celu", 1.3, lambda x, w: F.celu(x, 1.3)), ("selu", 0.0, lambda x, w: F.selu(x)), ("gelu", 0.0, lambda x, w: F.gelu(x)),
        ("prelu", 0.0, lambda x, w: F.prelu(x, w))]


@pytest.mark.parametrize("value", VALUES)
def test_activations(value):
    """mink_activation, all six kinds, forward and backward, on [130, 8] (and [5, 1]: fewer elements than one wave)."""
    from nerf_downstream_amd.minkowski import functional as Fn

    v = FP.POISONS[value]
    reached = FP.Reached([k for k, _, _ in ACTS])
    for kind, alpha, fn in ACTS:
        refs = {}
        for n, C in ((130, 8), (5, 1)):
            x, gy = _randn(n, C, 30 + n), _randn(n, C, 40 + n)
            slope = torch.linspace(0.1, 0.4, C) if kind == "prelu" else None
            rows = FP.poison_rows(n)
            xp, gyp = FP.poison(x, v, rows), FP.poison(gy, v, rows)
            sd = slope.cuda() if slope is not None else None
            s64 = slope.double() if slope is not None else None
            # (a)
            ref = fn(xp.double(), s64)
            refs[f"y {n}"] = ref
            FP.same_footprint(Fn.ActivationFunction.apply(xp.cuda(), kind, alpha, sd), ref, ACT_TOL, f"{kind} forward [{n}, {C}]")
            # (b)
            xd = x.clone().cuda().requires_grad_(True)
            sl = sd.clone().requires_grad_(True) if sd is not None else None
            Fn.ActivationFunction.apply(xd, kind, alpha, sl).backward(gyp.cuda())
            x64 = x.double().requires_grad_(True)
            w64 = s64.clone().requires_grad_(True) if s64 is not None else None
            fn(x64, w64).backward(gyp.double())
            refs[f"dx {n}"] = x64.grad
            FP.same_footprint(xd.grad, x64.grad, ACT_TOL, f"{kind} backward [{n}, {C}]")
            if sl is not None:  # a column sum of gy * min(x, 0): the row-reduction form
                FP.no_swallow(sl.grad, w64.grad, f"prelu slope gradient [{n}, {C}]")
        FP.visible(refs, f"{kind} {value}")
        reached.reach(kind)
    reached.finish(f"activations {value}")


# ================================================================================================ batch norm
# tolerances of tests/test_gpu_ops.py test_batch_norm (module) and test_one_launch_batch_norm_of_few_row_layers (C entry points)
BN_TOL = {"y": dict(atol=1e-5, rtol=1e-5), "mean": dict(atol=1e-5, rtol=0), "invstd": dict(atol=1e-5, rtol=1e-5),
          "rm": dict(atol=1e-6, rtol=0), "rv": dict(atol=1e-5, rtol=0), "dx": dict(atol=1e-5, rtol=1e-4),
          "dgamma": dict(atol=2e-3, rtol=1e-4), "dbeta": dict(atol=2e-3, rtol=1e-4), "dres": dict(atol=1e-6, rtol=0)}
BN_SMALL_TOL = dict(BN_TOL, y=dict(atol=2e-5, rtol=1e-5), dx=dict(atol=2e-4, rtol=0))
BN_FWD, BN_BWD = ("y", "mean", "invstd", "rm", "rv"), ("dx", "dgamma", "dbeta", "dres")


def _bn_ref(x, gamma, beta, res, relu, gy, eps=1e-5, eval_stats=None):
    """torch.nn.BatchNorm1d in float64, + residual, relu; the gradients of `gy`."""
    C = x.shape[1]
    bn = torch.nn.BatchNorm1d(C, eps=eps).double()
    with torch.no_grad():
        bn.weight.copy_(gamma.double()), bn.bias.copy_(beta.double())
        if eval_stats is not None:
            bn.running_mean.copy_(eval_stats[0].double()), bn.running_var.copy_(eval_stats[1].double())
    if eval_stats is not None:
        bn.eval()
    x64 = x.double().requires_grad_(True)
    r64 = res.double().requires_grad_(True) if res is not None else None
    z = bn(x64)
    if r64 is not None:
        z = z + r64
    if relu:
        z = torch.relu(z)
    z.backward(gy.double())
    xd = x64.detach()
    mean = xd.mean(0)
    var = ((xd - mean) ** 2).mean(0)
    return {"y": z.detach(), "mean": mean, "invstd": 1.0 / torch.sqrt(var + eps), "rm": bn.running_mean.clone(), "rv": bn.running_var.clone(),
            "dx": x64.grad, "dgamma": bn.weight.grad, "dbeta": bn.bias.grad, "dres": None if r64 is None else r64.grad}


def _bn_experiments(run, n, C, relu, res, value, what, tol, seed, names_fwd=BN_FWD, names_bwd=BN_BWD, eval_stats=None):
    """`run(x, res, gy)` -> {name: host tensor}.  (a) x poisoned: the forward outputs; (b) gy poisoned: the gradients.  In both,
    the columns the poison cannot reach equal the clean run's bit for bit."""
    v = FP.POISONS[value]
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, C, generator=g) * 1.5 + 0.3
    gy = torch.randn(n, C, generator=g)
    r = torch.randn(n, C, generator=g) if res else None
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    rows, pc = FP.poison_rows(n), FP.poison_channels(C)
    keep = _cols(C, pc)
    exps = [["a", FP.poison(x, v, rows), gy, names_fwd], ["b", x, FP.poison(gy, v, rows), names_bwd]]
    seen = {}
    for e in exps:
        ref = _bn_ref(e[1], gamma, beta, r, relu, e[2], eval_stats=eval_stats)
        names = [k for k in e[3] if ref.get(k) is not None]
        if eval_stats is not None:
            names = [k for k in names if k not in ("mean", "invstd", "rm", "rv")]
        e[3] = names
        e.append(ref)
        seen.update({f"({e[0]}) {k}": ref[k] for k in names})
    FP.visible(seen, what)  # (one case = the operator form under one poison value, both experiments)
    clean = run(x, r, gy, gamma, beta)
    for exp, xin, gin, names, ref in exps:
        names = [k for k in names if k in clean]
        got = run(xin, r, gin, gamma, beta)
        for k in names:
            FP.same_footprint(got[k], ref[k], tol[k], f"{what} ({exp}) {k}", behind="batch norm")
            FP.untouched(got[k], clean[k], keep[None, :] if got[k].dim() == 2 else keep, f"{what} ({exp}) {k}")
        if exp == "a" and eval_stats is None:
            for k in names:  # the poisoned column is non-finite in all of it
                col = FP.footprint(got[k])[..., pc]
                assert bool(col.all()), f"{what} (a) {k}: a poisoned column is not non-finite throughout"
        if exp == "b":
            for k in names_fwd:
                if k in clean:
                    assert torch.equal(got[k], clean[k]), f"{what} (b) {k}: the forward saw the gradient"


def _module_run(n, C, relu, res, training=True):
    from nerf_downstream_amd import minkowski as ME

    coords = torch.zeros(n, 4)
    coords[:, 1] = torch.arange(n)
    m = ME.TensorField(coordinates=coords.cuda(), features=torch.zeros(n, 1).cuda()).coordinate_manager
    key = ME.CoordinateMapKey(1)

    def run(x, r, gy, gamma, beta):
        bn = ME.MinkowskiBatchNorm(C).cuda()
        with torch.no_grad():
            bn.bn.weight.copy_(gamma), bn.bn.bias.copy_(beta)
            if not training:
                bn.bn.running_mean.copy_(torch.linspace(-0.3, 0.6, C)), bn.bn.running_var.copy_(torch.linspace(0.5, 2.0, C))
        bn.train(training)
        xg = x.cuda().requires_grad_(True)
        rg = r.cuda().requires_grad_(True) if r is not None else None
        y = bn(ME.SparseTensor(xg, key, m), relu=relu, residual=ME.SparseTensor(rg, key, m) if rg is not None else None).F
        y.backward(gy.cuda())
        out = {"y": y.detach().cpu(), "rm": bn.bn.running_mean.cpu(), "rv": bn.bn.running_var.cpu(), "dx": xg.grad.cpu(),
               "dgamma": bn.bn.weight.grad.cpu(), "dbeta": bn.bn.bias.grad.cpu()}
        if rg is not None:
            out["dres"] = rg.grad.cpu()
        return out

    return run


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("n,C,relu,res", [(300, 48, True, False), (1024, 128, True, True), (1025, 64, True, True), (1025, 64, False, False),
                                          (3001, 1536, True, False)])
def test_batch_norm_module(n, C, relu, res, value):
    """MinkowskiBatchNorm + relu / residual: the one-launch form (n <= mink_bn_small_rows()), the three-launch form at the
    first row count above it, and column slabs through blockIdx.y (C = 1536)."""
    from nerf_downstream_amd._lib import lib

    assert lib().mink_bn_small_rows() == 1024
    _bn_experiments(_module_run(n, C, relu, res), n, C, relu, res, value, f"bn module n={n} C={C}", BN_TOL, 50 + n)


@pytest.mark.parametrize("value", VALUES)
def test_batch_norm_module_eval_mode(value):
    n, C = 1025, 64
    stats = (torch.linspace(-0.3, 0.6, C), torch.linspace(0.5, 2.0, C))
    _bn_experiments(_module_run(n, C, True, True, training=False), n, C, True, True, value, "bn module eval", BN_TOL, 61, eval_stats=stats)


def _small_run(n, C, nslab, relu, res):
    """mink_bn_small_fwd / _bwd; with slabs, the value (and the gradient) arrives as `nslab` slabs and the poison sits in the
    last one."""
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(7 * n + nslab)
    extra = torch.randn(max(nslab - 1, 0), n, C, generator=g) * 0.01  # (small: the sum stays the given value to fp32 rounding)

    def slabs_of(t):
        if nslab == 0:
            return t[None].clone()
        return torch.cat([extra, (t - extra.double().sum(0).float())[None]])

    def run(x, r, gy, gamma, beta):
        sl = slabs_of(x).to(dev)
        y = sl[0].clone() if nslab == 0 else torch.empty(n, C, device=dev)
        ga, be = gamma.to(dev), beta.to(dev)
        rd = r.to(dev) if r is not None else None
        rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
        out, mean, invstd = torch.empty(n, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
        check(L.mink_bn_small_fwd(sl.data_ptr() if nslab else None, nslab, n, C, y.data_ptr(), 1e-5, 0.1, ga.data_ptr(), be.data_ptr(),
                                  rd.data_ptr() if rd is not None else None, int(relu), out.data_ptr(), mean.data_ptr(), invstd.data_ptr(),
                                  rm.data_ptr(), rv.data_ptr(), _st()))
        gsl = slabs_of(gy).to(dev)
        g_sum = torch.empty(n, C, device=dev)
        dx, dres = torch.empty(n, C, device=dev), (torch.empty(n, C, device=dev) if rd is not None else None)
        dgamma, dbeta = torch.empty(C, device=dev), torch.empty(C, device=dev)
        check(L.mink_bn_small_bwd(gsl.data_ptr(), nslab, None, g_sum.data_ptr() if nslab else None, y.data_ptr(), out.data_ptr(), n, C,
                                  mean.data_ptr(), invstd.data_ptr(), ga.data_ptr(), int(relu), dx.data_ptr(),
                                  dres.data_ptr() if dres is not None else None, dgamma.data_ptr(), dbeta.data_ptr(), _st()))
        torch.cuda.synchronize()
        o = {"y": out.cpu(), "mean": mean.cpu(), "invstd": invstd.cpu(), "rm": rm.cpu(), "rv": rv.cpu(), "dx": dx.cpu(),
             "dgamma": dgamma.cpu(), "dbeta": dbeta.cpu()}
        if dres is not None:
            o["dres"] = dres.cpu()
        return o

    return run


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("n,C,nslab,relu,res", [(63, 64, 3, True, True), (1024, 128, 1, False, True), (300, 48, 0, True, False)])
def test_one_launch_batch_norm_entry_points(n, C, nslab, relu, res, value):
    """mink_bn_small_fwd / _bwd at both SmallCfg widths (C % 16 == 0: 16 channels per workgroup, else 8), with and without
    split-K slabs.  Rows beyond n are read from row 0 by the kernel (`live ? r : 0`): poisoned, they must not count."""
    _bn_experiments(_small_run(n, C, nslab, relu, res), n, C, relu, res, value, f"bn small n={n} C={C} slabs={nslab}", BN_SMALL_TOL, 70 + n)


def _partials_run(n, C, rows, fold, slabs_bwd=False):
    """mink_bn_apply_from_partials (statistics from `rows` column partials, finalize folded into the apply pass when `fold`) and
    mink_bn_bwd; with `slabs_bwd` the backward is mink_bn_bwd_slabs with the gradient in two slabs and an addend that carries
    the poison."""
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    dev = torch.device("cuda", 0)

    def run(x, r, gy, gamma, beta):
        old = L.mink_bn_set_fold(fold)
        try:
            xd = x.to(dev)
            part = torch.zeros(rows, 2, C, dtype=F64, device=dev)
            for q in range(rows):  # genuine partials of x over interleaved rows
                xs = xd[q::rows].double()
                part[q, 0], part[q, 1] = xs.sum(0), (xs * xs).sum(0)
            ga, be, rd = gamma.to(dev), beta.to(dev), r.to(dev)
            y, mean, invstd = torch.empty(n, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
            rm, rv = torch.zeros(C, device=dev), torch.ones(C, device=dev)
            check(L.mink_bn_apply_from_partials(xd.data_ptr(), n, C, part.data_ptr(), rows, 1e-5, 0.1, ga.data_ptr(), be.data_ptr(), rd.data_ptr(),
                                                1, y.data_ptr(), mean.data_ptr(), invstd.data_ptr(), rm.data_ptr(), rv.data_ptr(), _st()))
            dx, dres = torch.empty(n, C, device=dev), torch.empty(n, C, device=dev)
            dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
            ws = torch.empty(L.mink_bn_workspace_bytes(n, C), dtype=torch.uint8, device=dev)
            if slabs_bwd:
                base = torch.randn(n, C, generator=torch.Generator().manual_seed(3)).to(dev)
                sl = torch.stack([base, -base]).contiguous()  # two slabs that cancel; the gradient itself arrives as addend + ...
                g_sum = torch.empty(n, C, device=dev)
                gyd = gy.to(dev)
                check(L.mink_bn_bwd_slabs(sl.data_ptr(), 2, gyd.data_ptr(), g_sum.data_ptr(), xd.data_ptr(), y.data_ptr(), n, C, mean.data_ptr(),
                                          invstd.data_ptr(), ga.data_ptr(), 1, dx.data_ptr(), dres.data_ptr(), dg.data_ptr(), db.data_ptr(),
                                          ws.data_ptr(), ws.numel(), _st()))
            else:
                gyd = gy.to(dev)
                check(L.mink_bn_bwd(gyd.data_ptr(), xd.data_ptr(), y.data_ptr(), n, C, mean.data_ptr(), invstd.data_ptr(), ga.data_ptr(), 1,
                                    dx.data_ptr(), dres.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
            torch.cuda.synchronize()
            out = {"y": y, "mean": mean, "invstd": invstd, "rm": rm, "rv": rv, "dx": dx, "dgamma": dg, "dbeta": db, "dres": dres}
            if slabs_bwd:
                out["g_sum"] = g_sum
            return {k: t.cpu() for k, t in out.items()}
        finally:
            L.mink_bn_set_fold(old)

    return run


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("fold", [0, 1128])
def test_batch_norm_from_partials_folded_and_separate(fold, value):
    """n = 2128, C = 256, 67 partial rows (test_batch_norm_finalize_inside_the_apply_pass_is_bitwise): the finalize as a launch
    of its own and folded into the apply pass."""
    _bn_experiments(_partials_run(2128, 256, 67, fold), 2128, 256, True, True, value, f"bn from partials fold={fold}", BN_TOL, 81)


@pytest.mark.parametrize("value", VALUES)
def test_batch_norm_backward_from_slabs_with_an_addend(value):
    """mink_bn_bwd_slabs: g = slab 0 + slab 1 + addend; the poison arrives in the addend.  g_sum carries it at its elements."""
    n, C = 1500, 64
    run = _partials_run(n, C, 40, 0, slabs_bwd=True)
    _bn_experiments(run, n, C, True, True, value, "bn bwd slabs", BN_TOL, 82)
    v = FP.POISONS[value]
    g = torch.Generator().manual_seed(82)
    x = torch.randn(n, C, generator=g) * 1.5 + 0.3
    gy = FP.poison(torch.randn(n, C, generator=g), v, FP.poison_rows(n))
    r = torch.randn(n, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    got = run(x, r, gy, gamma, beta)
    FP.same_footprint(got["g_sum"], gy.double(), None, "bn bwd slabs g_sum")  # (base - base + gy is gy exactly)


# ------------------------------------------------------------------------------------------------ fused bn + relu + sum pool
@functools.lru_cache(None)
def _stem_tables():
    from test_gpu_stem16 import _stem_inputs

    _, _, nbr_pool, i2o = _stem_inputs([41, 42], 16)
    return nbr_pool, i2o


def _pool_children(z, i2o, n_pool):
    return torch.zeros(n_pool, z.shape[1], dtype=F64).index_add_(0, i2o, z)


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("storage", ["fp32", "bf16"])
def test_fused_bn_relu_pool(storage, value):
    """mink_bn_relu_pool_fwd / _bwd (fp32 and bf16 storage of the input) on the stride-2 pooling table of a two-scene grid-16
    batch: reference BatchNorm1d in float64 -> relu -> the sum over the children.  With batch statistics the poisoned column is
    non-finite in all of the output; with given (eval) statistics only the pooled rows that have a poisoned child are -- a
    missing child, which the K = 8 form loads from row 0 (poisoned), must not show."""
    from nerf_downstream_amd._lib import check, lib

    L = lib()
    v = FP.POISONS[value]
    nbr_pool, i2o = _stem_tables()
    n, n_pool, C = i2o.shape[0], nbr_pool.shape[0], 64
    assert int((nbr_pool < 0).sum()) > 0 and nbr_pool.shape[1] == 8  # there are missing children
    i2o_h = i2o.cpu().long()
    g = torch.Generator().manual_seed(90)
    x = torch.randn(n, C, generator=g) * 1.5 + 0.3
    if storage == "bf16":
        x = x.to(torch.bfloat16).float()
    gp = torch.randn(n_pool, C, generator=g)
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.rand(C, generator=g) - 0.5
    rows, pc = FP.poison_rows(n), FP.poison_channels(C)
    keep = _cols(C, pc)
    dev = torch.device("cuda", 0)

    def run(xin, gin, mean, invstd):
        xd = xin.to(dev).to(torch.bfloat16).contiguous() if storage == "bf16" else xin.to(dev)
        md, isd, ga, be, gd = mean.float().to(dev), invstd.float().to(dev), gamma.to(dev), beta.to(dev), gin.to(dev)
        out = torch.empty(n_pool, C, device=dev)
        dx, dg, db = torch.empty(n, C, device=dev), torch.empty(C, device=dev), torch.empty(C, device=dev)
        ws = torch.empty(L.mink_bn_workspace_bytes(n, C), dtype=torch.uint8, device=dev)
        if storage == "bf16":
            check(L.mink_bn_relu_pool_fwd_b16(xd.data_ptr(), C, md.data_ptr(), isd.data_ptr(), ga.data_ptr(), be.data_ptr(), nbr_pool.data_ptr(),
                                              n_pool, 8, out.data_ptr(), _st()))
            check(L.mink_bn_relu_pool_bwd_b16(gd.data_ptr(), xd.data_ptr(), n, C, md.data_ptr(), isd.data_ptr(), ga.data_ptr(), be.data_ptr(),
                                              i2o.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
            res = {"y": out, "dgamma": dg, "dbeta": db}
        else:
            check(L.mink_bn_relu_pool_fwd(xd.data_ptr(), C, md.data_ptr(), isd.data_ptr(), ga.data_ptr(), be.data_ptr(), nbr_pool.data_ptr(),
                                          n_pool, 8, out.data_ptr(), _st()))
            check(L.mink_bn_relu_pool_bwd(gd.data_ptr(), xd.data_ptr(), n, C, md.data_ptr(), isd.data_ptr(), ga.data_ptr(), be.data_ptr(),
                                          i2o.data_ptr(), dx.data_ptr(), dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
            res = {"y": out, "dx": dx, "dgamma": dg, "dbeta": db}
        torch.cuda.synchronize()
        return {k: t.cpu() for k, t in res.items()}

    def ref(xin, gin, stats):
        x64 = xin.double().requires_grad_(True)
        if stats is None:
            bn = torch.nn.BatchNorm1d(C).double()
            with torch.no_grad():
                bn.weight.copy_(gamma.double()), bn.bias.copy_(beta.double())
            z = bn(x64)
            ga, be = bn.weight, bn.bias
        else:
            ga, be = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
            z = (x64 - stats[0]) * stats[1] * ga + be
        out = _pool_children(torch.relu(z), i2o_h, n_pool)
        out.backward(gin.double())
        return {"y": out.detach(), "dx": x64.grad, "dgamma": ga.grad, "dbeta": be.grad}

    def stats_of(xin):
        xd = xin.double()
        m = xd.mean(0)
        return m, 1.0 / torch.sqrt(((xd - m) ** 2).mean(0) + 1e-5)

    tol = {"y": dict(atol=1e-5, rtol=1e-5), "dx": dict(atol=1e-5, rtol=1e-4), "dgamma": dict(atol=1e-3, rtol=1e-4),
           "dbeta": dict(atol=1e-3, rtol=1e-4)}  # tests/test_gpu_ops.py test_fused_bn_relu_sumpool
    xp, gpp = FP.poison(x, v, rows), FP.poison(gp, v, FP.poison_rows(n_pool))
    # batch statistics: (a) forward output, (b) gradients (the fused backward's dx is the training-mode one)
    st = (torch.linspace(-0.3, 0.6, C).double(), torch.linspace(0.7, 1.4, C).double())
    r, rb, rs = ref(xp, gp, None), ref(x, gpp, None), ref(xp, gp, st)
    FP.visible({"(a) y": r["y"], "(b) dgamma": rb["dgamma"], "(b) dbeta": rb["dbeta"], "(b) dx": rb["dx"], "given statistics y": rs["y"]},
               f"bn_relu_pool {storage}")
    clean = run(x, gp, *stats_of(x))
    got = run(xp, gp, *stats_of(xp))
    FP.same_footprint(got["y"], r["y"], tol["y"], f"bn_relu_pool {storage} (a) y", behind="batch norm")
    FP.untouched(got["y"], clean["y"], keep[None, :], f"bn_relu_pool {storage} (a) y")
    assert bool(FP.footprint(got["y"])[:, pc].all())
    r = rb
    names = [k for k in ("dx", "dgamma", "dbeta") if k in clean]
    got = run(x, gpp, *stats_of(x))
    assert torch.equal(got["y"], clean["y"])
    for k in names:
        FP.same_footprint(got[k], r[k], tol[k], f"bn_relu_pool {storage} (b) {k}", behind="batch norm")
        FP.untouched(got[k], clean[k], keep[None, :] if got[k].dim() == 2 else keep, f"bn_relu_pool {storage} (b) {k}")
    # given statistics: the forward's footprint is the pooled rows with a poisoned child, nothing else
    r = rs
    got = run(xp, gp, *st)
    FP.same_footprint(got["y"], r["y"], tol["y"], f"bn_relu_pool {storage} given statistics y")
    expect = torch.zeros(n_pool, C, dtype=torch.bool)
    for row in rows:
        expect[i2o_h[row], pc] = True
    assert not bool((FP.footprint(got["y"]) & ~expect).any())  # (nothing outside them, whatever the ReLU lets through)


# ================================================================================================ instance and layer norm
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("C", [3, 24, 70])
def test_instance_norm_poison_stays_in_its_sample(C, value):
    import test_gpu_norm as TN

    v = FP.POISONS[value]
    off, eps = TN._offsets(TN.SIZES), 1e-8
    n = off[-1]
    x, dy, res, gamma, beta = TN._inputs(n, C, 7)
    s, e = off[1], off[2]  # the 700-row sample
    rows = [s + r for r in FP.poison_rows(e - s)]
    pc = FP.poison_channels(C)
    other = torch.ones(n, C, dtype=torch.bool)
    other[s:e, pc] = False  # every other sample, every other column
    xp, dyp = FP.poison(x, v, rows), FP.poison(dy, v, rows)
    for relu, residual in TN.VARIANTS:
        what = f"IN C={C} relu={relu} res={residual}"
        r = res if residual else None
        clean = TN._run_in(x, dy, res, gamma, beta, off, eps, relu, residual)
        # (a)
        ref = NR.instance_norm_fwd(xp, off, gamma, beta, eps, r, relu)
        mask = (clean[0] > 0) if relu else None
        rdx, rdga, rdbe, rdres = NR.instance_norm_bwd(dyp, x, off, gamma, beta, eps, r, relu, mask)
        FP.visible({"(a) y": ref, "(b) dx": rdx}, what)
        got = TN._run_in(xp, dy, res, gamma, beta, off, eps, relu, residual)
        FP.same_footprint(got[0], ref, TN.FWD_TOL, what + " (a) y", behind="instance norm")
        FP.untouched(got[0], clean[0], other, what + " (a) y")
        assert bool(FP.footprint(got[0])[s:e, pc].all())
        # (b)
        got = TN._run_in(x, dyp, res, gamma, beta, off, eps, relu, residual)
        assert torch.equal(got[0], clean[0])
        FP.same_footprint(got[1], rdx, TN.GRAD_TOL, what + " (b) dx", behind="instance norm")
        FP.untouched(got[1], clean[1], other, what + " (b) dx")
        FP.same_footprint(got[2], rdga, TN.GRAD_TOL, what + " (b) dgamma", behind="instance norm")
        FP.same_footprint(got[3], rdbe, TN.GRAD_TOL, what + " (b) dbeta", behind="instance norm")
        FP.untouched(got[2], clean[2], _cols(C, pc), what + " (b) dgamma")
        FP.untouched(got[3], clean[3], _cols(C, pc), what + " (b) dbeta")
        if residual:
            FP.same_footprint(got[4], rdres, None, what + " (b) dresidual")


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("C", [3, 32, 70])
def test_layer_norm_poison_stays_in_its_row(C, value):
    import test_gpu_norm as TN

    v = FP.POISONS[value]
    eps = 1e-5
    for n in (65, 1000):
        x, dy, res, gamma, beta = TN._inputs(n, C, 10 + n)
        rows, pc = FP.poison_rows(n), FP.poison_channels(C)
        other = torch.ones(n, 1, dtype=torch.bool)
        other[rows] = False
        xp, dyp = FP.poison(x, v, rows), FP.poison(dy, v, rows)
        for relu, residual in TN.VARIANTS:
            what = f"LN n={n} C={C} relu={relu} res={residual}"
            r = res if residual else None
            clean = TN._run_ln(x, dy, res, gamma, beta, eps, relu, residual)
            ref = NR.layer_norm_fwd(xp, gamma, beta, eps, r, relu)
            mask = (clean[0] > 0) if relu else None
            rdx, rdga, rdbe, rdres = NR.layer_norm_bwd(dyp, x, gamma, beta, eps, r, relu, mask)
            FP.visible({"(a) y": ref, "(b) dx": rdx}, what)
            got = TN._run_ln(xp, dy, res, gamma, beta, eps, relu, residual)
            FP.same_footprint(got[0], ref, TN.FWD_TOL, what + " (a) y", behind="layer norm")
            FP.untouched(got[0], clean[0], other.expand(n, C), what + " (a) y")
            got = TN._run_ln(x, dyp, res, gamma, beta, eps, relu, residual)
            assert torch.equal(got[0], clean[0])
            FP.same_footprint(got[1], rdx, TN.GRAD_TOL, what + " (b) dx", behind="layer norm")
            FP.untouched(got[1], clean[1], other.expand(n, C), what + " (b) dx")
            FP.same_footprint(got[2], rdga, TN.GRAD_TOL, what + " (b) dgamma", behind="layer norm")
            FP.same_footprint(got[3], rdbe, TN.GRAD_TOL, what + " (b) dbeta", behind="layer norm")
            if residual:
                FP.same_footprint(got[4], rdres, None, what + " (b) dresidual")


# ================================================================================================ pooling
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("case", ["B4", "one4100"])
@pytest.mark.parametrize("C", [3, 32])
def test_local_pools(case, C, value):
    """Sum, average and max pooling of csrc/pool.hip on the two inputs of tests/test_gpu_pool.py (dword and 16-byte lanes)."""
    import test_gpu_pool as TP

    Fn = TP._fns()
    v = FP.POISONS[value]
    n = TP._coords(case).shape[0]
    x = TP._randn(n, C, 100 + C)
    xp = FP.poison(x, v, FP.poison_rows(n))
    K, EPS = TP.K, TP.EPS
    for k, s in TP.KS:
        _, _, nbr, nbr_t = TP._tables(case, k, s)
        _, table = TP._ref_maps(case, k, s)
        m = table.shape[0]
        dy = TP._randn(m, C, 200 + C)
        dyp = FP.poison(dy, v, FP.poison_rows(m))
        what = f"{case} C={C} k={k} s={s}"
        # max: (a) value bitwise and arg = the first NaN in offset order; (b) the gradient goes to the chosen row only
        ry, rarg = PR.max_fwd(xp, table)
        _, carg = PR.max_fwd(x, table)
        rdx = PR.max_bwd(dyp, carg, table, n)
        FP.visible({"(a) y": ry, "(b) dx": rdx}, "max " + what)  # (a maximum absorbs -inf: then the gradient is the visible output)
        y, arg, _ = TP._run(Fn.SparseMaxPoolFunction, xp, dy, nbr, nbr_t)
        FP.same_footprint(y, ry, None, "max " + what + " (a) y")
        assert torch.equal(arg.long(), rarg), "max " + what + " (a) arg"
        _, arg, dx = TP._run(Fn.SparseMaxPoolFunction, x, dyp, nbr, nbr_t)
        assert torch.equal(arg.long(), carg)
        FP.same_footprint(dx, rdx, K * EPS * PR.max_bwd_abs(dyp, carg, table, n), "max " + what + " (b) dx")
        for fn, avg, fwd, bwd in ((Fn.AvgPoolFunction, True, PR.avg_fwd, PR.avg_bwd), (Fn.OverlapSumPoolFunction, False, PR.sum_fwd, PR.sum_bwd)):
            name = ("avg " if avg else "sum ") + what
            ry, rdx = fwd(xp, table), bwd(dyp, table, n)
            FP.visible({"(a) y": ry, "(b) dx": rdx}, name)
            y, _, _ = TP._run(fn, xp, dy, nbr, nbr_t)
            FP.same_footprint(y, ry, (K + 1) * EPS * PR.sum_fwd_abs(xp, table, avg), name + " (a) y")
            _, _, dx = TP._run(fn, x, dyp, nbr, nbr_t)
            FP.same_footprint(dx, rdx, (K + 1) * EPS * PR.sum_bwd_abs(dyp, table, n, avg), name + " (b) dx")


def _synthetic_table(m, K, n_in, seed, unnamed):
    """table [<= m, K]: an input row at most once per offset, as a kernel map has it; ~45 % empty entries; no window without
    entries; `unnamed` named nowhere."""
    g = torch.Generator().manual_seed(seed)
    t = torch.stack([torch.randperm(n_in, generator=g)[:m] for _ in range(K)], 1)
    keep0 = t[:, 0].clone()
    t[torch.rand(m, K, generator=g) < 0.45] = -1
    t[:, 0] = torch.where((t >= 0).sum(1) == 0, keep0, t[:, 0])
    for o, k in (t == unnamed).nonzero().tolist():
        t[o, k] = -1
    return t[(t >= 0).sum(1) >= 1]  # (a window that lost its only entry to `unnamed` is dropped)


@pytest.mark.parametrize("value", VALUES)
def test_table_max_and_sum_of_the_stem_and_dense_path(value):
    """mink_pool_max_fwd / _bwd (the table max of pool.hip) and mink_pool_sum_fwd on a synthetic table with
    overlapping windows, empty entries and one input row that no entry names."""
    from nerf_downstream_amd.minkowski import functional as Fn

    v = FP.POISONS[value]
    n_in, m, K, C, unnamed = 300, 211, 9, 8, 150
    table = _synthetic_table(m, K, n_in, 5, unnamed)
    m = table.shape[0]
    tt = torch.full((n_in, K), -1, dtype=torch.long)  # the transposed table: tt[i][k] = o iff table[o][k] = i
    o, k = (table >= 0).nonzero(as_tuple=True)
    tt[table[o, k], k] = o
    assert not bool((table == unnamed).any()) and m > 200 and int((table < 0).sum()) > 0
    nbr, nbr_t = table.int().cuda(), tt.int().cuda()
    x, dy = _randn(n_in, C, 6), _randn(m, C, 7)
    xp = FP.poison(x, v, FP.poison_rows(n_in, extra=[unnamed]))
    dyp = FP.poison(dy, v, FP.poison_rows(m))
    ry, rarg = PR.max_fwd(xp, table)
    _, carg = PR.max_fwd(x, table)
    rdx = PR.max_bwd(dyp, carg, table, n_in)
    FP.visible({"(a) y": ry, "(b) dx": rdx}, "table max")
    xd = xp.cuda().requires_grad_(True)
    y = Fn.MaxPoolFunction.apply(xd, nbr, nbr_t)
    FP.same_footprint(y, ry, None, "table max (a) y")
    arg = y.grad_fn.saved_tensors[0] if hasattr(y.grad_fn, "saved_tensors") else None
    if arg is not None:
        assert torch.equal(arg.cpu().long(), rarg), "table max (a) arg"
    xd = x.cuda().requires_grad_(True)
    Fn.MaxPoolFunction.apply(xd, nbr, nbr_t).backward(dyp.cuda())
    FP.same_footprint(xd.grad, rdx, 27 * PR.EPS32 * PR.max_bwd_abs(dyp, carg, table, n_in), "table max (b) dx")
    # the non-overlapping sum pooling of the stem (one window per input row: the first offset of every row that has one)
    i2o = torch.full((n_in,), 0, dtype=torch.long)
    single = torch.full_like(table, -1)
    taken = torch.zeros(n_in, dtype=torch.bool)
    for o, k in (table >= 0).nonzero().tolist():
        i = int(table[o, k])
        if not taken[i]:
            taken[i], single[o, k], i2o[i] = True, i, o
    ry = PR.sum_fwd(xp, single)
    FP.visible({"y": ry}, "table sum")
    y = Fn.SumPoolFunction.apply(xp.cuda(), single.int().cuda(), i2o.int().cuda())
    FP.same_footprint(y, ry, 8 * PR.EPS32 * PR.sum_fwd_abs(xp, single) + 2.0 ** -149, "table sum (a) y")


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("case", ["B4", "one4100"])
@pytest.mark.parametrize("C", [3, 32, 70])
def test_global_pools(case, C, value):
    """Global max / sum / average over the batch offsets: the poison at rows 0, 63, 64 and the last of the tensor, then ONE
    poisoned element at the first, a middle and the last row of every sample (what a butterfly that is not symmetric under NaN
    gets wrong), then two in one column (the first is the arg)."""
    import test_gpu_pool as TP

    Fn = TP._fns()
    v = FP.POISONS[value]
    off, boff = TP._offsets(case), TP._boff(case)
    n, B = off[-1], len(off) - 1
    x, dy = TP._randn(n, C, 500 + C), TP._randn(B, C, 600 + C)
    pc = FP.poison_channels(C)
    inputs = {"pattern": FP.poison(x, v, FP.poison_rows(n))}
    for where in ("first", "middle", "last"):
        xp = x.clone()
        for b in range(B):
            if off[b + 1] > off[b]:
                row = {"first": off[b], "middle": (off[b] + off[b + 1]) // 2, "last": off[b + 1] - 1}[where]
                xp[row, pc[b % len(pc)]] = v
        inputs[where] = xp
    two = x.clone()
    two[[off[0] + 70, off[1] - 3], pc[0]] = v
    inputs["two in a column"] = two
    reached = FP.Reached(list(inputs))
    for name, xp in inputs.items():
        what = f"global {case} C={C} {name}"
        ry, rarg = PR.global_max_fwd(xp, off)
        FP.visible({"max y": ry, "sum y": PR.global_sum_fwd(xp, off)}, what)  # (a maximum absorbs -inf, a sum does not)
        y, arg, dx = TP._run(Fn.GlobalMaxPoolFunction, xp, dy, boff)
        FP.same_footprint(y, ry, None, what + " max y")
        assert torch.equal(arg.long(), rarg), what + " max arg: " + str((arg.long() != rarg).nonzero()[:4].tolist())
        assert torch.equal(dx.double(), PR.global_max_bwd(dy, rarg, n)), what + " max dx"
        ref = PR.global_sum_fwd(xp, off)
        y, _, _ = TP._run(Fn.GlobalSumPoolFunction, xp, dy, boff)
        FP.same_footprint(y, ref, TP.EPS * ref.abs() + TP.TINY, what + " sum y")
        if C % 4 == 0:  # (mink_global_avg_fwd takes 16-byte lanes only)
            ref = PR.global_avg_fwd(xp, off)
            y, _, _ = TP._run(Fn.GlobalAvgPoolFunction, xp, dy, boff)
            FP.same_footprint(y, ref, dict(atol=1e-5, rtol=0), what + " avg y")  # (tests/test_gpu_ops.py test_relu_add_pool_globalavg)
        reached.reach(name)
    # (b): a poisoned gradient row goes to the arg row (max) or to every row of its sample (sum, avg), nowhere else
    dyp = FP.poison(dy, v, FP.poison_rows(B))
    _, carg = PR.global_max_fwd(x, off)
    rdx = PR.global_max_bwd(dyp, carg, n)
    _, _, dx = TP._run(Fn.GlobalMaxPoolFunction, x, dyp, boff)
    FP.same_footprint(dx, rdx, None, f"global {case} C={C} max (b) dx")
    rdx = PR.global_sum_bwd(dyp, off)
    _, _, dx = TP._run(Fn.GlobalSumPoolFunction, x, dyp, boff)
    FP.same_footprint(dx, rdx, None, f"global {case} C={C} sum (b) dx")
    FP.visible({"dx": rdx}, f"global {case} (b)")
    if C % 4 == 0:
        cnt = torch.tensor([max(off[b + 1] - off[b], 1) for b in range(B)], dtype=F64)
        _, _, dx = TP._run(Fn.GlobalAvgPoolFunction, x, dyp, boff)
        FP.same_footprint(dx, PR.global_sum_bwd(dyp.double() / cnt[:, None], off), dict(atol=1e-6, rtol=0), f"global {case} C={C} avg (b) dx")
    reached.finish(f"global pools {case} C={C} {value}")


@pytest.mark.parametrize("value", VALUES)
def test_field_to_sparse_average(value, oracle_maps):
    """TensorField.sparse() (mink_segment_mean): a poisoned point reaches its own voxel's mean and no other."""
    from nerf_downstream_amd import minkowski as ME
    from oracle import me_cpu as OME

    v = FP.POISONS[value]
    rng = np.random.default_rng(0)
    coords, _ = batch_scenes([1, 2], grid=12, cin=6, negative=True)
    rep = torch.from_numpy(np.sort(rng.integers(0, len(coords), 3 * len(coords))))
    coords = coords[rep].clone()
    feats = torch.from_numpy(rng.standard_normal((len(rep), 6)).astype(np.float32))
    coords[:, 1:] += torch.from_numpy(rng.uniform(0, 0.99, (len(rep), 3)).astype(np.float32))
    fp = FP.poison(feats, v, FP.poison_rows(len(rep)))
    ox = OME.TensorField(coordinates=coords, features=fp.double()).sparse()
    FP.visible({"F": ox.F}, "field -> sparse")
    x = ME.TensorField(coordinates=coords.cuda(), features=fp.cuda()).sparse()
    assert np.array_equal(x.C.cpu().numpy(), ox.C.numpy())
    FP.same_footprint(x.F, ox.F, dict(atol=1e-6, rtol=0), "field -> sparse F")  # (tests/test_gpu_ops.py test_field_to_sparse_average)


# ================================================================================================ interpolation and splat
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("C", [3, 32])
def test_interpolation_and_splat(C, value):
    """features_at_coordinates on the B4 map of tests/test_gpu_interp.py at strides 1 and 2 and TensorField.splat(): poisoned
    features, clean query coordinates.  One poisoned row is named by no query: it must appear nowhere.  A present corner of
    weight 0 multiplies (0 x NaN = NaN) in the kernels and in the restatement alike."""
    import test_gpu_interp as TI
    from nerf_downstream_amd import minkowski as ME

    v = FP.POISONS[value]
    case = "B4"
    q = TI._queries(case)
    qd = q.cuda()
    dy = TI._randn(q.shape[0], C, 200 + C)
    dyp = FP.poison(dy, v, FP.poison_rows(q.shape[0]))
    for ts in (1, 2):
        n = TI._level_coords(case, ts).shape[0]
        x = TI._randn(n, C, 100 + C + ts)
        rimap, rw = TI._ref_map(case, ts)
        named = torch.zeros(n, dtype=torch.bool)
        named[rimap[rimap >= 0]] = True
        unnamed = [int(i) for i in (~named).nonzero().flatten() if int(i) not in (0, 63, 64, n - 1)][:1]
        assert unnamed, "every row of the map is named by a query"
        xp = FP.poison(x, v, FP.poison_rows(n, extra=unnamed))
        what = f"interp C={C} ts={ts}"
        ref = IR.interp_fwd(xp, rimap, rw)
        FP.visible({"y": ref}, what)
        y = TI._tensor(case, ts, xp.cuda()).features_at_coordinates(qd)
        FP.same_footprint(y, ref, TI._fwd_bound(xp, rimap), what + " (a) y")
        ref = IR.interp_bwd(dyp, rimap, rw, n)
        FP.visible({"dx": ref}, what)
        xd = x.clone().cuda().requires_grad_(True)
        TI._tensor(case, ts, xd).features_at_coordinates(qd).backward(dyp.cuda())
        FP.same_footprint(xd.grad, ref, TI._bwd_bound(dyp, rimap, n), what + " (b) dx")
    fc = TI._field()
    coords, rimap, rw = IR.splat_coords(fc)
    nv = coords.shape[0]
    Ff, g = TI._randn(257, C, 700 + C), TI._randn(nv, C, 800 + C)
    Fp, gp = FP.poison(Ff, v, FP.poison_rows(257)), FP.poison(g, v, FP.poison_rows(nv))
    ref = IR.splat_fwd(Fp, rimap, rw, nv)
    FP.visible({"F_s": ref}, f"splat C={C}")
    st = ME.TensorField(features=Fp.cuda(), coordinates=fc.cuda()).splat()
    FP.same_footprint(st.F, ref, TI._bwd_bound(Fp, rimap, nv), f"splat C={C} (a) F_s")
    ref = IR.interp_fwd(gp, rimap, rw)
    FP.visible({"dF": ref}, f"splat C={C}")
    Fd = Ff.clone().cuda().requires_grad_(True)
    ME.TensorField(features=Fd, coordinates=fc.cuda()).splat().F.backward(gp.cuda())
    FP.same_footprint(Fd.grad, ref, TI._fwd_bound(gp, rimap), f"splat C={C} (b) dF")


# ================================================================================================ edge-convolution maximum
def _edge_ref(P, Q, idx, mean, invstd, gamma, beta):
    """z[i][j] = gamma ((P[idx[i][j]] + Q[i]) - mean) invstd + beta; y = lrelu(max_j z), arg = the first NaN or the first maximum."""
    e = P.double()[idx] + Q.double()[:, None, :]
    z = (e - mean) * invstd * gamma + beta
    arg = DR.first_argmax(z)
    zs = z.gather(1, arg[:, None, :])[:, 0, :]
    return DR.lrelu(zs), arg, zs


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("C,k", [(12, 5), (64, 20)])
def test_edge_maximum(C, k, value):
    """mink_edge_fwd / mink_edge_bwd on the samples of tests/test_gpu_dgcnn.py with a fixed, valid neighbour table built on the
    host from the clean features: P and Q poisoned, indices not.  The slot `at` starts at 0 and is only replaced by j < k."""
    import test_gpu_dgcnn as TD
    from nerf_downstream_amd._lib import check, lib
    from nerf_downstream_amd.minkowski import functional as Fn

    L = lib()
    v = FP.POISONS[value]
    n = TD.OFF[-1]
    feats = _randn(n, 8, 300 + C)
    idx = DR.knn(feats, TD.OFF, k)
    assert int(idx.min()) >= 0 and int(idx.max()) < n
    g = torch.Generator().manual_seed(310 + C)
    P, Q, dy = torch.randn(n, C, generator=g), torch.randn(n, C, generator=g), torch.randn(n, C, generator=g)
    mean, invstd = torch.randn(C, generator=g) * 0.2, torch.rand(C, generator=g) + 0.5
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.3
    idxd = idx.int().cuda().contiguous()
    members, seg = Fn.lazy_index_csr(idxd, n)()
    md, isd, ga, be = mean.cuda(), invstd.cuda(), gamma.cuda(), beta.cuda()
    m64, is64, g64, b64 = mean.double(), invstd.double(), gamma.double(), beta.double()

    def fwd(Pin, Qin):
        Pd, Qd = Pin.cuda(), Qin.cuda()
        y, arg = torch.empty(n, C, device="cuda"), torch.empty(n, C, dtype=torch.uint8, device="cuda")
        check(L.mink_edge_fwd(Pd.data_ptr(), Qd.data_ptr(), idxd.data_ptr(), n, k, C, md.data_ptr(), isd.data_ptr(), ga.data_ptr(), be.data_ptr(),
                              y.data_ptr(), arg.data_ptr(), _st()))
        return y, arg

    def bwd(dyin, arg, training):
        Pd, Qd, dyd = P.cuda(), Q.cuda(), dyin.cuda()
        dP, dQ = torch.empty(n, C, device="cuda"), torch.empty(n, C, device="cuda")
        dg, db = torch.empty(C, device="cuda"), torch.empty(C, device="cuda")
        ws = torch.empty(max(L.mink_edge_bwd_workspace_bytes(n, C), 8), dtype=torch.uint8, device="cuda")
        check(L.mink_edge_bwd(dyd.data_ptr(), Pd.data_ptr(), Qd.data_ptr(), idxd.data_ptr(), arg.data_ptr(), n, k, C, md.data_ptr(), isd.data_ptr(),
                              ga.data_ptr(), be.data_ptr(), int(training), members.data_ptr(), seg.data_ptr(), dP.data_ptr(), dQ.data_ptr(),
                              dg.data_ptr(), db.data_ptr(), ws.data_ptr(), ws.numel(), _st()))
        torch.cuda.synchronize()
        return dP.cpu(), dQ.cpu(), dg.cpu(), db.cpu()

    tol = dict(atol=1e-5, rtol=1e-5)  # (tests/test_gpu_dgcnn.py holds y to first-order bounds of a few ulps; the network test to 1e-5)
    # (a) P poisoned, then Q
    rows = FP.poison_rows(n)
    cases = [("P", FP.poison(P, v, rows), Q), ("Q", P, FP.poison(Q, v, rows))]
    FP.visible({name: _edge_ref(Pin, Qin, idx, m64, is64, g64, b64)[0] for name, Pin, Qin in cases}, "edge forward")  # (-inf in P: absorbed)
    for name, Pin, Qin in cases:
        ry, rarg, _ = _edge_ref(Pin, Qin, idx, m64, is64, g64, b64)
        y, arg = fwd(Pin, Qin)
        assert int(arg.max()) < k
        FP.same_footprint(y, ry, tol, f"edge forward, {name} poisoned: y")
        assert torch.equal(arg.cpu().long(), rarg), f"edge forward, {name} poisoned: arg"
    # (b) clean forward; eval-mode gradients against their formula, training-mode gradients column by column
    y, arg = fwd(P, Q)
    ry, rarg, zs = _edge_ref(P, Q, idx, m64, is64, g64, b64)
    assert torch.equal(arg.cpu().long(), rarg)
    dyp = FP.poison(dy, v, rows)
    gg = dyp.double() * torch.where(zs > 0, torch.ones_like(zs), 0.2 * torch.ones_like(zs))
    scale = g64 * is64
    rdQ = scale * gg
    onehot = torch.zeros(n, k, C, dtype=torch.bool).scatter_(1, rarg[:, None, :], True)
    terms = torch.where(onehot, gg[:, None, :].expand(-1, k, -1), torch.zeros((), dtype=F64))
    rdP = scale * torch.zeros(n, C, dtype=F64).index_add_(0, idx.reshape(-1), terms.reshape(-1, C))
    FP.visible({"dP": rdP, "dQ": rdQ}, "edge backward")
    dP, dQ, _, _ = bwd(dyp, arg, False)
    FP.same_footprint(dQ, rdQ, tol, "edge backward (eval) dQ")
    FP.same_footprint(dP, rdP, tol, "edge backward (eval) dP")
    pc = FP.poison_channels(C)
    clean = bwd(dy, arg, True)
    got = bwd(dyp, arg, True)
    for name, a, b in zip(("dP", "dQ", "dgamma", "dbeta"), got, clean):
        assert bool(FP.footprint(a)[..., pc].all()), f"edge backward (training) {name}: a poisoned column is not non-finite throughout"
        FP.untouched(a, b, _cols(C, pc)[None, :] if a.dim() == 2 else _cols(C, pc), f"edge backward (training) {name}")


# ================================================================================================ heads
@pytest.mark.parametrize("value", VALUES)
def test_classifier_head_and_cross_entropy(value):
    """mink_head_forward / _backward (global average + linear, with an EMPTY sample) and mink_softmax_ce_forward."""
    from nerf_downstream_amd.minkowski import functional as Fn

    v = FP.POISONS[value]
    B, C, ncls = 5, 64, 7
    counts = torch.tensor([70, 0, 1, 130, 33])
    boff = torch.cat([torch.zeros(1, dtype=torch.long), counts.cumsum(0)]).to(torch.int32)
    n = int(boff[-1])
    g = torch.Generator().manual_seed(400)
    x = torch.randn(n, C, generator=g)
    w, bias = torch.randn(C, ncls, generator=g) * 0.05, torch.randn(1, ncls, generator=g) * 0.1
    gl = torch.randn(B, ncls, generator=g)

    def pooled64(xx):
        return torch.stack([xx[boff[b]:boff[b + 1]].mean(0) if counts[b] > 0 else torch.zeros(C, dtype=F64) for b in range(B)])

    def ref(xin, gin):
        x64, w64, b64 = xin.double().requires_grad_(True), w.double().requires_grad_(True), bias.double().requires_grad_(True)
        logits = pooled64(x64) @ w64 + b64
        logits.backward(gin.double())
        return logits.detach(), x64.grad, w64.grad, b64.grad

    def run(xin, gin):
        xd, wd, bd = (t.cuda().requires_grad_() for t in (xin, w, bias))
        logits = Fn.global_avg_linear(xd, boff.cuda(), wd, bd)
        logits.backward(gin.cuda())
        return logits.detach().cpu(), xd.grad.cpu(), wd.grad.cpu(), bd.grad.cpu()

    tol = dict(atol=1e-5, rtol=0)  # tests/test_gpu_ops.py test_classifier_head_matches_torch
    xp = x.clone()
    xp[[0, 63, int(boff[3]) + 64], :] = FP.poison(x[[0, 63, int(boff[3]) + 64]], v, [0, 1, 2])  # samples 0 and 3
    rl, _, _, _ = ref(xp, gl)
    FP.visible({"logits": rl}, "head")
    got = run(xp, gl)
    FP.same_footprint(got[0], rl, tol, "head (a) logits")
    assert bool(torch.isfinite(got[0][[1, 2, 4]]).all()) and torch.equal(got[0][1], bias[0])  # the empty sample: logits = bias
    glp = FP.poison(gl, v, [1, 2, 4], channels=[0, ncls - 1])  # the empty sample, the one-row sample and a 33-row one
    _, rdx, rdw, rdb = ref(x, glp)
    FP.visible({"dx": rdx}, "head")
    got = run(x, glp)
    FP.same_footprint(got[1], rdx, (1e-5, float("inf")), "head (b) dx")  # (relative L2 error, as that test states it)
    FP.visible_reduction({"dw": rdw, "db": rdb}, "head")
    FP.no_swallow(got[2], rdw, "head (b) dw")
    FP.no_swallow(got[3], rdb, "head (b) db")
    # cross entropy: a poisoned logit (at the label's column, so that every poison value counts) makes the loss non-finite
    logits = torch.randn(B, ncls, generator=g)
    labels = torch.tensor([1, 2, 3, 4, 5])
    for b in (0, 2, 4):
        lp = logits.clone()
        lp[b, labels[b]] = v
        want = F.cross_entropy(lp.double(), labels)
        assert not bool(torch.isfinite(want))
        loss = Fn.cross_entropy(lp.cuda(), labels.cuda())
        assert not bool(torch.isfinite(loss)), f"cross entropy: row {b} poisoned, loss {float(loss)}"
        if FP.is_nan(v):
            assert bool(torch.isnan(loss))
    lp = logits.clone()
    lp[3, 0] = v  # ... and at another column, whatever torch's own loss is
    assert bool(torch.isfinite(Fn.cross_entropy(lp.cuda(), labels.cuda()))) == bool(torch.isfinite(F.cross_entropy(lp.double(), labels)))


@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("n,C", [(63, 8), (4097, 13)])
def test_segmentation_cross_entropy(n, C, value):
    """A poisoned logit in a counted row makes the loss non-finite, one in an ignored row leaves it finite (and equal to the
    clean loss), as in seghead_restate; pred stays in [0, C)."""
    import test_gpu_seghead as TS

    v = FP.POISONS[value]
    z, labels, w = SH.make_case(n, C, seed=100 + n % 97 + C, weighted=True)
    rows = FP.poison_rows(n)
    ign, cnt = rows[:2], rows[2:] or rows[:1]
    yt = None
    for name, poisoned, lab in (("ignored", ign, TS.IGNORE), ("counted", cnt, None)):
        lb = labels.copy()
        zp = z.copy()
        for r in poisoned:
            if lab is not None:
                lb[r] = lab
            else:
                lb[r] = r % C
            zp[r, lb[r] % C] = v  # (at the label's column for a counted row: every poison value then reaches the loss)
        ref = SH.ce(zp, lb, w, TS.IGNORE)
        clean = SH.ce(z, lb, w, TS.IGNORE)
        yt = torch.from_numpy(lb).cuda()
        got = TS._native(torch.from_numpy(zp).cuda(), yt, torch.from_numpy(w).cuda(), g=0.75)
        pred = got["pred"].cpu()
        assert int(pred.min()) >= 0 and int(pred.max()) < C, "pred left [0, C)"
        assert int(got["hist"].sum()) == got["st"]["n_valid"]
        if name == "ignored":
            assert np.isfinite(ref["loss"]) and ref["loss"] == clean["loss"]
            bound = (C + 8) * 2.0 ** -24 * max(1.0, float(np.abs(z).max()))  # (test_gpu_seghead._check_against_restatement)
            assert abs(got["loss"].item() - ref["loss"]) <= bound, (got["loss"].item(), ref["loss"])
            dz = got["dz"].cpu()
            assert bool(torch.isfinite(dz).all()) and bool((dz[poisoned] == 0).all())
        else:
            assert not np.isfinite(ref["loss"])
            assert not np.isfinite(got["loss"].item()), f"seg CE: counted rows {poisoned} poisoned, loss {got['loss'].item()}"
            if FP.is_nan(v):
                assert np.isnan(got["loss"].item())


# ================================================================================================ convolution
_CONV_TOL = {}


def _conv_tol(key, ref_fn, seq_fn, kind):
    """The bound of test_gpu_reduced_math.Judge.judge, computed once per (case, math) on the clean operands."""
    import test_gpu_reduced_math as RM

    if key not in _CONV_TOL:
        rel_s, max_s = RM._errs(seq_fn(kind), ref_fn(kind))
        _CONV_TOL[key] = (max(RM.REL_FLOOR, 2.0 * rel_s), max(RM.MAX_FLOOR, 2.0 * max_s))
    return _CONV_TOL[key]


def _widen(t, ld, fill):
    """[n, c] at row stride ld on the device, the pad columns holding `fill`."""
    n, c = t.shape
    wide = torch.full((n, ld), fill, dtype=torch.float32)
    wide[:, :c] = t
    return wide.cuda()[:, :c]


@pytest.mark.timeout(300)
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("math", ["fp32", "bf16", "bf16x3"])
def test_gather_gemm_forms(math, value):
    """Every case of test_gpu_reduced_math.GATHER_CASES: x (forward) or gy (data gradient) poisoned at rows 0, 63, 64, the last
    and one row that no table entry names, the pad columns of ldx > C poisoned throughout; reference _gather64 over the
    operands the launch form declares.  The statistics epilogue's column partials: no_swallow."""
    import test_gpu_reduced_math as RM
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd._lib import lib
    from nerf_downstream_amd.minkowski import functional as Fn

    v = FP.POISONS[value]
    L = lib()
    reached = FP.Reached(RM.GATHER_FORMS.get(math, []))
    ran = 0
    old = ME.set_conv_math(math)
    try:
        for ci, (name, op, n_out, K, cin, cout, o) in enumerate(RM.GATHER_CASES):
            assert n_out <= 6000
            perm16 = o.get("perm16", True)
            if not perm16 and math != "bf16":
                continue  # (the class-permuted compact form exists under bf16 math only)
            g = torch.Generator().manual_seed(1000 * ci + n_out + K)
            perm = RM._class_perm(n_out, g) if o.get("perm") else None
            n_in = max(4, n_out // 3 + 5) if perm is not None else max(4, n_out + 17)
            nbr = RM._table(n_out, K, n_in, g)
            unnamed = n_in // 2 + 1
            nbr[nbr == unnamed] = -1
            gin, gout = (cout, cin) if op == "dgrad" else (cin, cout)
            ldx = o.get("ldx", gin)
            src = torch.randn(n_in, ldx, generator=g)[:, :gin]
            w = torch.randn(K, cin, cout, generator=g) * 0.1
            if op == "dgrad":
                wr = w.transpose(1, 2)
                b = wr.flip(0) if perm is None else wr
            else:
                b = w
            wd, nd, bd = w.cuda(), nbr.cuda(), b.cuda()
            pd = perm.cuda() if perm is not None else None
            ks = o.get("ksplit", 1 if gin == 28 else 0)
            Fn._FORCE_KSPLIT = ks
            Fn._PLAN_CACHE.clear()
            L.mink_conv_set_stagger(0 if perm16 else 1 << 27)
            ks_eff = ks or Fn._plan_ksplit(L, n_out if perm is None else perm.numel(), K, gin, gout, int(perm is not None))
            cf = LW.conv_form(op, K, cin, cout, math, n_out=n_out, ldx=ldx, row_perm=perm is not None, ksplit=ks_eff, perm16=perm16,
                              shortcut_dense=False)
            kind = RM._declared_kind(cf, math)

            def launch(srcd):
                if op == "dgrad":
                    return Fn.gather_gemm(srcd, wd, nd, gout, w_transposed=True, flip_k=perm is None, row_perm=pd), None
                if o.get("stats"):
                    return Fn.gather_gemm(srcd, wd, nd, gout, stats=True)
                return Fn.gather_gemm(srcd, wd, nd, gout, row_perm=pd), None

            clean = _widen(src, ldx, 0.0)
            tol = _conv_tol((math, ci), lambda kd: sum(RM._gather64(p.double(), q.double(), nd) for p, q in RM._pairs(clean, bd, kd)),
                            lambda kd: RM._gather_seq32(RM._pairs(clean, bd, kd), nd), kind)
            rows = FP.poison_rows(n_in, extra=[unnamed])
            srcp = _widen(FP.poison(src, v, rows), ldx, v)
            ref = sum(RM._gather64(p.double(), q.double(), nd) for p, q in RM._pairs(srcp, bd, kind))
            FP.visible({"y": ref.cpu()}, f"{name} ({math})")
            y, part = launch(srcp)
            L.mink_conv_set_stagger(0)
            FP.same_footprint(y, ref, tol, f"{name} ({op}, {cf.form}, {math})", behind="bf16x3" if kind == "bf16x3" else None)
            reached.reach(cf.form)
            zs = -(-K // -(-K // ks_eff)) if cf.form != "class-permuted compact bf16" else 1
            if zs > 1:
                reached.reach("split-K")
            if o.get("stats"):
                assert part is not None, f"{name}: no statistics partials"
                reached.reach("stats split" if zs > 1 else "stats direct")
                r64 = ref.cpu()
                sums = torch.stack([r64.sum(0), (r64 * r64).sum(0)])
                FP.visible_reduction({"column sums": sums}, name)
                FP.no_swallow(part.sum(0), sums, f"{name}: statistics partials")
            ran += 1
    finally:
        Fn._FORCE_KSPLIT = 0
        L.mink_conv_set_stagger(0)
        Fn._PLAN_CACHE.clear()
        ME.set_conv_math(old)
    assert ran == len(RM.GATHER_CASES) - (0 if math == "bf16" else 1)
    reached.finish(f"gather-GEMM forms under {math}, {value}")


@pytest.mark.timeout(300)
@pytest.mark.parametrize("value", VALUES)
@pytest.mark.parametrize("math", ["fp32", "bf16", "bf16x3"])
def test_weight_gradient_forms(math, value):
    """Every case of test_gpu_reduced_math.WGRAD_CASES, x then gy poisoned: no_swallow against _wgrad64 (a zero-filled absent
    neighbour times a NaN gradient legitimately differs from a reference that skips the pair); with only x poisoned dW[k] of the
    offset no row has is exactly 0; and where the operator must not read at all -- a row no entry names, the pad columns of
    ldx > C -- the poison leaves dW bit for bit the clean run's."""
    import test_gpu_reduced_math as RM
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd._lib import lib
    from nerf_downstream_amd.minkowski import functional as Fn

    v = FP.POISONS[value]
    L = lib()
    reached = FP.Reached(RM.WGRAD_FORMS.get(math, []))
    old = ME.set_conv_math(math)
    try:
        for ci, (name, n_out, K, cin, cout, force, ldx) in enumerate(RM.WGRAD_CASES):
            assert n_out <= 6000
            n_in = max(4, n_out + 17)
            unnamed = n_in // 2 + 1
            for attempt in range(16):  # the first seeded table that names a poisoned x row and has an entry in a poisoned gy row
                g = torch.Generator().manual_seed(7000 + 31 * ci + n_out + 100000 * attempt)
                nbr = RM._table(n_out, K, n_in, g)
                nbr[nbr == unnamed] = -1
                if bool(torch.isin(nbr, torch.tensor(FP.poison_rows(n_in))).any()) and bool((nbr[FP.poison_rows(n_out)] >= 0).any()):
                    break
            ld = ldx or cin
            x = torch.randn(n_in, ld, generator=g)[:, :cin]
            dy = torch.randn(n_out, cout, generator=g)
            nd = nbr.cuda()
            cf = LW.conv_form("wgrad", K, cin, cout, math, n_out=n_out, ldx=ld, force_g=force)
            kind = "bf16" if cf.rounded else "fp32"

            def launch(xd, dyd):
                L.mink_conv_set_stagger(force << 12)
                Fn._PLAN_CACHE.clear()
                try:
                    return Fn.conv_wgrad(xd, dyd, nd, (K, cin, cout))
                finally:
                    L.mink_conv_set_stagger(0)

            def ref(xd, dyd):
                return sum(RM._wgrad64(p.double(), q.double(), nd) for p, q in RM._pairs(xd, dyd, kind))

            xc, dyc = _widen(x, ld, 0.0), dy.cuda()
            clean = launch(xc, dyc)
            # where the operator must not read: the unnamed row and the pad columns
            leak = _widen(FP.poison(x, v, [unnamed]), ld, v)
            assert torch.equal(launch(leak, dyc), clean), f"{name} ({cf.form}): a row no entry names, or a pad column, reached dW"
            xp = _widen(FP.poison(x, v, FP.poison_rows(n_in)), ld, 0.0)
            r = ref(xp, dyc)
            FP.visible_reduction({"dW": r.cpu()}, name)
            dw = launch(xp, dyc)
            FP.no_swallow(dw, r, f"{name} ({cf.form}, {math}) x poisoned")
            if K > 1:
                assert bool((dw[K // 2 - 1] == 0).all()), f"{name} ({cf.form}): dW of the offset no row has is not exactly 0"
            dyp = FP.poison(dy, v, FP.poison_rows(n_out)).cuda()
            r = ref(xc, dyp)
            FP.visible_reduction({"dW": r.cpu()}, name)
            FP.no_swallow(launch(xc, dyp), r, f"{name} ({cf.form}, {math}) gy poisoned")
            reached.reach(cf.form)
    finally:
        L.mink_conv_set_stagger(0)
        Fn._PLAN_CACHE.clear()
        ME.set_conv_math(old)
    reached.finish(f"weight-gradient forms under {math}, {value}")


@pytest.mark.parametrize("value", VALUES)
def test_stem_convolution_with_bf16_storage(value):
    """mink_rows_to_bf16 then mink_stem_conv_bf16s on the two-scene grid-24 input of tests/test_gpu_stem16.py."""
    import test_gpu_stem16 as T16
    from nerf_downstream_amd import minkowski as ME

    v = FP.POISONS[value]
    cin = 28
    coords, feats = batch_scenes([2, 3], grid=24, cin=cin)
    fp = FP.poison(feats, v, FP.poison_rows(feats.shape[0]))
    x = ME.TensorField(coordinates=coords.cuda(), features=fp.cuda()).sparse()
    k1 = ME.CoordinateMapKey(1)
    nbr, _ = x.coordinate_manager.kernel_table(k1, k1, 3, 1)
    xin = x.F.contiguous()
    torch.manual_seed(24)
    w = torch.randn(27, cin, 64, device="cuda") * 0.1
    xb, yb, part = T16._conv_b16(xin, w, nbr)
    assert torch.equal(FP.footprint(xb[:, :cin].float()), FP.footprint(xin)) and bool(torch.isfinite(xb[:, cin:].float()).all())
    xr, wr, tab = xb[:, :cin].double().cpu(), w.to(torch.bfloat16).double().cpu(), nbr.cpu().long()
    ref, mag = torch.zeros(tab.shape[0], 64, dtype=F64), torch.zeros(tab.shape[0], 64, dtype=F64)
    for k in range(27):
        has = tab[:, k] >= 0
        ref[has] += xr[tab[has, k]] @ wr[k]
        mag[has] += xr[tab[has, k]].abs() @ wr[k].abs()
    FP.visible({"y": ref}, "stem conv bf16 storage")
    FP.same_footprint(yb.float(), ref, ref.abs() * 2.0 ** -8 + mag * 1e-6 + 1e-30, "stem conv bf16 storage y")
    sums = torch.stack([ref.sum(0), (ref * ref).sum(0)])
    FP.visible_reduction({"column sums": sums}, "stem conv bf16 storage")
    FP.no_swallow(part.sum(0), sums, "stem conv bf16 storage: statistics partials")


# ================================================================================================ end to end
def _one_poisoned_feature(feats, v):
    fp = feats.clone()
    fp[feats.shape[0] // 3, 5] = v
    return fp


@pytest.mark.parametrize("value", ["nan", "+inf"])
@pytest.mark.parametrize("math", ["fp32", "bf16"])
@pytest.mark.parametrize("path", ["modules", "native trunk"])
def test_resnet14_reports_a_poisoned_input(path, math, value):
    """One non-finite input feature: the logits are non-finite, training_step returns a non-finite loss and check_finite raises.
    Through the Python modules on a two-scene grid-16 batch, and through the native trunk (minkowski/trunk.py, the path
    bench.py times) on the smallest batch that takes it (six 64^3 scenes, ~63 k voxels: below ~44 k the stem takes the module
    path) -- asserted."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.src.modules.classification_training import ClassificationTraining

    v = FP.POISONS[value]
    seeds, grid = (([31, 32], 16) if path == "modules" else ([31, 32, 33, 34, 35, 36], 64))
    coords, feats = batch_scenes(seeds, grid=grid, cin=28)
    labels = torch.arange(len(seeds), device="cuda")
    old_m, old_s = ME.set_conv_math(math), ME.set_conv_storage("fp32")
    try:
        torch.manual_seed(5)
        net = get_model("ResNet14", 28, 51).cuda()
        module = ClassificationTraining(net)
        for f, poisoned in ((feats, False), (_one_poisoned_feature(feats, v), True)):
            batch = {"coordinates": coords.cuda(), "features": f.cuda(), "labels": labels}
            loss, out = module.training_step(batch)
            assert (trunk_node(out) is not None) == (path == "native trunk"), "the path this case names was not taken"
            if not poisoned:
                assert bool(torch.isfinite(out).all()) and np.isfinite(float(loss))
                module.check_finite(float(loss))
                # one poisoned gradient element reaches the parameter gradients
                gl = torch.zeros_like(out)
                gl[0, 0] = v
                net.zero_grad(set_to_none=True)
                out.backward(gl)
                assert not bool(torch.isfinite(net.conv1.kernel.grad).all()), "a poisoned gradient did not reach the stem kernel"
                net.zero_grad(set_to_none=True)
                continue
            assert not bool(torch.isfinite(out).all()), "one poisoned input feature and finite logits: the network swallowed it"
            assert not np.isfinite(float(loss)), f"one poisoned input feature and a finite loss ({float(loss)})"
            with pytest.raises(ValueError):
                module.check_finite(float(loss))
    finally:
        ME.set_conv_math(old_m), ME.set_conv_storage(old_s)


@pytest.mark.parametrize("value", ["nan", "+inf"])
def test_res16unet_reports_a_poisoned_input(value):
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import SegmentationTraining

    v = FP.POISONS[value]
    coords, feats = batch_scenes([31, 32], grid=16, cin=28)
    C = 8
    labels = torch.randint(0, C, (feats.shape[0],), generator=torch.Generator().manual_seed(1))
    labels[::17] = 255
    torch.manual_seed(5)
    net = get_model("Res16UNet14A", 28, C).cuda()
    module = SegmentationTraining(net)
    for f, poisoned in ((feats, False), (_one_poisoned_feature(feats, v), True)):
        batch = {"coordinates": coords.cuda(), "features": f.cuda(), "labels": labels.cuda()}
        loss, out = module.training_step(batch)
        if not poisoned:
            assert bool(torch.isfinite(out).all()) and np.isfinite(float(loss))
            module.check_finite(float(loss))
            continue
        assert not bool(torch.isfinite(out).all()), "one poisoned input feature and finite logits: the network swallowed it"
        assert not np.isfinite(float(loss)), f"one poisoned input feature and a finite loss ({float(loss)})"
        with pytest.raises(ValueError):
            module.check_finite(float(loss))
