"""-m gpu: teacher-forced per-operator parity of the native trunk at the bench's launch shapes.

The whole-network tests (test_gpu_parity_full.py) see every launch the bench makes, but in bf16 they can only hold a tensor to
3 x 2^-8 (two bf16 networks drift apart through rounding ties), and when they fail they cannot say where.  Here every operator
of the stem and of every residual block is recomputed in float64 from the HIP run's OWN stored inputs -- activations,
statistics, incoming gradients, ReLU decisions (tests/layerwise.py) -- so no error carries over from the layers before, and each
one is held to its kernel test's bounds at the row counts that make the planners pick split-K, few-row, compacted and
class-permuted launches.  A failure names the operator.

Composites, where the trunk keeps no intermediate (minkowski/trunk.py _Saved.grad_stage):
  * the input gradient of an identity block is checked as conv1's data gradient + the residual gradient (g_x = g_xa + g_res):
    a block that leaves it pending (its conv1 data gradient still in split-K slabs) has it summed by the block before, inside
    that block's batch-norm backward (mink_bn_bwd_slabs / mink_bn_small_bwd store the sum), and g_xa is never written;
  * the input gradient of a strided block is conv1's class-permuted data gradient + the shortcut's (g_sc, checked on its own)
    scattered onto the rows it reaches (mink_rows_scatter_add);
  * conv2's data gradient g_h1 is stored by norm1's backward when it sums the slabs: checked as stored;
  * the stem's weight gradient recomputes its dY from (y, statistics, dgamma, dbeta, pooled gradient) inside the kernel: the
    reference recomputes it from the same stored values (layerwise.stem_wgrad_operand)."""
import pytest
import torch

import layerwise as LW
from helpers import _baseline_batch, _bench_like_step, _stem_masks_of_hip_run, trunk_node

pytestmark = [pytest.mark.gpu, pytest.mark.long]


def _pair(name, seed=777):
    from nerf_downstream_amd.co3d_3d.src.models import get_model

    torch.manual_seed(seed)
    return get_model(name, 28, 51).cuda()


def _conv_recs(layer, op, got, fn, ops, cf, reach=None):
    """check_conv of `got` against fn(**operands) as the launch form `cf` (layerwise.conv_form) multiplies them, with the other
    rounding as the discriminator; the form joins `reach`."""
    if reach is not None:
        reach.add("form: " + cf.form.split(" G")[0])
    return LW.check_conv(layer, op, got, LW.form_reference(fn, ops, cf), cf.rounded, LW.other_reference(fn, ops, cf))


def _stem_records(saved, model, out, math, before):
    """Stem: conv -> y (bf16-stored under bf16s), norm statistics, relu + pool -> out; backward: bn1.* and conv1.kernel."""
    recs = []
    x, w0, arena0, nbr0, nbr_pool, i2o, pad, b16, _ = saved.stem
    assert pad == 0
    n0, n1, C0 = x.shape[0], nbr_pool.shape[0], w0.shape[-1]
    ny = arena0.numel() - n1 * C0 - 2 * C0
    y = arena0[: n0 * C0 // 2].view(torch.bfloat16).view(n0, C0).float() if b16 else arena0[: n0 * C0].view(n0, C0)
    pooled = arena0[ny : ny + n1 * C0].view(n1, C0)
    mean, invstd = arena0[ny + n1 * C0 : ny + n1 * C0 + C0], arena0[ny + n1 * C0 + C0 : ny + n1 * C0 + 2 * C0]
    bn = model.bn1.bn
    gamma, beta = bn.weight.detach(), bn.bias.detach()
    conv_math = "bf16" if math == "bf16s" else math
    f_fwd = LW.conv_form("fwd", 27, x.shape[1], C0, conv_math, n_out=n0, ldx=x.stride(0))
    r_fwd = f_fwd.rounded
    ops = {"x": x, "w": w0.detach()}
    if b16:  # y is STORED as bf16: half an ulp of the float64 value on the rounded operands, and not of the unrounded one
        ref = LW.conv_fwd(nbr=nbr0, **LW.apply_rounding(ops, r_fwd))
        other = LW.conv_fwd(nbr=nbr0, **LW.apply_rounding(ops, frozenset()))
        assert LW.rounded_operands("store", 27, x.shape[1], C0, math) == {"y"}
        recs += LW.check_bf16_store("stem", "conv fwd (bf16 y)", y, ref)
        o = LW.check_bf16_store("stem", "conv fwd vs other", y, other)[0]
        o.ok, o.note = not o.ok, "must exceed the bound"
        recs.append(o)
    else:
        recs += _conv_recs("stem", "conv fwd", y, lambda x, w: LW.conv_fwd(x, w, nbr0), ops, f_fwd)
    recs += LW.check_stats("stem", "norm", mean, invstd, y, bn.eps)
    recs += LW.check_running("stem", before[bn], bn, y)
    # relu + pool: the forward's own ReLU decisions are those of the norm-gradient kernel (_stem_masks_of_hip_run)
    sm_bn, sm_w = (m.cuda() for m in _stem_masks_of_hip_run(out, model))
    z = LW.bn_fwd(y, gamma, beta, eps=bn.eps)
    flip = sm_bn != (z > 0)
    zf = float(z[flip].abs().max() / z.std()) if bool(flip.any()) else 0.0
    recs.append(LW.Record("stem", "relu flips", n0, tuple(z.shape), "fp32", zf, LW.FLIP_Z, zf <= LW.FLIP_Z, f"{int(flip.sum())} element(s)"))
    ref = LW.sum_pool(z * sm_bn, i2o, n1)
    recs += LW.check_scaled("stem", "norm+relu+pool fwd", pooled, ref, float(ref.abs().max()), rows=n1)
    # backward: the pooled gradient that reached the stem (block 0's input gradient)
    g = saved.g_stem_out
    dy, dga, dbe = LW.stem_bwd(g, y, gamma, beta, i2o, sm_bn, bn.eps)
    dz = g.double()[i2o.long()] * sm_bn.double()
    m64, is64 = LW.bn_stats(y, bn.eps)
    recs += LW.check_scaled("stem", "norm bwd dgamma", bn.weight.grad, dga, LW.reduction_scale(dz * (y.double() - m64) * is64), rows=n0)
    recs += LW.check_scaled("stem", "norm bwd dbeta", bn.bias.grad, dbe, LW.reduction_scale(dz), rows=n0)
    # conv1.kernel: dY is what the fused kernel recomputes (under its own ReLU decisions) -- fp32 values, rounded where declared
    r_w = LW.rounded_operands("wgrad", 27, x.shape[1], C0, conv_math, n_out=n0, ldx=x.stride(0))
    xs = x
    dy_w = LW.stem_bwd(g, y, gamma, beta, i2o, sm_w, bn.eps)[0]
    v = LW.stem_wgrad_operand(g, y, mean, invstd, gamma, beta, bn.weight.grad, bn.bias.grad, i2o, n0)
    decl = {"x": LW.bf16_rne(xs) if "x" in r_w else xs, "dy": LW.bf16_rne(v) if "dy" in r_w else dy_w}
    oth = {"x": xs if "x" in r_w else LW.bf16_rne(xs), "dy": dy_w if "dy" in r_w else LW.bf16_rne(v)}
    ref = LW.conv_wgrad(decl["x"], decl["dy"], nbr0)
    other = LW.conv_wgrad(oth["x"], oth["dy"], nbr0)
    recs += LW.check_conv("stem", "conv wgrad", model.conv1.kernel.grad, ref, r_w, other)
    return recs


def _block_records(i, st, saved, m, math, reach, L, before):
    recs = []
    arena, nbr1, nbr2, nbrd, ts_in, ts_out, n_in, n_out = saved[1 + i]
    C, cin = st.C, st.cin
    cnt = n_out * C
    y1, h1, y2, out = (arena[j * cnt : (j + 1) * cnt].view(n_out, C) for j in range(4))
    down = st.down is not None
    if i == 0:
        _, w0, arena0, _, nbr_pool, _, _, _, _ = saved.stem
        n1, C0 = nbr_pool.shape[0], w0.shape[-1]
        ny = arena0.numel() - n1 * C0 - 2 * C0
        x = arena0[ny : ny + n1 * C0].view(n1, C0)
    else:
        pa, _, _, _, _, _, _, pn = saved[i]
        pc = saved.plan.stages[i - 1].C
        x = pa[3 * pn * pc : 4 * pn * pc].view(pn, pc)
    assert x.shape == (n_in, cin)
    m1, is1, m2, is2, md, isd = saved.stats(i)
    W1, W2 = st.conv1.kernel.detach(), st.conv2.kernel.detach()
    n1m, n2m = st.norm1.bn, st.norm2.bn
    lay = f"block{i}"
    cm = "bf16" if math == "bf16s" else math
    fwd1, wg1 = (LW.conv_form(o, 27, cin, C, cm, n_out=n_out) for o in ("fwd", "wgrad"))
    dg1 = LW.conv_form("dgrad", 27, cin, C, cm, n_out=n_out, row_perm=down)
    fwd3, dg3, wg3 = (LW.conv_form(o, 27, C, C, cm, n_out=n_out) for o in ("fwd", "dgrad", "wgrad"))
    # ---- which launch forms this block's row counts reach (the planners decide by rows)
    ks1 = int(L.mink_conv_plan(n_out, 27, cin, C, 0))
    ks2 = int(L.mink_conv_plan(n_out, 27, C, C, 0))
    if max(ks1, ks2) > 1:
        reach.add("split-K")
    if n_out <= L.mink_bn_small_rows() and C % 16 == 0:
        reach.add("few-row")
    # ---- forward
    recs += _conv_recs(lay, "conv1 fwd", y1, lambda x, w: LW.conv_fwd(x, w, nbr1), {"x": x, "w": W1}, fwd1, reach)
    recs += LW.check_stats(lay, "norm1", m1, is1, y1, n1m.eps)
    recs += LW.check_running(lay + " norm1", before[n1m], n1m, y1)
    recs += LW.check_relu_out(lay, "norm1+relu fwd", h1, LW.bn_fwd(y1, n1m.weight, n1m.bias, eps=n1m.eps))
    recs += _conv_recs(lay, "conv2 fwd", y2, lambda x, w: LW.conv_fwd(x, w, nbr2), {"x": h1, "w": W2}, fwd3, reach)
    recs += LW.check_stats(lay, "norm2", m2, is2, y2, n2m.eps)
    recs += LW.check_running(lay + " norm2", before[n2m], n2m, y2)
    if down:
        yd, sd = arena[4 * cnt : 5 * cnt].view(n_out, C), arena[5 * cnt : 6 * cnt].view(n_out, C)
        Wd, ndm = st.down.kernel.detach(), st.normd.bn
        recs += _conv_recs(lay, "down fwd", yd, lambda x, w: LW.conv_fwd(x, w, nbrd), {"x": x, "w": Wd},
                           LW.conv_form("fwd", 1, cin, C, cm, n_out=n_out), reach)
        recs += LW.check_stats(lay, "normd", md, isd, yd, ndm.eps)
        recs += LW.check_running(lay + " normd", before[ndm], ndm, yd)
        ref = LW.bn_fwd(yd, ndm.weight, ndm.bias, eps=ndm.eps)
        recs += LW.check_scaled(lay, "normd fwd", sd, ref, float(ref.abs().max()))
        shortcut = sd
    else:
        shortcut = x
    recs += LW.check_relu_out(lay, "norm2+res+relu fwd", out, LW.bn_fwd(y2, n2m.weight, n2m.bias, shortcut, eps=n2m.eps))
    # ---- backward
    gs = saved.grad_stage(i)
    last = i == len(saved.plan.stages) - 1
    g_in = saved.g_out.view(n_out, C) if last else saved.grad_stage(i + 1)["g_x"]
    recs += LW.check_bn_bwd(lay, "norm2 bwd", gs["g_y2"], n2m.weight.grad, n2m.bias.grad, g_in, y2, n2m.weight, n2m.bias, out > 0,
                            got_dres=gs["g_res"], eps=n2m.eps)
    if down:
        recs += LW.check_bn_bwd(lay, "normd bwd", gs["g_yd"], ndm.weight.grad, ndm.bias.grad, gs["g_res"], yd, ndm.weight, ndm.bias, None,
                                eps=ndm.eps)
        recs += _conv_recs(lay, "down dgrad", gs["g_sc"], lambda dy, w: dy @ w[0].t(), {"dy": gs["g_yd"], "w": Wd},
                           LW.conv_form("dgrad", 1, cin, C, cm, n_out=n_out, row_perm=True), reach)
        recs += _conv_recs(lay, "down wgrad", st.down.kernel.grad, lambda x, dy: LW.conv_wgrad(x, dy, nbrd), {"x": x, "dy": gs["g_yd"]},
                           LW.conv_form("wgrad", 1, cin, C, cm, n_out=n_out), reach)
    recs += _conv_recs(lay, "conv2 dgrad", gs["g_h1"], lambda dy, w: LW.conv_dgrad(dy, w, nbr2, n_out), {"dy": gs["g_y2"], "w": W2}, dg3, reach)
    recs += _conv_recs(lay, "conv2 wgrad", st.conv2.kernel.grad, lambda x, dy: LW.conv_wgrad(x, dy, nbr2), {"x": h1, "dy": gs["g_y2"]}, wg3, reach)
    recs += LW.check_bn_bwd(lay, "norm1 bwd", gs["g_y1"], n1m.weight.grad, n1m.bias.grad, gs["g_h1"], y1, n1m.weight, n1m.bias, h1 > 0,
                            eps=n1m.eps)
    recs += _conv_recs(lay, "conv1 wgrad", st.conv1.kernel.grad, lambda x, dy: LW.conv_wgrad(x, dy, nbr1), {"x": x, "dy": gs["g_y1"]}, wg1, reach)
    if down:
        # the class-permuted strided data gradient: the kernel gathers through the transposed table in class order -- that form
        # of the reference must agree with the forward-table scatter (tables and permutation), then g_x as the composite
        ent = m.tables.get((ts_in, ts_out, 3, 1))
        perm = m.tables.get(("perm", ts_in, 128))
        assert ent is not None and ent[1] is not None and perm is not None, "the strided data gradient did not get its class-permuted tables"
        reach.add("class-permuted strided dgrad")
        gy = gs["g_y1"].double()
        a, b = LW.conv_dgrad(gy, W1, nbr1, n_in), LW.conv_dgrad_gather(gy, W1, ent[1], perm=perm)
        e = LW.conv_errors(b, a)[0]
        recs.append(LW.Record(lay, "conv1 dgrad tables", n_in, tuple(a.shape), "float64", e, 1e-12, e <= 1e-12, "transposed + perm vs scatter"))
        sc = LW.scatter_rows(gs["g_sc"], nbrd[:, 0], n_in)
        recs += _conv_recs(lay, "conv1 dgrad + down", gs["g_x"], lambda dy, w: LW.conv_dgrad(dy, w, nbr1, n_in) + sc,
                           {"dy": gs["g_y1"], "w": W1}, dg1, reach)
    else:
        stages = saved.plan.stages
        may_defer = i > 0 and stages[i - 1].level == st.level and stages[i - 1].C == cin
        deferred = may_defer and cin <= 1024 and int(L.mink_conv_plan(n_out, 27, C, cin, 0)) > 1
        if deferred:
            reach.add("deferred identity")
        else:
            recs += _conv_recs(lay, "conv1 dgrad", gs["g_xa"], lambda dy, w: LW.conv_dgrad(dy, w, nbr1, n_in), {"dy": gs["g_y1"], "w": W1}, dg1, reach)
        res = gs["g_res"].double()
        recs += _conv_recs(lay, "conv1 dgrad + res" + (" (deferred)" if deferred else ""), gs["g_x"],
                           lambda dy, w: LW.conv_dgrad(dy, w, nbr1, n_in) + res, {"dy": gs["g_y1"], "w": W1}, dg1, reach)
    return recs


@pytest.mark.timeout(60)
@pytest.mark.parametrize("name,batch,math,expect", [
    ("ResNet14", 16, "fp32", {"few-row", "split-K", "class-permuted strided dgrad"}),
    ("ResNet14", 16, "bf16", {"few-row", "split-K", "class-permuted strided dgrad", "form: dense gather_gemm2 bf16",
                              "form: class-permuted compact bf16", "form: dense_xwt", "form: wgrad16<1>"}),
    ("ResNet14", 16, "bf16s", {"few-row", "split-K", "class-permuted strided dgrad", "form: class-permuted compact bf16"}),
    ("ResNet34", 4, "fp32", {"few-row", "split-K", "class-permuted strided dgrad", "deferred identity"}),
    ("ResNet14", 16, "bf16x3", {"few-row", "split-K", "class-permuted strided dgrad", "form: dense gather_gemm2 bf16x3",
                                "form: staged gather_gemm2 (transposed weights) bf16x3", "form: dense_xwt", "form: wgrad fp32"}),
])
def test_every_operator_teacher_forced_against_float64(name, batch, math, expect):
    """Bench.py's own step (three passes, maps prepared ahead, forked shortcut, flat gradient sink) at BASELINE's shapes; from its
    last pass every forward and backward operator of the stem and of every block, and every parameter gradient as it sits in
    the flat buffer, against float64 fed with that pass's own stored inputs (bounds: tests/layerwise.py).  Each convolution is
    judged on what its launch form multiplies (layerwise.conv_form: bf16-rounded, split-bf16 or exact fp32 operands), and the
    forms reached ("form: ...") are part of what each configuration must reach."""
    from nerf_downstream_amd._lib import lib
    from nerf_downstream_amd.minkowski import functional as Fn
    from nerf_downstream_amd.minkowski import trunk

    b = _baseline_batch(batch=batch)
    hip = _pair(name)
    old = Fn.set_conv_math("bf16" if math == "bf16s" else math), Fn.set_conv_storage("bf16" if math == "bf16s" else "fp32")
    trunk.KEEP_GRAD_ARENA = True
    before = {}  # every batch norm's running statistics before the last pass (layerwise.check_running)
    try:
        out, field, reducer = _bench_like_step(hip, {"coordinates": b["coordinates"].cuda(), "features": b["features"].cuda()},
                                               b["labels"].long().cuda(), before_last_pass=lambda: before.update(LW.running_snapshot(hip)))
    finally:
        trunk.KEEP_GRAD_ARENA = False
        Fn.set_conv_math(old[0]), Fn.set_conv_storage(old[1])
    node = trunk_node(out)
    assert hip._trunk_plan and node is not None, "the native trunk (bench.py's path) was not taken"
    assert field.coordinate_manager.prepared, "the last pass must run on maps prepared ahead"
    saved = node.saved
    assert saved.g_buf is not None, "the gradient arena was not kept"
    assert saved[0][7] is (math == "bf16s"), "bf16 storage of the stem taken iff asked for"
    lo, hi = reducer.flat.data_ptr(), reducer.flat.data_ptr() + 4 * reducer.flat.numel()
    assert all(lo <= p.grad.data_ptr() < hi for p in hip.parameters()), "parameter gradients must be read where the bench keeps them"
    L = lib()
    reach = set()
    with torch.no_grad():
        recs = _stem_records(saved, hip, out, math, before)
        for i, st in enumerate(node.plan.stages):
            recs += _block_records(i, st, saved, field.coordinate_manager, math, reach, L, before)
    assert len(before) == sum(1 for r in recs if r.op == "running var"), "a batch norm's running statistics went unchecked"
    # every parameter gradient of the trunk was checked against its operator's float64 backward
    checked = {r.op for r in recs}
    n_blocks = len(node.plan.stages)
    assert sum(1 for r in recs if r.op.endswith("wgrad") and not r.op.endswith("vs other")) == 1 + 2 * n_blocks + \
        sum(s.down is not None for s in node.plan.stages)
    assert {"conv1 fwd", "conv2 fwd", "norm1 bwd dx", "norm2 bwd dgamma", "conv2 dgrad"} <= checked
    bad = LW.report(recs, f"{name} B={batch} {math}", force=False)
    print(f"[{name} B={batch} {math}] {len(recs)} checks over the stem and {n_blocks} blocks; paths reached: {sorted(reach)}; "
          f"worst conv error {max(r.err for r in recs if r.bound == LW.CONV_REL and not r.op.endswith('vs other')):.2e}")
    assert not bad, [r.line() for r in bad]
    assert expect <= reach, ("launch paths this configuration must reach", sorted(expect - reach))
