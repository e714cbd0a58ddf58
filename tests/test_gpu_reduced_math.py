"""The convolution kernels under reduced math (set_conv_math "bf16" and "bf16x3"), launch form by launch form, against a float64
restatement of exactly what each form computes -- on synthetic tables in the style of test_gpu_ops.py
test_row_compacted_kernel_against_float64: ragged row counts (1, 63, 65, a few thousand), an offset nobody has, one a whole
64-row tile lacks.

What a form computes is read from the shape-aware rounding table (layerwise.conv_form, a restatement of gather_gemm_impl in
csrc/conv.hip and wgrad_plan in csrc/conv_wgrad.hip):
  * bf16 forms:    float64 over bf16_rne(x) and bf16_rne(w) (or dY);
  * bf16x3 forms:  float64 over the three products xh*wh + xh*wl + xl*wh, h = rne(v) and l = rne(v - h) taken in fp32
                   (conv_common.h pack_bf16 / conv.hip bf16_residual; layerwise.bf16_split);
  * fp32 forms:    float64 over the fp32 operands (the scalar gather_gemm_kernel has no MATH parameter, and the weight
                   gradients outside wgrad16_kernel / the bf16 streaming kernel stay exact fp32 under every math mode).

The bound comes from fp32 accumulation alone, the way test_gpu_ops._chain_tolerance measures it: the same declared products
summed one fused step at a time in fp32 against the same float64 reference, twice that (the MFMAs add several products per step
in another association), and never less than a floor of a few fp32 ulps of the output (REL_FLOOR, MAX_FLOOR).  Each case is also
held OUTSIDE that bound of the references it must not match -- the other rounding (as layerwise.check_conv's "declared vs
other"), bf16 truncation instead of round-to-nearest-even, and for bf16x3 the one-plane form, a dropped hi*lo product and a
truncated lo plane -- wherever that reference sits more than SEP bounds from the declared one.
The lo*lo product bf16x3 leaves out is at most 2^-16 of a product (~2^-18 RMS, ~3e-6 of a reduction's L2 norm:
tests/test_reduced_math_cpu.py): the size of the bound itself, so no case relies on resolving it -- the exact-fp32 reference
is a control for bf16x3 only where it sits SEP bounds away, while the one-plane form, a dropped hi*lo product (2^-9) and a
truncated lo plane (~8e-6 of the norm) sit well outside."""
import pytest
import torch

import layerwise as LW
from helpers import class_perm

pytestmark = pytest.mark.gpu

REL_FLOOR, MAX_FLOOR = 1e-6, 2e-6  # relative L2 / max |err| / max |ref|: a few fp32 ulps of the output
SEP = 3.0  # a control is asserted where its reference sits at least this many bounds from the declared one


def _dev():
    return torch.device("cuda", 0)


def _table(n_out, K, n_in, g):
    nbr = torch.randint(0, n_in, (n_out, K), generator=g, dtype=torch.int32)
    nbr[torch.rand(n_out, K, generator=g) < 0.45] = -1  # the mid-layer fill
    if K > 1:
        nbr[:, K // 2 - 1] = -1  # an offset nobody has
    if n_out > 128:
        nbr[64:128, min(1, K - 1)] = -1  # ... and one that a whole tile lacks
    return nbr


def _class_perm(n_out, g):
    """Rows grouped by eight classes, every segment padded with -1 to a multiple of 128 (mink_class_partition's form)."""
    return class_perm(torch.randint(0, 8, (n_out,), generator=g))


def _strided(n, c, ld, g, dev):
    """[n, c] fp32 rows on `dev` at row stride `ld` (a view of a wider tensor when ld > c: made there, since copying a view
    to the device packs it)."""
    return torch.randn(n, ld, generator=g).to(dev)[:, :c]


# ------------------------------------------------------------------------------------------------ products of a form
def _pairs(a, b, kind):
    """The (left, right) operand pairs whose products a form sums, in the kernel's order (smallest terms first for bf16x3).
    kind: "fp32", "bf16", "bf16 trunc", "bf16x3", "bf16x3 one plane", "bf16x3 no hi*lo", "bf16x3 lo trunc"."""
    if kind == "fp32":
        return [(a.float(), b.float())]
    if kind in ("bf16", "bf16 trunc"):
        r = LW.bf16_rne if kind == "bf16" else LW.bf16_trunc
        return [(r(a.float()), r(b.float()))]
    ah, al = LW.bf16_split(a, LW.bf16_trunc if kind == "bf16x3 lo trunc" else LW.bf16_rne)
    bh, bl = LW.bf16_split(b, LW.bf16_trunc if kind == "bf16x3 lo trunc" else LW.bf16_rne)
    if kind == "bf16x3 one plane":
        return [(ah, bh)]
    if kind == "bf16x3 no hi*lo":
        return [(al, bh), (ah, bh)]
    return [(al, bh), (ah, bl), (ah, bh)]


def _declared_kind(cf, math):
    if not cf.rounded:
        return "fp32"
    return "bf16x3" if cf.split else "bf16"


def _controls(declared, math):
    """The references a kernel of the `declared` kind must NOT match."""
    if declared == "bf16":
        return ["fp32", "bf16 trunc"]
    if declared == "bf16x3":
        return ["fp32", "bf16x3 one plane", "bf16x3 no hi*lo", "bf16x3 lo trunc"]
    return ["bf16x3" if math == "bf16x3" else "bf16"]  # an exact-fp32 form: the rounding the math mode would have applied


def _errs(got, ref):
    got, ref = got.double(), ref.double()
    d = got - ref
    return float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300))


class Judge:
    """Collects (case, form, error, bound) lines and failures of one family of cases."""

    def __init__(self):
        self.lines, self.fails, self.forms = [], [], {}

    def judge(self, case, form, got, ref_fn, seq_fn, declared, math):
        ref = ref_fn(declared)
        rel_s, max_s = _errs(seq_fn(declared), ref)
        tol_r, tol_m = max(REL_FLOOR, 2.0 * rel_s), max(MAX_FLOOR, 2.0 * max_s)
        rel, mx = _errs(got, ref)
        ok = rel <= tol_r and mx <= tol_m
        worst = max(rel / tol_r, mx / tol_m)
        self.forms[form] = max(self.forms.get(form, 0.0), worst)
        line = f"{case:46s} {form:52s} {declared:7s} rel {rel:.1e} <= {tol_r:.1e}  max {mx:.1e} <= {tol_m:.1e}"
        if not ok:
            self.fails.append(line)
        for ctl in _controls(declared, math):
            cref = ref_fn(ctl)
            sep_r, sep_m = _errs(cref, ref)
            if sep_r < SEP * tol_r and sep_m < SEP * tol_m:
                line += f"  [{ctl}: {sep_r:.1e} apart, too close]"
                continue
            r_o, m_o = _errs(got, cref)
            if r_o <= tol_r and m_o <= tol_m:
                self.fails.append(f"{case} {form}: within the bound of {ctl!r} (rel {r_o:.1e}, max {m_o:.1e})")
            line += f"  [{ctl}: {r_o:.1e}]"
        self.lines.append(line)

    def finish(self, title, expected):
        print(f"\n{title}")
        for ln in self.lines:
            print("  " + ln)
        print("  forms reached (worst error / bound):")
        for f, w in sorted(self.forms.items()):
            print(f"    {f:60s} {w:.2f}")
        missing = set(expected) - set(self.forms)
        assert not self.fails, "\n".join(self.fails)
        assert not missing, f"launch forms not reached: {sorted(missing)}"


# ------------------------------------------------------------------------------------------------ gather-GEMM (fwd, dgrad)
def _gather64(a, b, nbr):
    """float64 sum_k a[nbr[:, k]] @ b[k]: a [n_in, gin], b [K, gin, gout]."""
    out = torch.zeros(nbr.shape[0], b.shape[2], dtype=torch.float64, device=a.device)
    for k in range(nbr.shape[1]):
        sel = nbr[:, k] >= 0
        out[sel] += a[nbr[sel, k].long()] @ b[k]
    return out


def _gather_seq32(pairs, nbr):
    """The same products summed one fused fp32 step at a time, offsets and channels ascending."""
    a0, b0 = pairs[0]
    s = torch.zeros(nbr.shape[0], b0.shape[2], dtype=torch.float32, device=a0.device)
    for k in range(nbr.shape[1]):
        sel = (nbr[:, k] >= 0)[:, None]
        rows = nbr[:, k].clamp_min(0).long()
        gath = [(torch.where(sel, a[rows], torch.zeros((), device=a.device)), b[k]) for a, b in pairs]
        for c in range(b0.shape[1]):
            for xa, bk in gath:
                s.addcmul_(xa[:, c : c + 1], bk[c][None, :])
    return s


GATHER_CASES = [
    # (name, op, n_out, K, cin, cout, options)   cin / cout: the convolution's (W [K, cin, cout])
    ("fwd dense 3000x27", "fwd", 3000, 27, 64, 64, {}),
    ("fwd dense 65x8 cout 96", "fwd", 65, 8, 64, 96, {}),
    ("fwd dense 63x1", "fwd", 63, 1, 64, 64, {}),
    ("fwd dense 1x27", "fwd", 1, 27, 64, 64, {}),
    ("dgrad dense 3000x27", "dgrad", 3000, 27, 64, 64, {}),
    ("dgrad dense 65x8", "dgrad", 65, 8, 96, 64, {}),
    ("dgrad dense 63x1", "dgrad", 63, 1, 128, 64, {}),
    ("tconv fwd staged 2000x8", "fwd", 2000, 8, 64, 64, {"perm": True}),
    ("tconv fwd staged 1000x1", "fwd", 1000, 1, 64, 64, {"perm": True}),
    ("dgrad class-permuted 2000x27", "dgrad", 2000, 27, 64, 64, {"perm": True}),
    ("dgrad class-permuted 2000x8", "dgrad", 2000, 8, 128, 64, {"perm": True}),
    ("dgrad class-permuted 2000x27 dense (bit 27)", "dgrad", 2000, 27, 64, 64, {"perm": True, "perm16": False}),
    ("dgrad class-permuted 1500x8 48 (tail)", "dgrad", 1500, 8, 48, 48, {"perm": True}),
    ("fwd stem flat 3000x27 cin 28", "fwd", 3000, 27, 28, 64, {}),
    ("fwd stem flat 3000x27 cin 28 ldx 32", "fwd", 3000, 27, 28, 64, {"ldx": 32}),
    ("fwd tail 1000x27 cin 48", "fwd", 1000, 27, 48, 64, {}),
    ("fwd tail 1000x27 cin 20", "fwd", 1000, 27, 20, 32, {}),
    ("dgrad tail 1000x27 cout 48", "dgrad", 1000, 27, 64, 48, {}),
    ("fwd scalar 1000x27 cin 27", "fwd", 1000, 27, 27, 64, {}),
    ("fwd scalar 1000x27 ldx 30", "fwd", 1000, 27, 28, 64, {"ldx": 30}),
    ("dgrad scalar 1000x8 cout 27", "dgrad", 1000, 8, 64, 27, {}),
    ("fwd split-K 3 + stats 3000x27", "fwd", 3000, 27, 64, 64, {"ksplit": 3, "stats": True}),
    ("fwd un-split + stats 3000x27", "fwd", 3000, 27, 64, 64, {"ksplit": 1, "stats": True}),
    ("fwd split-K 4 + stats 1000x8", "fwd", 1000, 8, 64, 64, {"ksplit": 4, "stats": True}),
    ("dgrad split-K 7 3000x27", "dgrad", 3000, 27, 64, 64, {"ksplit": 7}),
]

_GG2 = ["dense gather_gemm2", "dense gather_gemm2 (transposed weights)", "staged gather_gemm2 (transposed-conv fwd)",
        "staged gather_gemm2 (transposed weights)", "staged gather_gemm2 (transposed weights) + channel tail",
        "flat gather_gemm2 (cin 28)", "dense gather_gemm2 + channel tail",
        "dense gather_gemm2 (transposed weights) + channel tail"]
GATHER_FORMS = {
    "bf16": [f + " bf16" for f in _GG2] + ["class-permuted compact bf16", "scalar gather_gemm", "split-K", "stats direct", "stats split"],
    "bf16x3": [f + " bf16x3" for f in _GG2] + ["scalar gather_gemm", "split-K", "stats direct", "stats split"],
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("math", ["bf16", "bf16x3"])
def test_gather_gemm_forms_under_reduced_math_against_float64(math):
    """Forward and data-gradient gather-GEMMs: the dense gather_gemm2 form at K = 27 / 8 / 1, the staged (class-permuted) form
    with and without transposed weights (the transposed-convolution forward), the compact bf16 data gradient and the dense one
    it replaces (set_stagger bit 27), the flat cin = 28 stem form, channel tails, the scalar form (cin = 27, ldx % 4 != 0:
    exact fp32 under every math), split-K with the direct and split statistics epilogues."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd._lib import lib
    from nerf_downstream_amd.minkowski import functional as Fn

    dev = _dev()
    L = lib()
    J = Judge()
    old = ME.set_conv_math(math)
    try:
        for ci, (name, op, n_out, K, cin, cout, o) in enumerate(GATHER_CASES):
            perm16 = o.get("perm16", True)
            if not perm16 and math != "bf16":
                continue  # (the class-permuted compact form exists under bf16 math only)
            g = torch.Generator().manual_seed(1000 * ci + n_out + K)
            perm = _class_perm(n_out, g) if o.get("perm") else None
            n_in = max(4, n_out // 3 + 5) if perm is not None else max(4, n_out + 17)
            nbr = _table(n_out, K, n_in, g)
            gin, gout = (cout, cin) if op == "dgrad" else (cin, cout)
            ldx = o.get("ldx", gin)
            srcd = _strided(n_in, gin, ldx, g, dev)
            w = torch.randn(K, cin, cout, generator=g) * 0.1
            if op == "dgrad":  # the kernel reads W[k] as [cout][cin]; the same-map form flips k, the class-permuted one does not
                wr = w.transpose(1, 2)
                b = wr.flip(0) if perm is None else wr
            else:
                b = w
            wd, nd = w.to(dev), nbr.to(dev)
            pd = perm.to(dev) if perm is not None else None
            ks = o.get("ksplit", 1 if gin == 28 else 0)
            Fn._FORCE_KSPLIT = ks
            Fn._PLAN_CACHE.clear()
            L.mink_conv_set_stagger(0 if perm16 else 1 << 27)
            ks_eff = ks or Fn._plan_ksplit(L, n_out if perm is None else perm.numel(), K, gin, gout, int(perm is not None))
            cf = LW.conv_form(op, K, cin, cout, math, n_out=n_out, ldx=ldx, row_perm=perm is not None, ksplit=ks_eff, perm16=perm16,
                              shortcut_dense=False)
            part = None
            if op == "dgrad":
                y = Fn.gather_gemm(srcd, wd, nd, gout, w_transposed=True, flip_k=perm is None, row_perm=pd)
            elif o.get("stats"):
                y, part = Fn.gather_gemm(srcd, wd, nd, gout, stats=True)
            else:
                y = Fn.gather_gemm(srcd, wd, nd, gout, row_perm=pd)
            L.mink_conv_set_stagger(0)
            bd = b.to(dev)
            ref_fn = lambda kind: sum(_gather64(p.double(), q.double(), nd) for p, q in _pairs(srcd, bd, kind))  # noqa: E731
            seq_fn = lambda kind: _gather_seq32(_pairs(srcd, bd, kind), nd)  # noqa: E731
            J.judge(f"{name} ({op})", cf.form, y, ref_fn, seq_fn, _declared_kind(cf, math), math)
            zs = -(-K // -(-K // ks_eff)) if cf.form != "class-permuted compact bf16" else 1
            if zs > 1:
                J.forms.setdefault("split-K", 0.0)
            if part is not None or o.get("stats"):
                assert part is not None, f"{name}: no statistics partials"
                tag = "stats split" if zs > 1 else "stats direct"
                yd = y.double()
                s = part.sum(0)
                e0 = float(((s[0] - yd.sum(0)).abs() / yd.abs().sum(0).clamp_min(1e-30)).max())
                e1 = float(((s[1] - (yd * yd).sum(0)).abs() / (yd * yd).sum(0).clamp_min(1e-30)).max())
                J.forms[tag] = max(J.forms.get(tag, 0.0), max(e0, e1) / 1e-5)
                if max(e0, e1) > 1e-5:  # fp32 sums of y's own values, per partial row
                    J.fails.append(f"{name}: {tag} column sums off by {e0:.1e} / {e1:.1e}")
    finally:
        Fn._FORCE_KSPLIT = 0
        L.mink_conv_set_stagger(0)
        Fn._PLAN_CACHE.clear()
        ME.set_conv_math(old)
    J.finish(f"gather-GEMM forms under {math}", GATHER_FORMS[math])


# ------------------------------------------------------------------------------------------------ weight gradient
def _wgrad64(a, b, nbr):
    """float64 dW[k] = a[nbr[:, k]]^T b."""
    K = nbr.shape[1]
    out = torch.zeros(K, a.shape[1], b.shape[1], dtype=torch.float64, device=a.device)
    for k in range(K):
        sel = nbr[:, k] >= 0
        out[k] = a[nbr[sel, k].long()].T @ b[sel]
    return out


def _wgrad_seq32(pairs, nbr, chunk=1):
    """The same products summed row by row in fp32 (every row's outer products one fused step each)."""
    a0, b0 = pairs[0]
    K = nbr.shape[1]
    rows = nbr.clamp_min(0).long()
    live = (nbr >= 0).float()
    s = torch.zeros(K, a0.shape[1], b0.shape[1], dtype=torch.float32, device=a0.device)
    gath = [(a[rows] * live[:, :, None], b) for a, b in pairs]  # [n_out, K, cin]
    for o in range(nbr.shape[0]):
        for xa, bb in gath:
            s.addcmul_(xa[o][:, :, None], bb[o][None, None, :])
    return s


WGRAD_CASES = [
    # (name, n_out, K, cin, cout, force (set_stagger bits 12-26: G code | row splits << 4), ldx)
    ("wgrad 1000x27 64 G1 z1", 1000, 27, 64, 64, 1 | (1 << 4), None),
    ("wgrad 1000x27 64 G1 z4", 1000, 27, 64, 64, 1 | (4 << 4), None),
    ("wgrad 1000x27 64->128 G3 z1", 1000, 27, 64, 128, 2 | (1 << 4), None),
    ("wgrad 1000x27 128 G3 z4", 1000, 27, 128, 128, 2 | (4 << 4), None),
    ("wgrad 1000x27 64 G9 (fp32 kernel)", 1000, 27, 64, 64, 3 | (2 << 4), None),
    ("wgrad 530x27 256 plan", 530, 27, 256, 256, 0, None),
    ("wgrad 1000x8 64 G3 z1 (partial group)", 1000, 8, 64, 64, 2 | (1 << 4), None),
    ("wgrad 4097x8 64 G3 z4 (partial group)", 4097, 8, 64, 64, 2 | (4 << 4), None),
    ("wgrad 1000x8 128->64 G1 z4", 1000, 8, 128, 64, 1 | (4 << 4), None),
    ("wgrad 4097x1 64->128 plan", 4097, 1, 64, 128, 0, None),
    ("wgrad 63x1 128 plan", 63, 1, 128, 128, 0, None),
    ("wgrad 1000x27 48 (fp32 widths)", 1000, 27, 48, 64, 0, None),
    ("wgrad 1000x27 96 (fp32 widths)", 1000, 27, 96, 96, 0, None),
    ("wgrad 1000x8 96->48 (fp32 widths)", 1000, 8, 96, 48, 0, None),
    ("wgrad 100x27 96->48 (fp32 widths)", 100, 27, 96, 48, 0, None),
    ("wgrad 1000x1 64 ldx 66 (fp32: stride)", 1000, 1, 64, 64, 0, 66),
    ("wgrad stem 6000x27 cin 3 G9", 6000, 27, 3, 64, 3, None),
    ("wgrad stem 6000x27 cin 20 G9", 6000, 27, 20, 64, 3, None),
    ("wgrad stem 6000x27 cin 28 G9", 6000, 27, 28, 64, 3, None),
    ("wgrad stem 6000x27 cin 32 G9", 6000, 27, 32, 32, 3, None),
]

WGRAD_FORMS = {
    "bf16": ["wgrad16<1> G1", "wgrad16<1> G1 split", "wgrad16<3> G3", "wgrad16<3> G3 split", "wgrad fp32 G9 split",
             "wgrad_stream_bf16 G9 split", "wgrad fp32 G1", "wgrad fp32 G1 split"],
    "bf16x3": ["wgrad fp32 G1", "wgrad fp32 G3", "wgrad fp32 G9 split", "wgrad_stream G9 split"],
}


@pytest.mark.timeout(300)
@pytest.mark.parametrize("math", ["bf16", "bf16x3"])
def test_weight_gradient_forms_under_reduced_math_against_float64(math):
    """Weight gradients: wgrad16_kernel (bf16 operands) at K = 27 / 8 / 1 under forced G = 1 / 3 / 9 and forced row splits
    (set_stagger bits 12-26, conv_wgrad.hip wgrad_plan, g_conv.wgrad_force), K = 8 with G = 3 (a partial last group), one and several row splits;
    widths that must stay on the exact-fp32 kernel (48, 96, a row stride that is not a multiple of 4); the streaming bf16 stem
    kernel at cin = 3 / 20 / 28 / 32 -- against float64 on the operands the table declares (bf16x3 math: every weight gradient is
    exact fp32)."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd._lib import lib
    from nerf_downstream_amd.minkowski import functional as Fn

    dev = _dev()
    L = lib()
    J = Judge()
    old = ME.set_conv_math(math)
    try:
        for ci, (name, n_out, K, cin, cout, force, ldx) in enumerate(WGRAD_CASES):
            g = torch.Generator().manual_seed(7000 + 31 * ci + n_out)
            n_in = max(4, n_out + 17)
            nbr = _table(n_out, K, n_in, g)
            xd = _strided(n_in, cin, ldx or cin, g, dev)
            dyd, nd = torch.randn(n_out, cout, generator=g).to(dev), nbr.to(dev)
            L.mink_conv_set_stagger(force << 12)
            Fn._PLAN_CACHE.clear()  # (the workspace size follows the forced plan)
            cf = LW.conv_form("wgrad", K, cin, cout, math, n_out=n_out, ldx=ldx or cin, force_g=force)
            dw = Fn.conv_wgrad(xd, dyd, nd, (K, cin, cout))
            L.mink_conv_set_stagger(0)
            ref_fn = lambda kind: sum(_wgrad64(p.double(), q.double(), nd) for p, q in _pairs(xd, dyd, kind))  # noqa: E731
            seq_fn = lambda kind: _wgrad_seq32(_pairs(xd, dyd, kind), nd)  # noqa: E731
            # (the weight gradient has no split form: its controls are the bf16 roundings of x and dY)
            declared = "bf16" if cf.rounded else "fp32"
            J.judge(name, cf.form, dw, ref_fn, seq_fn, declared, "bf16")
    finally:
        L.mink_conv_set_stagger(0)
        Fn._PLAN_CACHE.clear()
        ME.set_conv_math(old)
    J.finish(f"weight-gradient forms under {math}", WGRAD_FORMS[math])
