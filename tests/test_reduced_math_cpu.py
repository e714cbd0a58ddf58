"""CPU checks of the reduced-math restatements the GPU tests rely on (tests/test_gpu_reduced_math.py, tests/test_gpu_layerwise.py):

  * the shape-aware rounding table (layerwise.conv_form) at every convolution of Mink-ResNet14, ResNet50 and Res16UNet14 /
    14A / 18A -- what it must say where the old shape-blind table was wrong, that it agrees with that table on ResNet14's
    block shapes, and that every launch form those layers reach is one the GPU kernel matrix launches;
  * the three-product split-bf16 restatement: bf16 products are exact in fp32, three products land within 2^-16 of the exact
    product, and the GPU matrix's bound rejects emulated kernels that are subtly wrong (one plane, a dropped hi*lo product,
    truncation instead of round-to-nearest-even)."""
import pytest
import torch

import layerwise as LW
import test_gpu_reduced_math as RM

MODELS = [("ResNet14", 28), ("ResNet50", 28), ("Res16UNet14", 3), ("Res16UNet14A", 3), ("Res16UNet18A", 3)]
ROWS = (900, 40_000, 400_000)  # a coarse level, a bench-size mid level, a full-resolution ScanNet level


def _layers(name, cin):
    """(layer, kind, K, cin, cout, stride) of every convolution: kind "conv", "tconv" or "pointwise" (use_mm)."""
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.minkowski.modules import MinkowskiConvolutionTranspose

    torch.manual_seed(0)
    model = get_model(name, cin, 20)
    out = []
    for lname, mod in model.named_modules():
        kern = getattr(mod, "kernel", None)
        if not isinstance(kern, torch.Tensor):
            continue
        if kern.dim() == 2:
            out.append((lname, "pointwise", 1, kern.shape[0], kern.shape[1], 1))
        else:
            kind = "tconv" if isinstance(mod, MinkowskiConvolutionTranspose) else "conv"
            out.append((lname, kind, kern.shape[0], kern.shape[1], kern.shape[2], mod.stride))
    return out


def _layer_forms(kind, K, cin, cout, stride, math, n_out, first):
    """{op: ConvForm} the launches of one layer take (functional.py ConvolutionFunction / PointwiseConvolutionFunction)."""
    forms = {}
    if kind == "pointwise":  # forward and data gradient are library GEMMs; the weight gradient the K = 1 identity table
        forms["wgrad"] = LW.conv_form("wgrad", 1, cin, cout, math, n_out=n_out)
        return forms
    cin_fwd = cin + (-cin) % 4 if first else cin  # the stem's input carries no gradient: one zero column (ConvolutionFunction)
    forms["fwd"] = LW.conv_form("fwd", K, cin_fwd, cout, math, n_out=n_out, row_perm=kind == "tconv")
    if not first:
        forms["dgrad"] = LW.conv_form("dgrad", K, cin, cout, math, n_out=n_out, row_perm=kind == "conv" and stride > 1)
    forms["wgrad"] = LW.conv_form("wgrad", K, cin_fwd, cout, math, n_out=n_out)
    return forms


def _family(form):
    return form.split(" G")[0]


@pytest.mark.parametrize("name,cin", MODELS)
def test_rounding_table_at_every_layer_shape(name, cin):
    layers = _layers(name, cin)
    gpu_forms = {m: set(RM.GATHER_FORMS[m]) | {_family(f) for f in RM.WGRAD_FORMS["bf16"] + RM.WGRAD_FORMS["bf16x3"]}
                 for m in ("bf16", "bf16x3")}
    wgrad_kinds = set()
    for lname, kind, K, ci, co, stride in layers:
        first = lname == layers[0][0]
        for n_out in ROWS:
            for math in ("bf16", "bf16x3"):
                f = _layer_forms(kind, K, ci, co, stride, math, n_out, first)
                for op, cf in f.items():
                    where = f"{name} {lname} {op} {K}x{ci}->{co} rows {n_out} {math}"
                    fam = _family(cf.form)
                    # (mink_dense_xwt, exact fp32 under every math, has its own test: test_gpu_ops.test_shortcut_data_gradient_pieces)
                    assert fam in gpu_forms[math] | {"dense_xwt"}, f"{where}: {cf.form!r} is not launched by the GPU kernel matrix"
                    if op == "wgrad":
                        if math == "bf16x3":  # split-bf16 exists in the gather-GEMMs only
                            assert not cf.rounded, where
                        elif ci % 64 or co % 64:  # wgrad16_kernel takes 64-multiple widths only; the stem streams
                            assert bool(cf.rounded) == (fam == "wgrad_stream_bf16"), where
                        if math == "bf16":
                            wgrad_kinds.add(bool(cf.rounded))
                    elif cf.form == "dense_xwt":  # the strided 1x1x1 shortcut's data gradient: exact fp32 dense GEMM
                        assert op == "dgrad" and K == 1 and stride > 1, where
                        assert not cf.rounded, where
                    else:  # every gather of 16-byte rows rounds (bf16) or splits (bf16x3) both operands
                        assert cf.rounded == ({"dy", "w"} if op == "dgrad" else {"x", "w"}), where
                        assert cf.split == (math == "bf16x3"), where
                    if kind == "tconv" and op == "fwd":  # class permutation without transposed weights: the staged form
                        assert fam.startswith("staged gather_gemm2 (transposed-conv fwd)"), where
    if name.startswith("Res16UNet"):
        assert wgrad_kinds == {True, False}, "Res16UNet mixes bf16 and exact-fp32 weight gradients under bf16 math"


def test_rounding_table_keeps_the_resnet14_cases():
    """On ResNet14's blocks the shape-aware table says what the shape-blind one said -- forward x, w; data gradient dY, w except
    the 1x1x1 strided shortcut's; weight gradient x, dY -- wherever wgrad_plan keeps G < 9 (so tests/test_gpu_layerwise.py's bf16
    cases hold their bounds unchanged).  Where the plan takes G = 9 (wide layers at many rows) the weight gradient runs on the
    exact-fp32 kernel, and the old table was wrong there."""
    legacy = {"fwd": {"x", "w"}, "dgrad": {"dy", "w"}, "wgrad": {"x", "dy"}}
    g9 = 0
    for lname, kind, K, ci, co, stride in [l for l in _layers("ResNet14", 28) if l[0].startswith("layer")]:
        for n_out in (300, 2000, 9000, 50_000):
            f = _layer_forms(kind, K, ci, co, stride, "bf16", n_out, False)
            for op, cf in f.items():
                want = set() if (op == "dgrad" and K == 1) else legacy[op]
                if op == "wgrad" and LW.wgrad_plan(n_out, K, ci, co)[0] == 9:
                    want, g9 = set(), g9 + 1
                assert cf.rounded == want, (lname, op, n_out, cf)
    assert g9 > 0


def test_rounding_table_where_the_shape_blind_table_was_wrong():
    cf = LW.conv_form
    # the scalar gather (27 channels; a row stride that is not a multiple of 4) has no MATH parameter
    assert cf("fwd", 27, 27, 64, "bf16").rounded == frozenset()
    assert cf("fwd", 27, 28, 64, "bf16", ldx=30).form == "scalar gather_gemm"
    # the 32 / 48 / 96-wide weight gradients of Res16UNet stay exact fp32 under bf16 math; 64-multiples round
    for ci, co in ((32, 32), (48, 96), (96, 96), (64, 96)):
        assert cf("wgrad", 27, ci, co, "bf16", n_out=5000).rounded == frozenset(), (ci, co)
    assert cf("wgrad", 27, 64, 128, "bf16", n_out=5000).form.startswith("wgrad16<")
    # the K = 8 down convolution's weight gradient at a large level: wgrad16 with G = 3 (a partial last group of two offsets)
    assert cf("wgrad", 8, 64, 64, "bf16", n_out=60_000).form.startswith("wgrad16<3> G3")
    assert cf("wgrad", 1, 128, 128, "bf16", n_out=60_000).form.startswith("wgrad16<1> G1")
    # ... and a 64-wide weight gradient whose plan takes G = 9 away from the stem shape: the exact-fp32 kernel
    assert cf("wgrad", 27, 64, 64, "bf16", n_out=200_000).rounded == frozenset()
    # the transposed convolution's forward: class permutation without transposed weights -> staged gather_gemm2, not compact
    assert cf("fwd", 8, 256, 128, "bf16", row_perm=True).form == "staged gather_gemm2 (transposed-conv fwd) bf16"
    assert cf("dgrad", 8, 128, 256, "bf16", row_perm=True).form == "class-permuted compact bf16"
    assert cf("dgrad", 8, 128, 256, "bf16", row_perm=True, perm16=False).form == "staged gather_gemm2 (transposed weights) bf16"
    # split-bf16 never reaches a weight gradient
    assert cf("wgrad", 27, 64, 64, "bf16x3", n_out=5000).rounded == frozenset()
    assert cf("fwd", 27, 64, 64, "bf16x3").split


# ------------------------------------------------------------------------------------------------ three-product restatement
def _operands(n=1 << 18, seed=3):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * torch.exp(torch.randn(n, generator=g)), torch.randn(n, generator=g)


def test_bf16_products_are_exact_in_fp32():
    """hi*hi, hi*lo, lo*hi of bf16 planes carry at most 16 significant bits: fp32 holds them exactly, so the float64 sum of the
    three products is exactly what the bf16 MFMAs multiply, and only the fp32 accumulation separates the kernel from it."""
    a, b = _operands()
    ah, al = LW.bf16_split(a)
    bh, bl = LW.bf16_split(b)
    for p, q in ((ah, bh), (ah, bl), (al, bh)):
        assert torch.equal((p * q).double(), p.double() * q.double())
    # the planes are bf16 values, and lo is the fp32 residual rounded to nearest even
    for v, h, lo in ((a, ah, al), (b, bh, bl)):
        assert torch.equal(h, LW.bf16_rne(v)) and torch.equal(lo, LW.bf16_rne(v - h))


def test_three_products_land_within_2_pow_16_of_the_exact_product():
    """|hi*hi + hi*lo + lo*hi - a*b| <= 2^-16 |a*b| + |lo*lo| (the two residuals a - hi - lo are <= 2^-17 |a| each), RMS within
    2^-16; the lo*lo product left out is itself <= 2^-16 of the product -- ~2^-18 RMS, 2.7e-6 of a reduction's L2 norm: about the
    fp32-accumulation bound of the GPU matrix, which therefore does not rely on it (its exact-fp32 reference is a control only
    where it sits SEP bounds away)."""
    a, b = _operands()
    ah, al = LW.bf16_split(a)
    bh, bl = LW.bf16_split(b)
    A, B = a.double(), b.double()
    ex = A * B
    three = ah.double() * bh.double() + ah.double() * bl.double() + al.double() * bh.double()
    lolo = (al.double() * bl.double()).abs()
    assert float(((A - ah.double() - al.double()).abs() / A.abs()).max()) <= 2.0 ** -17
    assert bool(((three - ex).abs() <= 2.0 ** -16 * ex.abs() + lolo).all())
    assert float(((three - ex) / ex).pow(2).mean().sqrt()) <= 2.0 ** -16
    assert float((lolo / ex.abs()).max()) <= 2.0 ** -16
    # the controls are far outside: one plane 2^-9, a dropped hi*lo product 2^-10 (RMS)
    one = ah.double() * bh.double()
    drop = one + al.double() * bh.double()
    assert float(((one - ex) / ex).pow(2).mean().sqrt()) > 2.0 ** -10
    assert float(((drop - ex) / ex).pow(2).mean().sqrt()) > 2.0 ** -11


def _emulated(x, w, nbr, kind):
    """A "kernel" that sums the products of `kind` per offset with fp32 matrix products (another association than the bound's)."""
    out = torch.zeros(nbr.shape[0], w.shape[2])
    for k in range(nbr.shape[1]):
        sel = nbr[:, k] >= 0
        for p, q in RM._pairs(x, w, kind):
            out[sel] += p[nbr[sel, k].long()] @ q[k]
    return out


@pytest.mark.parametrize("n_out,K,cin,cout", [(700, 27, 64, 64), (300, 8, 96, 64), (500, 1, 64, 128)])
@pytest.mark.parametrize("math", ["bf16", "bf16x3"])
def test_matrix_bound_rejects_subtly_wrong_kernels(n_out, K, cin, cout, math):
    """The GPU matrix's judge (bound from fp32 accumulation alone) on emulated kernels: the declared products pass, and every
    negative control fails -- exact fp32 operands; bf16 truncation instead of RNE; for bf16x3 the one-plane form, a dropped hi*lo
    product and a truncated lo plane."""
    g = torch.Generator().manual_seed(n_out + K)
    nbr = RM._table(n_out, K, n_out + 17, g)
    x = torch.randn(n_out + 17, cin, generator=g)
    w = torch.randn(K, cin, cout, generator=g) * 0.1

    def ref_fn(kind):
        return sum(RM._gather64(p.double(), q.double(), nbr) for p, q in RM._pairs(x, w, kind))

    def seq_fn(kind):
        return RM._gather_seq32(RM._pairs(x, w, kind), nbr)

    declared = math
    for kernel in [declared] + RM._controls(declared, math) + (["fp32"] if math == "bf16x3" else []):
        J = RM.Judge()
        J.judge("emulated", kernel, _emulated(x, w, nbr, kernel), ref_fn, seq_fn, declared, math)
        if kernel == declared:
            assert not J.fails, J.lines
        else:
            assert J.fails, (kernel, J.lines)
