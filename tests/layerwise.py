"""Teacher-forced, operator-by-operator float64 references of the Mink-ResNet trunk and of Res16UNet, and the comparators that
judge a kernel's output against them (tests/test_gpu_layerwise.py and tests/test_gpu_seg_layerwise.py on the GPU,
tests/test_layerwise_cpu.py and tests/test_seg_layerwise_cpu.py for the negative controls).

Every reference is plain torch float64 on whatever device its inputs are on, fed with the operands the kernel itself read
(the HIP run's own stored activations, gradients, statistics and ReLU decisions): no error carries over from one layer to
the next, so each operator is held to what its own kernel test holds it to.

Tables are the trunk's: nbr[n_out, K] = input row of output row o at offset k, or -1 (oracle/maps.py kernel_map_table);
weights are [K, cin, cout]."""
import ctypes
from dataclasses import dataclass

import torch

# ---------------------------------------------------------------------------------------------------------- bounds
CONV_REL = 2e-5  # relative L2 per tensor (tests/test_gpu_ops.py)
CONV_MAX = 1e-4  # max |err| / max |ref|: one bad row or element cannot hide in the norm
NORM_BOUND = 1e-5  # batch-norm quantities, relative to their scale (fp32 rounding only)
FLIP_Z = 1e-4  # a ReLU branch may differ from float64's own only where |z| <= FLIP_Z * sd(z)
STORE_MAX = 2e-5  # bf16-stored values: half a bf16 ulp of the float64 value + STORE_MAX * max |ref|
# "declared vs other" is asserted where the two rounding references sit more than DISCRIMINATE bounds apart.  Rounding one
# operand to bf16 moves a product by 2^-9 / sqrt(3) = 1.1e-3 relative (RMS): 100 bounds (2e-3) would sit above that separation
# and skip the check almost everywhere; 20 (4e-4) still leaves a kernel within the bound of one reference 19 bounds from the other.
DISCRIMINATE = 20.0


# ------------------------------------------------------------------------------------------------ rounding table
def bf16_rne(t):
    """Round to bf16, nearest even (`(__bf16)v` and the MFMA packers of csrc/conv_common.h / stem16.hip), back in t's dtype."""
    return t.float().to(torch.bfloat16).to(t.dtype)


def bf16_trunc(t):
    """Round to bf16 by truncation -- NOT what any kernel may do (negative control)."""
    return (t.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(t.dtype)


# csrc/ constants the dispatch below depends on
BK, BN = 32, 64  # conv_common.h BK / BN: reduction chunk, output columns per workgroup of the gather-GEMMs
WT, WROWS = 64, 128  # conv_wgrad.hip WT / WROWS: weight-gradient super-tile, rows per tile
CONV_MATH = {"fp32": 0, "bf16": 1, "bf16s": 1, "bf16x3": 3}  # "bf16s": bf16 math + bf16 storage of the stem (functional.set_conv_storage)


def _cdiv(a, b):
    return -(-a // b)


def wgrad_plan(n_out, K, cin, cout, force=0):
    """(G, nsplit) of wgrad_plan (conv_wgrad.hip): offsets per workgroup and row splits.  `force`: set_stagger bits 12-26
    (g_conv.wgrad_force: bits 0-3 of it the G code 1 / 2 / 3 -> G = 1 / 3 / 9, bits 4.. a forced row-split count)."""
    tiles = _cdiv(cin, WT) * _cdiv(cout, WT)
    row_tiles = _cdiv(n_out, WROWS)
    G = 1
    if K >= 9 and tiles * _cdiv(K, 9) * row_tiles >= 1024:
        G = 9
    elif K >= 3 and tiles * _cdiv(K, 3) * row_tiles >= 1024:
        G = 3
    tiny = row_tiles <= 4 and tiles * K >= 512
    if tiny:
        G = 1
    if force & 0xF:
        G = {1: 1, 2: 3}.get(force & 0xF, 9)
    z = _cdiv(512, tiles * _cdiv(K, G))
    if tiny:
        z = 1
    if force >> 4:
        z = force >> 4
    z = max(1, min(z, row_tiles))
    streamed = G == 9 and K == 27 and cin <= 32 and tiles == 1 and z >= 16
    if streamed:
        z = z // 8 * 8
    rows = _cdiv(_cdiv(n_out, z), WROWS) * WROWS
    nsplit = max(1, _cdiv(n_out, rows))
    if streamed:
        nsplit = _cdiv(nsplit, 8) * 8
    return G, nsplit


@dataclass(frozen=True)
class ConvForm:
    """What one convolution launch computes: the kernel it reaches, the operands it rounds to bf16 before its fp32-accumulating
    products, and whether the rounding is the split-bf16 one (v = hi + lo, products hi*hi + hi*lo + lo*hi: form_reference)."""
    form: str
    rounded: frozenset
    split: bool = False


def conv_form(op, K, cin, cout, math, n_out=1, ldx=None, ldy=None, row_perm=False, aligned=True, ksplit=1, force_g=0, perm16=True,
              shortcut_dense=True, flip=False, acc=False):
    """The launch form and operand rounding of one convolution operator, restated from the planners plan_gather
    (csrc/conv.hip) and wgrad_plan (csrc/conv_wgrad.hip) with the default switches and within their 32-bit
    size limits; tests/test_conv_dispatch_cpu.py holds the restatement to the library's own answer.

    op: "fwd" (W as [K][cin][cout]), "dgrad" (the same-map or class-permuted gather with the forward weights read transposed),
    "wgrad" (dW[k] = X[nbr[:, k]]^T dY) or "store" (the stem's y under "bf16s").  cin / cout are the CONVOLUTION's; ldx is the
    row stride of the gathered operand (x, or dY for "dgrad"; default: contiguous), ldy that of dY for "wgrad".  row_perm: the
    launch goes through a class permutation (a strided data gradient, or the forward of a transposed convolution).  aligned:
    the operand pointers are 16-byte aligned (torch allocations are).  ksplit: the split the launch is asked for.  force_g:
    set_stagger bits 12-26 (wgrad_plan's hook).  flip / acc: flip_k bits 0 / 1 of a gather launch (weights of offset K-1-k;
    y += result) -- a flipped launch never takes the flat stem path, an accumulating one never the class-permuted compact
    kernel.  perm16: set_stagger bit 27 clear (the class-permuted bf16 data gradient on compact_gemm_kernel).  shortcut_dense:
    a K = 1 class-permuted data gradient is the exact-fp32 dense GEMM mink_dense_xwt + a scatter (functional.py
    ConvolutionFunction.backward, trunk.hip), not a gather."""
    m = CONV_MATH[math]
    if op == "store":
        return ConvForm("bf16 store" if math == "bf16s" else "fp32 store", frozenset({"y"}) if math == "bf16s" else frozenset())
    if op == "wgrad":
        ldx = cin if ldx is None else ldx
        ldy = cout if ldy is None else ldy
        G, nsplit = wgrad_plan(n_out, K, cin, cout, force_g)
        tag = f" G{G}" + (" split" if nsplit > 1 else "")
        # the streaming kernels take the stem shape (stream_ok of wgrad_plan in conv_wgrad.hip)
        stream_ok = K == 27 and cin <= 32 and ldx < 64
        if G == 9 and stream_ok:
            if m == 1:  # wgrad_plan in conv_wgrad.hip: bf16_stream
                return ConvForm("wgrad_stream_bf16" + tag, frozenset({"x", "dy"}))
            return ConvForm("wgrad_stream" + tag, frozenset())
        if m == 1 and G != 9 and cin % WT == 0 and cout % WT == 0 and aligned and (ldx | ldy) % 4 == 0:  # wgrad_plan in conv_wgrad.hip: the wgrad16_kernel branch
            return ConvForm(f"wgrad16<{3 if G == 3 else 1}>" + tag, frozenset({"x", "dy"}))
        return ConvForm("wgrad fp32" + tag, frozenset())  # launch_wgrad<G>: exact fp32 under every math (bf16x3 included)
    assert op in ("fwd", "dgrad"), op
    wt = op == "dgrad"
    if wt and row_perm and K == 1 and cin % 4 == 0 and cout % 4 == 0 and shortcut_dense:
        return ConvForm("dense_xwt", frozenset())
    gin, gout = (cout, cin) if wt else (cin, cout)  # the GEMM's reduction / output widths
    names = {"dy", "w"} if wt else {"x", "w"}
    ldx = gin if ldx is None else ldx
    vec = aligned and ldx % 4 == 0 and gin % 4 == 0 and (wt or gout % 4 == 0)  # plan_gather in conv.hip: al, vec
    if m == 0:
        return ConvForm("fp32", frozenset())
    # the class-permuted branch (compact_perm_shape in conv.hip and its use in plan_gather): bf16 math takes it for the data gradient only
    if (row_perm and wt and m == 1 and perm16 and K >= 8 and gin >= 64 and gin % BK == 0 and gout % BN == 0 and vec
            and gout % 4 == 0 and not acc):
        return ConvForm("class-permuted compact bf16", frozenset(names))
    if not vec:  # gather_gemm_kernel (plan_gather in conv.hip, its last branch): operands that are not 16-byte rows -- no MATH parameter, exact fp32
        return ConvForm("scalar gather_gemm", frozenset())
    # gather_gemm2_kernel<W_T, STAGE, FLAT, MATH> (plan_gather in conv.hip: flat; the row-compacted forms need fp32 math: compact_ok)
    if row_perm:
        form = "staged gather_gemm2" + (" (transposed weights)" if wt else " (transposed-conv fwd)")
    elif wt:
        form = "dense gather_gemm2 (transposed weights)"
    elif gin == 28 and ldx <= 32 and not flip and _cdiv(K, _cdiv(K, ksplit)) == 1:
        form = "flat gather_gemm2 (cin 28)"  # FLAT = 28: un-split forward launches only
    else:
        form = "dense gather_gemm2"
    if gin % BK and "flat" not in form:
        form += " + channel tail"
    return ConvForm(form + (" bf16x3" if m == 3 else " bf16"), frozenset(names), split=m == 3)


CKP = 9  # conv_common.h: offsets per workgroup of the row-compacted kernel


def gather_launch_form(n_out, K, cin, cout, ldx, ldy, wt, flip, perm, acc, ksplit, math="fp32", pipe=0):
    """(launch form, slabs written) of one mink_conv_gather_gemm call -- plan_gather (csrc/conv.hip) for 16-byte aligned
    operands and default set_stagger switches, fp32 math included (conv_form names the fp32 launches just "fp32": its callers ask
    which operands are rounded, this one which kernel runs and how many slabs it writes).  cin / cout are the GEMM's reduction /
    output widths (the ABI's arguments), wt / flip / perm / acc its w_transposed, flip_k bit 0, row_perm and flip_k bit 1, ksplit
    the split asked for, pipe mink_conv_set_pipeline's mode.  The dense, flat, staged and scalar forms under reduced math are
    conv_form's."""
    math = CONV_MATH[math]
    vec = ldx % 4 == 0 and cin % 4 == 0 and (wt or cout % 4 == 0)
    mid = K >= 8 and cin >= 64 and cin % BK == 0 and cout % BN == 0 and vec and ldy % 4 == 0 and not acc
    if perm and mid and (math == 0 or (math == 1 and wt)):
        ncc = cin // BK
        zc = _cdiv(ncc, _cdiv(ncc, ksplit))
        return "class-permuted compact" + (" bf16" if math == 1 else "") + (" three-stage" if wt and pipe & 2 else ""), zc
    compact_ok = math == 0 and mid and not perm
    kper = _cdiv(K, ksplit)
    sk = False
    if pipe & 8 and ksplit > 1 and compact_ok:  # sk_plan: 1,024 workers, runs of at least five offset-tiles
        run = _cdiv(n_out, 64) * _cdiv(cout, BN) * K // 1024
        sk = run >= 5 and _cdiv(K, run) + 1 <= ksplit
    zs = ksplit if sk else _cdiv(K, kper)
    if compact_ok and (kper <= CKP or sk):
        return ("stream-K" if sk else "row-compacted" + (" three-stage" if pipe & 1 else "")), zs
    if math:
        conv_cin, conv_cout = (cout, cin) if wt else (cin, cout)
        cf = conv_form("dgrad" if wt else "fwd", K, conv_cin, conv_cout, {0: "fp32", 1: "bf16", 3: "bf16x3"}[math], n_out=n_out, ldx=ldx, row_perm=perm,
                          ksplit=ksplit, shortcut_dense=False, flip=flip, acc=acc)
        return cf.form, zs
    if not vec:
        return "scalar gather_gemm", zs
    if perm:
        return "staged gather_gemm2" + (" (transposed weights)" if wt else "") + (" accumulate" if acc else ""), zs
    if cin == 28 and zs == 1 and not flip and not wt and ldx <= 32:
        return "flat gather_gemm2 (cin 28)", zs
    return "dense gather_gemm2" + (" (transposed weights)" if wt else ""), zs


def _launch_info_consts():
    from nerf_downstream_amd import _lib

    return _lib.constants("MINK_KERNEL_")


def ask_gather_launch(L, n_in, ldx, cin, wt, flip, n_out, K, perm, n_virtual, ldy, cout, ksplit, acc=False, bias=False, stats=False,
                      slabs=False, xw_aligned=True, y_aligned=True):
    """The library's own answer for one mink_conv_gather_gemm / _stats / _slabs call under the switches now set
    (mink_conv_gather_gemm_launch_info: the planner the launch runs) -> (return code, ConvLaunchInfo)."""
    from nerf_downstream_amd import _lib

    info = _lib.ConvLaunchInfo()
    rc = L.mink_conv_gather_gemm_launch_info(n_in, ldx, cin, int(wt), int(flip) | (2 if acc else 0), n_out, K, int(perm), n_virtual, ldy, cout,
                                             int(bias), ksplit, int(stats), int(slabs), int(xw_aligned), int(y_aligned), ctypes.byref(info))
    return rc, info


def ask_wgrad_launch(L, n_in, ldx, cin, ldy, cout, n_out, K, fuse=0, n_pool=0, aligned=True):
    """The same for mink_conv_wgrad (fuse 0), mink_conv_wgrad_bn_relu_pool (1) and _b16 (2)."""
    from nerf_downstream_amd import _lib

    info = _lib.ConvLaunchInfo()
    rc = L.mink_conv_wgrad_launch_info(n_in, ldx, cin, ldy, cout, n_out, K, fuse, n_pool, int(aligned), ctypes.byref(info))
    return rc, info


def launch_form_name(info, cin, acc=False):
    """A gather-GEMM launch the library names (ConvLaunchInfo) in gather_launch_form's words.  cin (the GEMM's reduction width)
    and acc are the call's: conv_form tags a channel tail under reduced math, gather_launch_form an accumulating staged launch.
    The instantiation that carries the timing switches, which the restatement does not cover, reads "... ablation"."""
    kind = _launch_info_consts()
    t = list(info.targ)
    if info.kernel == kind["COMPACT"]:
        _, perm, abl, math, p3, sk = t
        if sk:
            return "stream-K"
        return (("class-permuted compact" if perm else "row-compacted") + (" bf16" if math == 1 else "") + (" three-stage" if p3 else "")
                + (" ablation" if abl else ""))
    if info.kernel == kind["GATHER_SCALAR"]:
        return "scalar gather_gemm"
    assert info.kernel == kind["GATHER2"], info.kernel
    wt, stage, flat, math = t[:4]
    if stage:
        form = "staged gather_gemm2" + (" (transposed weights)" if wt else " (transposed-conv fwd)" if math else "")
    elif wt:
        form = "dense gather_gemm2 (transposed weights)"
    else:
        form = "flat gather_gemm2 (cin 28)" if flat else "dense gather_gemm2"
    if math:
        return form + (" + channel tail" if cin % BK and not flat else "") + (" bf16x3" if math == 3 else " bf16")
    return form + (" accumulate" if stage and acc else "")


def wgrad_form_name(info, instantiation=False):
    """A weight-gradient launch the library names in conv_form("wgrad")'s words ("wgrad16<3> G3 split"), or, `instantiation`,
    the streaming kernels by their template arguments ("wgrad_stream<FUSE, FLAT>": the fused stem cases)."""
    kind = _launch_info_consts()
    t = list(info.targ)
    tag = " split" if info.slabs > 1 else ""
    if info.kernel == kind["WGRAD"]:
        return f"wgrad fp32 G{t[0]}" + tag
    if info.kernel == kind["WGRAD16"]:
        return f"wgrad16<{t[0]}> G{t[0]}" + tag
    args = {kind["WGRAD_STREAM"]: [n for n, on in (("FUSE", t[1]), ("FLAT", t[2])) if on],
            kind["WGRAD_STREAM_BF16"]: [n for n, on in (("FUSE", t[0]), ("B16", t[1])) if on], kind["WGRAD_STREAM_B16T"]: []}[info.kernel]
    name = {kind["WGRAD_STREAM"]: "wgrad_stream", kind["WGRAD_STREAM_BF16"]: "wgrad_stream_bf16", kind["WGRAD_STREAM_B16T"]: "wgrad_stream_b16t"}[info.kernel]
    if instantiation:
        return name + (f"<{', '.join(args)}>" if args else "")
    return name + " G9" + tag  # (the streaming kernels take nine offsets per workgroup: wgrad_plan's `streaming`)


def rounded_operands(op, K, cin, cout, math, **shape):
    """The operands a kernel rounds to bf16 before its fp32-accumulating products (conv_form: shape-aware -- a scalar-form
    gather and a weight gradient whose widths are not multiples of 64 stay exact fp32 under bf16 math, the K = 1 strided
    data gradient is the exact-fp32 dense GEMM mink_dense_xwt, and bf16x3 math splits instead of rounding: conv_form.split).
    "bf16s" also STORES the stem's convolution output as bf16 (op "store": the y it keeps)."""
    return conv_form(op, K, cin, cout, math, **shape).rounded


def form_reference(fn, ops, cf, rnd=bf16_rne):
    """float64 fn(**ops) on the operands as the form `cf` (conv_form) multiplies them: rounded where it rounds, and for split-bf16
    the three products hi*hi + hi*lo + lo*hi of its two operands.  fn must be bilinear in them up to a constant term (a residual
    added to a data gradient): that term is fn at zero operands, counted once."""
    if not cf.split:
        return fn(**apply_rounding(ops, cf.rounded, rnd))
    (p, a), (q, b) = ops.items()
    ah, al = (t.double() for t in bf16_split(a))
    bh, bl = (t.double() for t in bf16_split(b))
    c = fn(**{p: torch.zeros_like(ah), q: torch.zeros_like(bh)})
    return fn(**{p: ah, q: bh}) + fn(**{p: ah, q: bl}) + fn(**{p: al, q: bh}) - 2 * c


def other_reference(fn, ops, cf):
    """The other rounding of check_conv: the fp32 operands where the form rounds or splits, every operand rounded to bf16 where
    it multiplies them exactly."""
    return fn(**apply_rounding(ops, frozenset() if cf.rounded else frozenset(ops)))


def bf16_split(t, rnd=None):
    """(hi, lo) of split-bf16 (conv_common.h pack_bf16 / conv.hip bf16_residual): hi = rne(v), lo = rne(v - hi), both taken in fp32."""
    rnd = rnd or bf16_rne
    v = t.float()
    hi = bf16_rne(v)
    return hi, rnd(v - hi)


def apply_rounding(ops, rounded, rnd=bf16_rne):
    """{name: tensor} -> the same, float64, with the names in `rounded` passed through `rnd` first (on their fp32 values)."""
    return {k: (rnd(v.float()) if k in rounded else v).double() for k, v in ops.items()}


# ------------------------------------------------------------------------------------------------ reference operators
def check_table(nbr, n_in):
    """Every entry of a table is -1 or a row of its n_in-row source: the references index with it on the device, where an
    out-of-range index is a memory fault, not an exception."""
    lo, hi = int(nbr.min()), int(nbr.max())
    assert lo >= -1 and hi < n_in, f"table entries in [{lo}, {hi}], source has {n_in} rows"


def _valid(nbr, k):
    o = torch.nonzero(nbr[:, k] >= 0).squeeze(1)
    return o, nbr[o, k].long()


def scatter_rows(src, rows, n):
    """out[rows[o]] += src[o] for rows[o] >= 0 (mink_rows_scatter_add: a 1x1x1 strided table's -1 entries are skipped)."""
    check_table(rows[:, None], n)
    o = torch.nonzero(rows >= 0).squeeze(1)
    return torch.zeros(n, src.shape[1], dtype=torch.float64, device=src.device).index_add_(0, rows[o].long(), src[o].double())


def conv_fwd(x, w, nbr):
    """y[o] = sum_k x[nbr[o, k]] @ w[k]."""
    check_table(nbr, x.shape[0])
    y = torch.zeros(nbr.shape[0], w.shape[2], dtype=torch.float64, device=x.device)
    for k in range(nbr.shape[1]):
        o, i = _valid(nbr, k)
        if o.numel():
            y.index_add_(0, o, x[i].double() @ w[k].double())
    return y


def conv_dgrad(gy, w, nbr, n_in):
    """dX of conv_fwd: gx[nbr[o, k]] += gy[o] @ w[k]^T (scattered through the FORWARD table: independent of the tables the
    kernels gather through)."""
    check_table(nbr, n_in)
    assert gy.shape[0] == nbr.shape[0]
    gx = torch.zeros(n_in, w.shape[1], dtype=torch.float64, device=gy.device)
    for k in range(nbr.shape[1]):
        o, i = _valid(nbr, k)
        if o.numel():
            gx.index_add_(0, i, gy[o].double() @ w[k].double().t())
    return gx


def conv_dgrad_gather(gy, w, table, flip_k=False, perm=None):
    """dX in the form the kernels compute it, one row per table row: gx[i] = sum_k gy[table[i, k]] @ w[k']^T with
    k' = K-1-k (`flip_k`: a centred odd stride-1 kernel through its own forward table) or k' = k (the transposed table of a
    strided convolution).  `perm` (the class partition of the strided data gradient, -1 padded) must visit every row once."""
    K = table.shape[1]
    check_table(table, gy.shape[0])
    if perm is not None:
        p = perm[perm >= 0].long()
        assert p.numel() == table.shape[0] and torch.equal(torch.sort(p).values, torch.arange(table.shape[0], device=p.device)), \
            "class permutation does not visit every row exactly once"
    gx = torch.zeros(table.shape[0], w.shape[1], dtype=torch.float64, device=gy.device)
    for k in range(K):
        r, o = _valid(table, k)
        if r.numel():
            gx.index_add_(0, r, gy[o].double() @ w[K - 1 - k if flip_k else k].double().t())
    return gx


def conv_wgrad(x, gy, nbr):
    """dW[k] = x[nbr[:, k]]^T @ gy over the valid pairs."""
    check_table(nbr, x.shape[0])
    assert gy.shape[0] == nbr.shape[0]
    K = nbr.shape[1]
    gw = torch.zeros(K, x.shape[1], gy.shape[1], dtype=torch.float64, device=x.device)
    for k in range(K):
        o, i = _valid(nbr, k)
        if o.numel():
            gw[k] = x[i].double().t() @ gy[o].double()
    return gw


def bn_stats(y, eps=1e-5):
    """Training-mode batch statistics: mean and 1 / sqrt(biased variance + eps), float64."""
    y = y.double()
    mean = y.mean(0)
    return mean, (((y - mean) ** 2).mean(0) + eps).rsqrt()


def _bn(y, gamma, beta, eps):
    mean, invstd = bn_stats(y, eps)
    return (y - mean) * invstd * gamma + beta


def bn_fwd(y, gamma, beta, residual=None, eps=1e-5):
    """z = gamma * (y - mean) * invstd + beta [+ residual] -- the pre-activation; the caller applies its ReLU decision."""
    z = _bn(y.double(), gamma.double(), beta.double(), eps)
    return z if residual is None else z + residual.double()


def bn_bwd(g, y, gamma, beta, mask=None, eps=1e-5):
    """Backward of out = [mask *] bn(y) (+ a residual, whose gradient is the masked g): autograd in float64.
    `mask`: the KERNEL's ReLU decisions (out > 0 of the stored output), None = no ReLU.  -> (dy, d_residual, dgamma, dbeta)."""
    y64 = y.double().detach().requires_grad_(True)
    ga = gamma.double().detach().requires_grad_(True)
    be = beta.double().detach().requires_grad_(True)
    dz = g.double() if mask is None else g.double() * mask.double()
    with torch.enable_grad():
        z = _bn(y64, ga, be, eps)
        dy, dga, dbe = torch.autograd.grad(z, (y64, ga, be), dz)
    return dy, dz, dga, dbe


def sum_pool(x, in2out, n_out):
    """Sum pooling (2, 2): out[in2out[i]] += x[i]."""
    assert in2out.shape[0] == x.shape[0]
    check_table(in2out[:, None], n_out)
    assert int(in2out.min()) >= 0
    return torch.zeros(n_out, x.shape[1], dtype=torch.float64, device=x.device).index_add_(0, in2out.long(), x.double())


def stem_bwd(g_pool, y, gamma, beta, in2out, mask, eps=1e-5):
    """Backward of pool(relu(bn(y))) under the kernel's ReLU decisions `mask` [n, C]: -> (dy, dgamma, dbeta)."""
    assert in2out.shape[0] == y.shape[0] and int(in2out.min()) >= 0 and int(in2out.max()) < g_pool.shape[0]
    dy, _, dga, dbe = bn_bwd(g_pool.double()[in2out.long()], y, gamma, beta, mask, eps)
    return dy, dga, dbe


def fma32(a, b, c):
    """fp32 fma(a, b, c), exactly (the product of two floats is exact in float64)."""
    return (a.double() * b.double() + c.double()).float()


def stem_wgrad_operand(g_pool, y, mean, invstd, gamma, beta, dgamma, dbeta, in2out, n):
    """The dY operand the stem's fused weight-gradient kernel recomputes in fp32 from the kernel's own (y, mean, invstd,
    dgamma, dbeta) (csrc/conv_wgrad.hip, wgrad_stream*_kernel<FUSE>) -- what it then rounds to bf16 under bf16 math:
      xh = fma(y, invstd, fl(-mean * invstd)),  m = fma(xh, gamma, beta) > 0,
      v  = fl(gamma * invstd) * fma(-fl(dgamma / n), xh, fma(dp, m, -fl(dbeta / n)))   (1 / n and the quotients as fl(x * fl(1 / n)))."""
    assert in2out.shape[0] == y.shape[0] and int(in2out.min()) >= 0 and int(in2out.max()) < g_pool.shape[0]
    f = torch.float32
    y, mean, invstd, gamma, beta, dgamma, dbeta = (t.to(f) for t in (y, mean, invstd, gamma, beta, dgamma, dbeta))
    inv_n = torch.tensor(1.0 / n, dtype=f, device=y.device)
    xh = fma32(y, invstd, -mean * invstd)
    m = (fma32(xh, gamma, beta) > 0).to(f)
    dp = g_pool.to(f)[in2out.long()]
    inner = fma32(dp, m, -(dbeta * inv_n))
    return (gamma * invstd) * fma32(-(dgamma * inv_n), xh, inner)


# ------------------------------------------------------------------------------------------------ segmentation (Res16UNet)
# The transposed convolution is stated through the fine -> coarse table of the ordinary convolution it inverts:
# nbr[n_coarse, K] = fine row of coarse row o at offset k (oracle/maps.py kernel_map_table(fine, coarse, offsets(2, ts))).
def tconv_fwd(x, w, nbr, n_fine):
    """y[nbr[o, k]] += x[o] @ w[k]: coarse rows x [n_coarse, cin] up-sampled onto the n_fine rows (scattered through nbr)."""
    check_table(nbr, n_fine)
    assert x.shape[0] == nbr.shape[0]
    y = torch.zeros(n_fine, w.shape[2], dtype=torch.float64, device=x.device)
    for k in range(nbr.shape[1]):
        o, i = _valid(nbr, k)
        if o.numel():
            y.index_add_(0, i, x[o].double() @ w[k].double())
    return y


def tconv_dgrad(gy, w, nbr):
    """dX of tconv_fwd: gx[o] = sum_k gy[nbr[o, k]] @ w[k]^T (gathered through nbr)."""
    check_table(nbr, gy.shape[0])
    gx = torch.zeros(nbr.shape[0], w.shape[1], dtype=torch.float64, device=gy.device)
    for k in range(nbr.shape[1]):
        o, i = _valid(nbr, k)
        if o.numel():
            gx.index_add_(0, o, gy[i].double() @ w[k].double().t())
    return gx


def tconv_wgrad(x, gy, nbr):
    """dW of tconv_fwd: dW[k] = x[o]^T @ gy[nbr[o, k]] over the valid pairs."""
    check_table(nbr, gy.shape[0])
    assert x.shape[0] == nbr.shape[0]
    gw = torch.zeros(nbr.shape[1], x.shape[1], gy.shape[1], dtype=torch.float64, device=x.device)
    for k in range(nbr.shape[1]):
        o, i = _valid(nbr, k)
        if o.numel():
            gw[k] = x[o].double().t() @ gy[i].double()
    return gw


def pointwise_fwd(x, w, bias=None):
    """1x1x1 stride-1 convolution (kernel [cin, cout]) [+ bias [1, cout]]."""
    y = x.double() @ w.double().reshape(x.shape[1], -1)
    return y if bias is None else y + bias.double().reshape(1, -1)


def pointwise_dgrad(gy, w):
    return gy.double() @ w.double().reshape(-1, gy.shape[1]).t()


def pointwise_wgrad(x, gy):
    return x.double().t() @ gy.double()


def bias_grad(gy):
    """d bias of y = conv(x) + bias: the column sums of dY, [1, cout]."""
    return gy.double().sum(0, keepdim=True)


def cat_fwd(*parts):
    """ME.cat: the feature columns of tensors on one coordinate map, side by side."""
    assert len({p.shape[0] for p in parts}) == 1
    return torch.cat([p.double() for p in parts], 1)


def cat_bwd(g, widths):
    """The gradient of each part of a cat: its own columns of g."""
    assert g.shape[1] == sum(widths)
    return list(g.double().split(list(widths), 1))


def sparse_mean(f, inverse, n_unique):
    """TensorField.sparse(): every voxel's feature is the mean of the field rows that fall into it (inverse[row] = voxel)."""
    check_table(inverse[:, None], n_unique)
    assert inverse.shape[0] == f.shape[0] and int(inverse.min()) >= 0
    inv = inverse.long()
    s = torch.zeros(n_unique, f.shape[1], dtype=torch.float64, device=f.device).index_add_(0, inv, f.double())
    cnt = torch.zeros(n_unique, dtype=torch.float64, device=f.device).index_add_(0, inv, torch.ones_like(inv, dtype=torch.float64))
    assert bool((cnt > 0).all()), "a voxel without field rows"
    return s / cnt[:, None]


def slice_fwd(y, inverse):
    """SparseTensor.slice(field): every field row reads its voxel's features."""
    check_table(inverse[:, None], y.shape[0])
    return y.double()[inverse.long()]


def slice_bwd(g, inverse, n_unique):
    """dY of slice_fwd: the field rows' gradients summed onto their voxels."""
    return sum_pool(g, inverse, n_unique)


def bn_eval_fwd(y, running_mean, running_var, gamma, beta, residual=None, eps=1e-5):
    """Eval-mode batch norm (running statistics) [+ residual]: the pre-activation."""
    z = (y.double() - running_mean.double()) * (running_var.double() + eps).rsqrt() * gamma.double() + beta.double()
    return z if residual is None else z + residual.double()


def cross_entropy_grad(logits, labels, ignore_index=-100):
    """d mean cross entropy / d logits over the rows whose label is not ignored, float64."""
    keep = labels != ignore_index
    p = torch.softmax(logits.double(), 1)
    p[keep, labels[keep].long()] -= 1.0
    p[~keep] = 0.0
    return p / max(int(keep.sum()), 1)


# ------------------------------------------------------------------------------------------------ comparators
@dataclass
class Record:
    layer: str
    op: str
    rows: int
    shape: tuple
    rounding: str
    err: float
    bound: float
    ok: bool
    note: str = ""

    def line(self):
        return (f"{self.layer:10s} {self.op:22s} rows {self.rows:8d}  {str(tuple(self.shape)):16s} {self.rounding:8s} "
                f"err {self.err:.2e}  bound {self.bound:.0e}  {'ok' if self.ok else 'FAIL'}" + (f"  {self.note}" if self.note else ""))


def _rnd_name(rounded):
    return "+".join(sorted(rounded)) if rounded else "fp32"


def conv_errors(got, ref):
    """(relative L2, max |err| / max |ref|)."""
    got, ref = got.double(), ref.double()
    d = got - ref
    return float(d.norm() / ref.norm().clamp_min(1e-300)), float(d.abs().max() / ref.abs().max().clamp_min(1e-300))


def check_conv(layer, op, got, ref, rounded=frozenset(), ref_other=None):
    """A convolution output, data gradient or weight gradient against float64 on the DECLARED-rounded operands: relative L2
    <= CONV_REL and max |err| <= CONV_MAX max |ref|.  `ref_other`: float64 on the other rounding (fp32 operands where the table
    rounds, rounded where it does not); where the two references are more than DISCRIMINATE bounds apart, the kernel must
    also sit OUTSIDE the bound of the other -- a kernel that silently rounds differently from the table fails here.
    -> [Record] (the second one, "declared vs other", only when it applies)."""
    if tuple(got.shape) != tuple(ref.shape):  # (e.g. a padded channel's gradient handed back with the rest)
        return [Record(layer, op, got.shape[0], tuple(got.shape), _rnd_name(rounded), float("inf"), CONV_REL, False,
                       f"shape {tuple(got.shape)}, reference {tuple(ref.shape)}")]
    rel, mx = conv_errors(got, ref)
    ok = rel <= CONV_REL and mx <= CONV_MAX
    recs = [Record(layer, op, got.shape[0], tuple(got.shape), _rnd_name(rounded), rel, CONV_REL, ok, f"max {mx:.1e}")]
    if ref_other is not None:
        sep, _ = conv_errors(ref_other, ref)
        if sep > DISCRIMINATE * CONV_REL:
            rel_o, mx_o = conv_errors(got, ref_other)
            ok_o = ok and not (rel_o <= CONV_REL and mx_o <= CONV_MAX)
            recs.append(Record(layer, op + " vs other", got.shape[0], tuple(got.shape), "other", rel_o, CONV_REL, ok_o,
                               f"references {sep:.1e} apart; must exceed the bound"))
        else:
            recs.append(Record(layer, op + " vs other", got.shape[0], tuple(got.shape), "other", sep, CONV_REL, True,
                               "references too close to discriminate"))
    return recs


def check_scaled(layer, op, got, ref, scale, bound=NORM_BOUND, rows=None, mask=None, note=""):
    """max |got - ref| <= bound * scale (elements where `mask` is False excluded).  bound=0: bit for bit (copies)."""
    if tuple(got.shape) != tuple(ref.shape):
        return [Record(layer, op, rows if rows is not None else got.shape[0], tuple(got.shape), "fp32", float("inf"), bound, False,
                       f"shape {tuple(got.shape)}, reference {tuple(ref.shape)}")]
    d = (got.double() - ref.double()).abs()
    if mask is not None:
        d = d[mask]
    err = float(d.max() / max(float(scale), 1e-300)) if d.numel() else 0.0
    return [Record(layer, op, rows if rows is not None else got.shape[0], tuple(got.shape), "fp32", err, bound, err <= bound, note)]


def check_stats(layer, op, mean, invstd, y, eps=1e-5):
    """Batch statistics of the kernel against bn_stats of the y it normalised: mean within NORM_BOUND of the rms of y, invstd
    within NORM_BOUND relative, channel by channel."""
    m64, is64 = bn_stats(y, eps)
    rms = float((y.double() ** 2).mean(0).sqrt().max())
    return (check_scaled(layer, op + " mean", mean, m64, rms, rows=y.shape[0])
            + check_scaled(layer, op + " invstd", invstd.double() / is64, torch.ones_like(is64), 1.0, rows=y.shape[0]))


def check_relu_out(layer, op, got, z):
    """A ReLU output of the kernel against relu(z) of float64: where the kernel's branch (got > 0) differs from float64's,
    |z| <= FLIP_Z sd(z) (a legitimate decision at zero to rounding); everywhere else max |err| <= NORM_BOUND max |ref|."""
    z = z.double()
    ref = z.clamp_min(0)
    flip = (got > 0) != (z > 0)
    nf = int(flip.sum())
    zmax = float(z[flip].abs().max() / z.std()) if nf else 0.0
    recs = check_scaled(layer, op, got, ref, float(ref.abs().max()), mask=~flip, note=f"{nf} branch(es) differ")
    recs.append(Record(layer, op + " flips", got.shape[0], tuple(got.shape), "fp32", zmax, FLIP_Z, zmax <= FLIP_Z,
                       f"{nf} element(s), largest |z|/sd(z)"))
    return recs


def reduction_scale(terms):
    """Per-column sum of |terms| (the scale fp32 rounding of a column sum is proportional to), its max over columns."""
    return float(terms.double().abs().sum(0).max())


def check_bn_bwd(layer, op, got_dy, got_dga, got_dbe, g, y, gamma, beta, mask, got_dres=None, eps=1e-5):
    """Batch-norm backward (+ ReLU under the kernel's `mask`, + residual) against autograd in float64: dx within NORM_BOUND
    of max |ref|; dgamma / dbeta, column sums over all rows, within NORM_BOUND of the sum of |terms| of their worst column."""
    dy, dz, dga, dbe = bn_bwd(g, y, gamma, beta, mask, eps)
    mean, invstd = bn_stats(y, eps)
    n = y.shape[0]
    recs = check_scaled(layer, op + " dx", got_dy, dy, float(dy.abs().max()), rows=n)
    recs += check_scaled(layer, op + " dgamma", got_dga, dga, reduction_scale(dz * (y.double() - mean) * invstd), rows=n)
    recs += check_scaled(layer, op + " dbeta", got_dbe, dbe, reduction_scale(dz), rows=n)
    if got_dres is not None:
        recs += check_scaled(layer, op + " dresidual", got_dres, dz, float(dz.abs().max()), rows=n)
    return recs


def check_bf16_store(layer, op, got, ref):
    """A value the kernel STORES as bf16: within half a bf16 ulp of the float64 value, plus STORE_MAX * max |ref|."""
    ref = ref.double()
    a = ref.abs().float().clamp_min(torch.finfo(torch.float32).tiny)
    ulp = torch.ldexp(torch.ones_like(a), torch.frexp(a).exponent - 8).double()  # bf16: 8 significant bits
    slack = (got.double() - ref).abs() - 0.5 * ulp
    err = float(slack.max() / ref.abs().max())
    return [Record(layer, op, got.shape[0], tuple(got.shape), "y", max(err, 0.0), STORE_MAX, err <= STORE_MAX, "beyond half an ulp")]


def running_snapshot(model):
    """{nn.BatchNorm1d: (name, running_mean, running_var, num_batches_tracked)}, copied by clones queued on the current stream
    (no device sync: a pass that follows keeps the schedule it would have had).  A forked shortcut's norm moves its statistics
    on the branch stream, which the current stream joins before the pass ends, so the clones read every earlier pass's update
    and none of a later one's."""
    return {m: (n, m.running_mean.detach().clone(), m.running_var.detach().clone(), m.num_batches_tracked.detach().clone())
            for n, m in model.named_modules() if isinstance(m, torch.nn.BatchNorm1d)}


def running_update(r0, v0, y, momentum=0.1):
    """nn.BatchNorm1d's update of its running statistics by a batch y [n, C], float64:
    (1 - momentum) r0 + momentum mean(y), (1 - momentum) v0 + momentum var(y) n / (n - 1)  (the UNBIASED variance).
    -> (running mean, running var, batch mean, biased batch variance)."""
    y = y.double()
    n = y.shape[0]
    mean = y.mean(0)
    var = ((y - mean) ** 2).mean(0)
    return ((1 - momentum) * r0.double() + momentum * mean, (1 - momentum) * v0.double() + momentum * var * n / max(n - 1, 1),
            mean, var)


# The fp32 update fl(fl(keep r0) + fl(momentum fl(m))) rounds three times, and keep = fl(1 - 0.1f), 0.1f miss 0.9 / 0.1 by
# under half a rounding each: it sits within 4 unit roundoffs (2 ulps) of |keep r0| + |momentum m| of the exact update --
# the slack the running-statistics check allows on top of NORM_BOUND, whatever the size of r0 next to the batch's spread.
RUN_SLACK = 4 * 2.0 ** -24


def check_running(layer, before, bn, y, passes=1):
    """The running statistics a batch norm left after `passes` training passes, the last of which normalised y, against
    running_update of the values it held before that pass (`before`: an entry of running_snapshot), channel by channel:
    |err| of the mean <= NORM_BOUND sd(y), of the var <= NORM_BOUND var(y), each beyond RUN_SLACK of the update's own terms
    (the fp32 rounding of the update itself); num_batches_tracked advanced by exactly one per pass."""
    _, r0, v0, t0 = before
    mom = bn.momentum
    rm, rv, mean, var = running_update(r0, v0, y, mom)
    n = y.shape[0]
    slack_m = RUN_SLACK * ((1 - mom) * r0.double().abs() + mom * mean.abs())
    slack_v = RUN_SLACK * ((1 - mom) * v0.double().abs() + mom * var * n / max(n - 1, 1))
    em = float((((bn.running_mean.double() - rm).abs() - slack_m).clamp_min(0) / var.sqrt().clamp_min(1e-300)).max())
    ev = float((((bn.running_var.double() - rv).abs() - slack_v).clamp_min(0) / var.clamp_min(1e-300)).max())
    steps = int(bn.num_batches_tracked) - int(t0)
    return [Record(layer, "running mean", n, tuple(rm.shape), "fp32", em, NORM_BOUND, em <= NORM_BOUND, "of sd, beyond the slack"),
            Record(layer, "running var", n, tuple(rv.shape), "fp32", ev, NORM_BOUND, ev <= NORM_BOUND,
                   "unbiased; of var, beyond the slack"),
            Record(layer, "batches tracked", n, (), "int", float(abs(steps - passes)), 0.0, steps == passes,
                   f"+{steps} over {passes} pass(es)")]


def far_running_stats(model, seed=91):
    """Seed every batch norm's running statistics far from (0, 1) and from any batch's own: mean +-[0.2, 0.6], var in
    [1.5, 3]; one channel in eight with its variance near eps (5e-6 .. 5e-5) and gamma = sqrt(var + eps), so that its output
    keeps its scale while dropping eps moves it by 10-40 %; beta N(0, 0.1).  An eval-mode kernel that normalises with the
    batch's statistics, swaps mean and variance or drops eps is then an O(1) error."""
    g = torch.Generator().manual_seed(seed)
    for m in model.modules():
        if isinstance(m, torch.nn.BatchNorm1d):
            C = m.num_features
            sign = torch.where(torch.rand(C, generator=g) < 0.5, -1.0, 1.0)
            rm = sign * (0.2 + 0.4 * torch.rand(C, generator=g))
            rv = 1.5 + 1.5 * torch.rand(C, generator=g)
            tiny = torch.arange(C) % 8 == 3
            rv[tiny] = 5e-6 + 4.5e-5 * torch.rand(int(tiny.sum()), generator=g)
            gamma = torch.ones(C)
            gamma[tiny] = (rv[tiny] + m.eps).sqrt()
            with torch.no_grad():
                m.running_mean.copy_(rm), m.running_var.copy_(rv), m.weight.copy_(gamma)
                m.bias.copy_(0.1 * torch.randn(C, generator=g))
                m.num_batches_tracked.fill_(1234)


def check_running_unchanged(before, model):
    """After an eval-mode pass: every running statistic and step counter bit for bit as before."""
    recs = []
    for m, (name, r0, v0, t0) in before.items():
        same = torch.equal(m.running_mean, r0) and torch.equal(m.running_var, v0) and torch.equal(m.num_batches_tracked, t0)
        recs.append(Record(name, "running stats kept", 0, tuple(r0.shape), "eval", 0.0 if same else float("inf"), 0.0, same))
    return recs


def report(records, title="", force=False):
    """One table line per operator; printed when something failed, when `force`, or with MINK_TEST_VERBOSE."""
    import os

    bad = [r for r in records if not r.ok]
    if bad or force or os.environ.get("MINK_TEST_VERBOSE"):
        print(f"\n[{title}] teacher-forced per-operator errors vs float64 ({len(records)} checks, {len(bad)} failed)")
        for r in records:
            print("  " + r.line())
    return bad
