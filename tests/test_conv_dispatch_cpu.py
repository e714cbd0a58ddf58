"""CPU: which launch the convolution dispatchers make, asked of the library itself (mink_conv_gather_gemm_launch_info /
mink_conv_wgrad_launch_info run plan_gather of csrc/conv.hip and wgrad_plan of csrc/conv_wgrad.hip, the planners the launches
run) and compared with the restatement the GPU suites name their cases by (layerwise.gather_launch_form / conv_form /
wgrad_plan).  Host arithmetic only."""
import contextlib
import ctypes
import itertools

import pytest

import layerwise as LW

BK, BN, CKP = LW.BK, LW.BN, LW.CKP
MATH_NAME = {0: "fp32", 1: "bf16", 3: "bf16x3"}
N_OUT = (1, 63, 65, 130, 257, 300, 1100, 12101, 40000)
KS = (1, 8, 9, 27)
WIDTHS = ((27, 7), (28, 64), (32, 96), (64, 64), (96, 128), (128, 64))
KSPLITS = (1, 2, 3, 7, 9, 14, 27)
PIPES = (0, 1, 2, 3, 8)


def _lib():
    from nerf_downstream_amd import _lib

    return _lib.lib(), _lib


@contextlib.contextmanager
def _knobs(L, stagger=0, math=0, pipeline=0, trace=None):
    old_math = L.mink_conv_set_math(math)
    old_pipe = L.mink_conv_set_pipeline(pipeline)
    L.mink_conv_set_stagger(stagger)
    if trace:
        L.mink_conv_trace(*trace)  # (a dummy address: the planner only asks whether a buffer is set and how many workgroups it holds)
    try:
        yield
    finally:
        L.mink_conv_trace(None, 0)
        L.mink_conv_set_stagger(0)
        L.mink_conv_set_pipeline(old_pipe)
        L.mink_conv_set_math(old_math)


def _strides(cin, cout):
    """(ldx, ldy): contiguous, + 4, and ldx 30 for the 27-channel shape."""
    return [(cin, cout), (cin + 4, cout + 4)] + ([(30, cout)] if cin == 27 else [])


def _n_virtual(n_out):
    return (n_out // 128 + 8) * 128  # a class partition's padded length: eight classes, each padded to 128 rows


def _inst(info):
    return (info.kernel,) + tuple(info.targ)


def _legal(K, cin, cout, ldx, wt, perm, acc, ksplit):
    """What gather_gemm_impl accepts (csrc/conv.hip): a split of at most max(K, cin / 32) slices; accumulation through a row
    permutation only, on an un-split launch with 16-byte rows."""
    if ksplit > max(K, cin // BK):
        return False
    vec = ldx % 4 == 0 and cin % 4 == 0 and (wt or cout % 4 == 0)
    return not acc or (perm and vec and LW._cdiv(K, LW._cdiv(K, ksplit)) == 1)


def _gather_sweep():
    for math in (0, 1, 3):
        for pipe in PIPES:
            yield math, pipe, [
                (n_out, K, cin, cout, ldx, ldy, wt, flip, perm, acc, ks)
                for n_out in N_OUT for K in KS for cin, cout in WIDTHS for ldx, ldy in _strides(cin, cout)
                for wt, flip, perm, acc in itertools.product((False, True), repeat=4) for ks in KSPLITS
                if _legal(K, cin, cout, ldx, wt, perm, acc, ks)]


GATHER_SWEEP_CASES = 276480  # len of every list of _gather_sweep, summed: the sweep is fixed, nothing in it is skipped


def test_gather_launch_forms_match_the_restatement():
    """Every case of the sweep: the form and the slab count of the library's plan are gather_launch_form's.  Aligned operands,
    default set_stagger bits, pipeline bit 2 clear: the domain the restatement is stated for."""
    L, _ = _lib()
    compared, seen, bad = 0, set(), []
    for math, pipe, cases in _gather_sweep():
        with _knobs(L, math=math, pipeline=pipe):
            for n_out, K, cin, cout, ldx, ldy, wt, flip, perm, acc, ks in cases:
                rc, info = LW.ask_gather_launch(L, n_out + 17, ldx, cin, wt, flip, n_out, K, perm, _n_virtual(n_out) if perm else 0, ldy, cout, ks,
                                                acc=acc)
                want = LW.gather_launch_form(n_out, K, cin, cout, ldx, ldy, wt, flip, perm, acc, ks, MATH_NAME[math], pipe)
                got = (LW.launch_form_name(info, cin, acc), info.slabs) if rc == 0 else ("refused", rc)
                compared += 1
                seen.add(_inst(info))
                if got != want and len(bad) < 20:
                    bad.append((dict(n_out=n_out, K=K, cin=cin, cout=cout, ldx=ldx, ldy=ldy, wt=wt, flip=flip, perm=perm, acc=acc, ksplit=ks,
                                     math=math, pipe=pipe), got, want))
    assert not bad, bad
    assert compared == GATHER_SWEEP_CASES, compared
    test_gather_launch_forms_match_the_restatement.seen = seen


WGRAD_FORCES = (0, 1 | (1 << 4), 2 | (1 << 4), 2 | (4 << 4), 3 | (1 << 4), 3 | (2 << 4), 3 | (17 << 4))
WGRAD_SWEEP_CASES = len(N_OUT + (43648, 43649)) * len(KS) * sum(len(_strides(*w)) for w in WIDTHS) * 2 * len(WGRAD_FORCES)


def test_weight_gradient_forms_match_the_restatement():
    """conv_form("wgrad") and wgrad_plan against the library over the same shapes, plus the stem's threshold row counts and the
    forced plans the GPU suites use: kernel, offsets per workgroup, row splits, workspace size."""
    L, lib = _lib()
    compared, seen = 0, set()
    streaming = (lib.constants("MINK_KERNEL_")["WGRAD_STREAM"], lib.constants("MINK_KERNEL_")["WGRAD_STREAM_BF16"])
    for math in (0, 1):
        for force in WGRAD_FORCES:
            with _knobs(L, stagger=force << 12, math=math):
                for n_out in N_OUT + (43648, 43649):
                    for K in KS:
                        for cin, cout in WIDTHS:
                            for ldx, ldy in _strides(cin, cout):
                                rc, info = LW.ask_wgrad_launch(L, n_out + 17, ldx, cin, ldy, cout, n_out, K)
                                assert rc == 0
                                cf = LW.conv_form("wgrad", K, cin, cout, MATH_NAME[math], n_out=n_out, ldx=ldx, ldy=ldy, force_g=force)
                                G, nsplit = LW.wgrad_plan(n_out, K, cin, cout, force)
                                where = (n_out, K, cin, cout, ldx, ldy, math, hex(force))
                                assert (LW.wgrad_form_name(info), info.slabs) == (cf.form, nsplit), where
                                assert L.mink_conv_wgrad_workspace_bytes(n_out, K, cin, cout) == (4 * nsplit * K * cin * cout if nsplit > 1 else 0), where
                                _, fused = LW.ask_wgrad_launch(L, n_out + 17, ldx, cin, cout, cout, n_out, K)  # (a fused call's dy is y: ldy = cout)
                                assert L.mink_conv_wgrad_bn_relu_pool_supported(n_out + 17, ldx, cin, n_out, K, cout) == int(fused.kernel in streaming), where
                                compared += 1
                                seen.add(_inst(info))
    assert compared == WGRAD_SWEEP_CASES, compared
    test_weight_gradient_forms_match_the_restatement.seen = seen


def _gather(L, n_out, K, cin, cout, ks=1, wt=False, perm=False, **kw):
    rc, info = LW.ask_gather_launch(L, n_out + 17, kw.pop("ldx", cin), cin, wt, wt, n_out, K, perm, _n_virtual(n_out) if perm else 0,
                                    kw.pop("ldy", cout), cout, ks, **kw)
    assert rc == 0, L.mink_last_error()
    return info


def test_every_instantiation_is_reached():
    """The planners can name 30 gather-GEMM and 28 weight-gradient instantiations (the ones csrc/conv.hip and conv_wgrad.hip
    compile).  The sweeps reach the production ones; the ones behind measurement switches are asked for here, switch by switch."""
    L, lib = _lib()
    kind = lib.constants("MINK_KERNEL_")
    epi = lib.constants("MINK_EPILOGUE_")
    C, G2, SC = kind["COMPACT"], kind["GATHER2"], kind["GATHER_SCALAR"]
    if not hasattr(test_gather_launch_forms_match_the_restatement, "seen"):
        test_gather_launch_forms_match_the_restatement()
    if not hasattr(test_weight_gradient_forms_match_the_restatement, "seen"):
        test_weight_gradient_forms_match_the_restatement()
    seen = set(test_gather_launch_forms_match_the_restatement.seen) | set(test_weight_gradient_forms_match_the_restatement.seen)

    def reach(info, kernel, *targ):
        assert _inst(info) == (kernel,) + targ + (0,) * (6 - len(targ)), (_inst(info), kernel, targ)
        seen.add(_inst(info))
        return info

    mid = dict(n_out=300, K=27, cin=64, cout=64, ks=3)
    two = _gather(L, **mid)
    # set_stagger bits 2-7 (the timing switches) and the trace buffer: the ABL instantiation, forward layout only; a transposed
    # launch with the bits set stays on the plain kernel, and the class-permuted data gradient has an ABL twin of its own
    for bit in range(2, 8):
        with _knobs(L, stagger=1 << bit, pipeline=1):  # (the timing switches outrank the three-stage form)
            reach(_gather(L, **mid), C, 0, 0, 1)
            reach(_gather(L, wt=True, **mid), C, 1)
            reach(_gather(L, wt=True, perm=True, **mid), C, 1, 1, 1)
    with _knobs(L, stagger=4, math=1, pipeline=2):  # ... which is fp32 under bf16 math too
        reach(_gather(L, wt=True, perm=True, **mid), C, 1, 1, 1)
    with _knobs(L, trace=(0x10000, 1 << 20)):
        reach(_gather(L, **mid), C, 0, 0, 1)
        reach(_gather(L, wt=True, **mid), C, 1)
    # pipeline bit 2: the two-stage kernel with the three-stage LDS footprint, whatever bit 0 says
    with _knobs(L, pipeline=1):
        three = reach(_gather(L, **mid), C, 0, 0, 0, 0, 1)
    for mode in (4, 5):
        with _knobs(L, pipeline=mode):
            for wt in (False, True):
                info = reach(_gather(L, wt=wt, **mid), C, int(wt))
                assert info.lds_bytes == three.lds_bytes > two.lds_bytes
    # pipeline bit 3 (stream-K) outranks both; bit 1: the class-permuted data gradients, fp32 and bf16
    with _knobs(L, pipeline=8 | 4 | 1):
        sk = reach(_gather(L, 12101, 27, 64, 64, ks=7), C, 0, 0, 0, 0, 0, 1)
        assert tuple(sk.grid) == (1024, 1, 1) and sk.slabs == 7 and sk.epilogue == epi["SPLITK_REDUCE"]
        reach(_gather(L, 12101, 27, 64, 64, ks=7, wt=True), C, 1, 0, 0, 0, 0, 1)
    with _knobs(L, pipeline=2):
        reach(_gather(L, wt=True, perm=True, **mid), C, 1, 1, 0, 0, 1)
    with _knobs(L, pipeline=2, math=1):
        reach(_gather(L, wt=True, perm=True, **mid), C, 1, 1, 0, 1, 1)
    # set_stagger bit 8: the class-permuted form takes cin = 32; bit 9: no flat stem path; bit 27: bf16 class-permuted data gradients
    # on the dense kernel; bit 30 / 31: the mid layers / the class-permuted data gradients on the dense kernel
    with _knobs(L):
        reach(_gather(L, 300, 27, 32, 64, wt=True, perm=True), G2, 1, 1)
        reach(_gather(L, 300, 27, 28, 64), G2, 0, 0, 28)
    with _knobs(L, stagger=1 << 8):
        reach(_gather(L, 300, 27, 32, 64, wt=True, perm=True), C, 1, 1)
    with _knobs(L, stagger=1 << 9):
        reach(_gather(L, 300, 27, 28, 64), G2)
    with _knobs(L, stagger=1 << 27, math=1):
        reach(_gather(L, wt=True, perm=True, **mid), G2, 1, 1, 0, 1)
    with _knobs(L, stagger=1 << 30):  # (both row-compacted forms)
        reach(_gather(L, **mid), G2)
        reach(_gather(L, wt=True, perm=True, **mid), G2, 1, 1)
    with _knobs(L, stagger=-(1 << 31)):
        reach(_gather(L, **mid), C)
        reach(_gather(L, wt=True, perm=True, **mid), G2, 1, 1)

    # ---- weight gradient: forced plans, set_stagger bits 10 / 11 / 28, the fused entries
    W, W16, WS, WS16, WT16 = kind["WGRAD"], kind["WGRAD16"], kind["WGRAD_STREAM"], kind["WGRAD_STREAM_BF16"], kind["WGRAD_STREAM_B16T"]

    def wgrad(n_out, cin, cout, ldx=None, ldy=None, n_in=None, **kw):
        rc, info = LW.ask_wgrad_launch(L, n_in or n_out + 17, ldx or cin, cin, ldy or cout, cout, n_out, 27, **kw)
        assert rc == 0, L.mink_last_error()
        return info

    for code, G in ((1, 1), (2, 3), (3, 9)):
        with _knobs(L, stagger=((code | (2 << 4)) << 12) | (1 << 10)):  # (bit 10: the narrow shape at G = 9 stays on the tiled kernel)
            for cin, narrow in ((96, 0), (20, 1)):
                buf = reach(wgrad(1000, cin, 64), W, G, narrow, 1, 1)
                assert buf.slabs == 2 and buf.epilogue == epi["SLAB_REDUCE"] and buf.grid[1] == 2
                reach(wgrad(1000, cin, 64, n_in=1 << 24), W, G, narrow, 1, 0)  # 2^24 input rows: no 32-bit buffer offsets
                reach(wgrad(1000, cin, 64, aligned=False), W, G, narrow, 0, 0)
                reach(wgrad(1000, cin, 64, ldx=cin + 1), W, G, narrow, 0, 0)
    stem = dict(n_out=43649, cin=28, cout=64, ldx=32)
    with _knobs(L):
        reach(wgrad(**stem), WS, 4, 0, 1)
        reach(wgrad(43649, 16, 64), WS, 4, 0, 0)
        reach(wgrad(fuse=1, n_pool=9000, **stem), WS, 4, 1, 1)
        reach(wgrad(43649, 16, 64, fuse=1, n_pool=9000), WS, 4, 1, 0)
        rc, _ = LW.ask_wgrad_launch(L, 43665, 32, 28, 64, 64, 43649, 27, fuse=2, n_pool=9000)  # bf16 storage needs bf16 math
        assert rc == -1 and b"needs bf16 math" in L.mink_last_error()
        rc, _ = LW.ask_wgrad_launch(L, 43665, 32, 28, 64, 64, 43648, 27, fuse=1, n_pool=9000)  # one row under the streaming threshold
        assert rc == -1 and b"not supported by the streaming kernel" in L.mink_last_error()
    with _knobs(L, stagger=1 << 10):  # bit 10: the tiled kernel for the stem
        reach(wgrad(**stem), W, 9, 1, 1, 1)
    with _knobs(L, math=1):
        reach(wgrad(**stem), WS16, 0, 0)
        reach(wgrad(fuse=1, n_pool=9000, **stem), WS16, 1, 0)
        reach(wgrad(fuse=2, n_pool=9000, **stem), WT16)
        reach(wgrad(43649, 28, 32, ldx=32, fuse=2, n_pool=9000), WS16, 1, 1)
    with _knobs(L, math=1, stagger=1 << 11):  # bit 11: bf16 storage without the LDS transposition
        reach(wgrad(fuse=2, n_pool=9000, **stem), WS16, 1, 1)
    with _knobs(L, math=1, stagger=1 << 28):  # bit 28: bf16 math keeps the fp32 weight-gradient kernels
        reach(wgrad(**stem), WS, 4, 0, 1)
        reach(wgrad(300, 64, 64), W, 1, 0, 1, 1)
    with _knobs(L, math=1, stagger=1 << 29):  # bit 29 (workgroup order of the streaming kernels) changes no plan
        reach(wgrad(**stem), WS16, 0, 0)
    for code, G in ((1, 1), (2, 3)):
        with _knobs(L, math=1, stagger=(code | (1 << 4)) << 12):
            reach(wgrad(300, 64, 128), W16, G)

    bools = (0, 1)
    gather = {(SC, wt, 0, 0, 0, 0, 0) for wt in bools}
    gather |= {(G2, wt, st, 0, m, 0, 0) for wt in bools for st in bools for m in (0, 1, 3)} | {(G2, 0, 0, 28, m, 0, 0) for m in (0, 1, 3)}
    gather |= {(C, wt, 0, 0, 0, p3, 0) for wt in bools for p3 in bools} | {(C, wt, 0, 0, 0, 0, 1) for wt in bools} | {(C, 0, 0, 1, 0, 0, 0)}
    gather |= {(C, 0, 1, 0, 0, 0, 0), (C, 1, 1, 1, 0, 0, 0)} | {(C, 1, 1, 0, m, p3, 0) for m in bools for p3 in bools}
    wg = {(W, G, nr, v, b, 0, 0) for G in (1, 3, 9) for nr in bools for v, b in ((1, 1), (1, 0), (0, 0))}
    wg |= {(W16, 1, 0, 0, 0, 0, 0), (W16, 3, 0, 0, 0, 0, 0), (WT16, 0, 0, 0, 0, 0, 0)}
    wg |= {(WS, 4, f, fl, 0, 0, 0) for f in bools for fl in bools} | {(WS16, 0, 0, 0, 0, 0, 0), (WS16, 1, 0, 0, 0, 0, 0), (WS16, 1, 1, 0, 0, 0, 0)}
    assert len(gather) == 30 and len(wg) == 28
    assert seen == gather | wg, (sorted(seen - gather - wg), sorted((gather | wg) - seen))


def test_misaligned_operands_leave_the_vector_kernels():
    """x or w off 16 bytes: the scalar kernel, whatever the shape.  y, the workspace or the bias off 16 bytes: a mid layer keeps
    its pipelined dense kernel but not the row-compacted ones (their epilogue stores 16 bytes), with or without a permutation."""
    L, lib = _lib()
    kind = lib.constants("MINK_KERNEL_")
    with _knobs(L):
        for n_out, K, cin, cout in ((300, 27, 64, 64), (257, 27, 28, 64), (130, 9, 96, 128)):
            for wt in (False, True):
                assert _gather(L, n_out, K, cin, cout, wt=wt, xw_aligned=False).kernel == kind["GATHER_SCALAR"]
        for perm in (False, True):
            for ks in (1, 2):
                assert _gather(L, 300, 27, 64, 64, ks=ks * (1 if perm else 3), wt=perm, perm=perm).kernel == kind["COMPACT"]
                info = _gather(L, 300, 27, 64, 64, ks=ks * (1 if perm else 3), wt=perm, perm=perm, y_aligned=False)
                assert info.kernel == kind["GATHER2"] and info.targ[1] == int(perm)


def test_the_planned_split_is_the_one_the_launch_takes():
    """mink_conv_plan's slab count, handed back as ksplit, keeps every mid layer on the kernel the planner planned for: the
    row-compacted kernel takes at most CKP offsets per slice unless the stream-K form takes the launch, and writes exactly the
    slabs the caller sized its workspace for.  (Plan and launch once disagreed on the stream-K gate: ADVICE.md.)"""
    L, lib = _lib()
    C, G2 = lib.constants("MINK_KERNEL_")["COMPACT"], lib.constants("MINK_KERNEL_")["GATHER2"]
    checked = 0
    for pipe in PIPES + (4, 9, 11):
        for stagger in (0, 4):
            with _knobs(L, pipeline=pipe, stagger=stagger):
                for n_out in N_OUT:
                    for K in (8, 9, 27):
                        for cin, cout in ((64, 64), (96, 128), (128, 64), (512, 512)):
                            for perm in (False, True):
                                rows = _n_virtual(n_out) if perm else n_out
                                plan = L.mink_conv_plan(rows, K, cin, cout, int(perm))
                                info = _gather(L, n_out, K, cin, cout, ks=plan, wt=perm, perm=perm)
                                where = (n_out, K, cin, cout, perm, pipe, stagger, plan)
                                if perm or plan * CKP >= K or info.targ[5]:
                                    # (a channel-chunk split that does not divide the chunk count writes fewer slabs than planned)
                                    slabs = LW._cdiv(cin // BK, LW._cdiv(cin // BK, plan)) if perm else plan
                                    assert info.kernel == C and info.targ[1] == int(perm) and info.slabs == slabs <= plan, where
                                else:  # beyond the slab budget of the row-compacted kernel: the dense kernel, un-split
                                    assert info.kernel == G2 and plan == 1 and 4 * n_out * cout * LW._cdiv(K, CKP) > 128 << 20, where
                                checked += 1
    assert checked == len(PIPES + (4, 9, 11)) * 2 * len(N_OUT) * 3 * 4 * 2


def test_slabs_with_bias_or_statistics_are_refused_before_any_launch():
    """A split launch that leaves its slabs to the caller cannot add a bias or sum statistics: refused by the plan, ahead of the
    kernel (it used to be refused after the launch).  The query refuses it with the call's words; the call itself, which cannot
    be given the combination through the public entries, still refuses an undersized workspace first (tests/test_capi.py)."""
    L, lib = _lib()
    epi = lib.constants("MINK_EPILOGUE_")
    with _knobs(L):
        for form in (dict(n_out=300, K=27, cin=64, cout=64), dict(n_out=257, K=27, cin=32, cout=96)):
            for extra in (dict(bias=True), dict(stats=True), dict(bias=True, stats=True)):
                rc, info = LW.ask_gather_launch(L, 317, form["cin"], form["cin"], False, False, form["n_out"], form["K"], False, 0, form["cout"],
                                                form["cout"], 3, slabs=True, **extra)
                assert rc == -1 and b"slabs are left to the caller only without bias and statistics" in L.mink_last_error()
                assert info.kernel == 0
                rc, info = LW.ask_gather_launch(L, 317, form["cin"], form["cin"], False, False, form["n_out"], form["K"], False, 0, form["cout"],
                                                form["cout"], 1, slabs=True, **extra)  # un-split: nothing is left to the caller
                assert rc == 0 and info.slabs == 1 and info.epilogue in (epi["NONE"], epi["COLSUM"])
            rc, info = LW.ask_gather_launch(L, 317, form["cin"], form["cin"], False, False, form["n_out"], form["K"], False, 0, form["cout"],
                                            form["cout"], 3, slabs=True)
            assert rc == 0 and info.slabs == 3 and info.epilogue == epi["SLABS"]
        P = 0x10000  # aligned, never dereferenced: every refusal below comes before the first launch
        nsl = ctypes.c_int32(-1)
        assert L.mink_conv_gather_gemm_slabs(P, 317, 64, 64, P, 0, 0, P, 300, 27, None, 0, P, 64, 64, 3, P, 4 * 3 * 300 * 64 - 1,
                                             ctypes.byref(nsl), None) == -1
        assert b"slabs" in L.mink_last_error() and nsl.value == 1
        # accumulation on a split launch: refused by the plan as well
        rc, _ = LW.ask_gather_launch(L, 317, 64, 64, True, False, 300, 27, True, _n_virtual(300), 64, 64, 3, acc=True)
        assert rc == -1 and b"accumulation needs an un-split launch" in L.mink_last_error()
        assert L.mink_conv_gather_gemm(P, 317, 64, 64, P, 1, 2, P, 300, 27, P, _n_virtual(300), P, 64, 64, None, 3, P, 4 * 3 * 300 * 64, None) == -1
        assert b"accumulation needs an un-split launch" in L.mink_last_error()


def test_statistics_and_reduce_epilogues():
    """The epilogue of a plan: direct statistics (column sums of the per-tile partials: 64-row tiles for the row-compacted
    kernel, 128 for the dense one), the split reduce with and without statistics, and what a shape the reduce cannot sum for
    (cout no multiple of 4) falls back to."""
    L, lib = _lib()
    epi = lib.constants("MINK_EPILOGUE_")
    with _knobs(L):
        assert _gather(L, 700, 8, 96, 128, stats=True).epilogue == epi["COLSUM"]
        assert _gather(L, 257, 27, 32, 96, stats=True).epilogue == epi["COLSUM"]
        assert _gather(L, 130, 27, 64, 64, ks=7, stats=True).epilogue == epi["SPLITK_REDUCE_STATS"]
        assert _gather(L, 130, 27, 64, 64, ks=7).epilogue == epi["SPLITK_REDUCE"]
        assert _gather(L, 130, 27, 27, 7, ks=3, stats=True).epilogue == epi["SPLITK_REDUCE"]
        assert _gather(L, 130, 27, 64, 64, ks=7, stats=True, wt=True).epilogue == epi["SPLITK_REDUCE"]  # statistics: forward layout only
        assert _gather(L, 130, 27, 64, 64).epilogue == epi["NONE"]
        rc, info = LW.ask_gather_launch(L, 0, 64, 64, False, False, 0, 27, False, 0, 64, 64, 1)
        assert rc == 0 and _inst(info) == (0,) * 7 and info.block == 0  # no rows: no launch
        rc, _ = LW.ask_gather_launch(L, 317, 64, 64, False, False, 300, 28, False, 0, 64, 64, 1)
        assert rc == -1 and b"kernel volume 28" in L.mink_last_error()
