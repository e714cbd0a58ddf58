"""CPU: the builders and the reference of tests/big_tables.py at toy sizes, with the "2^24", "2^31" and "2^32" thresholds passed
in as small numbers -- the builders meet their stated conditions, the gathered-rows reference equals a plain float64 convolution
(and its autograd gradients) over the whole small operand, and the comparison flags a kernel that wraps one probe row to its
2^24 alias or reads past a byte limit 2^32 bytes early."""
import numpy as np
import pytest
import torch

import big_tables as BT
import layerwise as LW
from helpers import class_perm
from test_gpu_ops import ATOL, RTOL  # the fp32 convolution bounds the GPU cases are held to: no new number here

TOY24 = 256              # stands for 2^24
TOY_LIMITS = (4096, 8192)  # stand for 2^31 and 2^32 bytes


def test_probe_rows_name_every_edge():
    n_in, ldx = 300, 8  # 32-byte rows: byte 4096 is row 128, byte 8192 row 256
    rows = BT.probe_rows(n_in, ldx, 4, t24=TOY24, limits=TOY_LIMITS, n_random=40, seed=3)
    assert rows.dtype == np.int64 and np.all(np.diff(rows) > 0) and rows[0] == 0 and rows[-1] == n_in - 1
    want = {0, 1, n_in - 2, n_in - 1, 63, 64, 127, 128, 253, 254, 255, 256}
    assert want <= set(rows.tolist())
    assert len(rows) > len(want) + 20  # ... and the random rows
    # the pair around a limit: the last row that starts below it and the first at or above it, also where the limit is no
    # multiple of the pitch (12-byte rows: byte 4096 lies inside row 341)
    assert BT.crossing_rows(12, 1000, limits=(4096,)) == [341, 342]
    assert 341 * 12 < 4096 <= 342 * 12
    assert BT.crossing_rows(32, 128, limits=TOY_LIMITS) == [127]  # rows that do not exist are left out
    # an operand that ends below 2^24 names no row at or above it
    small = BT.probe_rows(TOY24 - 2, ldx, 4, t24=TOY24, limits=TOY_LIMITS, n_random=10)
    assert small[-1] == TOY24 - 3 and TOY24 - 2 not in small
    # the real thresholds: the stem shape just under the flat path's gate
    real = set(BT.probe_rows((1 << 24) - 2, 32, 4, n_random=5).tolist())
    assert {(1 << 22) - 1, 1 << 22, (1 << 23) - 1, 1 << 23, (1 << 24) - 3} <= real and (1 << 24) - 2 not in real
    assert set(BT.crossing_rows(256, (1 << 24) + 5)) == {(1 << 23) - 1, 1 << 23, (1 << 24) - 1, 1 << 24}


@pytest.mark.parametrize("n_out,K", [(333, 27), (1001, 8), (77, 1)])
def test_probe_table_meets_its_conditions(n_out, K):
    rows = BT.probe_rows(300, 8, 4, t24=TOY24, limits=TOY_LIMITS, n_random=30, seed=n_out)
    t = BT.probe_table(n_out, K, rows, 0.3, seed=5)
    assert t.dtype == torch.int32 and tuple(t.shape) == (n_out, K)
    BT.check_probe_table(t, rows)
    for k in range(K):
        assert set(rows.tolist()) <= set(t[:, k].tolist()) and (t[:, k] == -1).any()
    assert (t[n_out // 2] == -1).all()
    if K > 1:
        assert 0.15 < float((t == -1).float().mean()) < 0.45
    assert torch.equal(t, BT.probe_table(n_out, K, rows, 0.3, seed=5))  # seeded
    # the checker is a checker: each broken promise is caught
    bad = t.clone()
    bad[bad == int(rows[-1])] = int(rows[0])
    with pytest.raises(AssertionError, match="lacks probe rows"):
        BT.check_probe_table(bad, rows)
    bad = t.clone()
    bad[:, 0] = bad[:, 0].clamp_min(0)
    with pytest.raises(AssertionError, match="no missing neighbour"):
        BT.check_probe_table(bad, rows)
    bad = t.clone()
    bad[n_out // 2, 0] = 0
    if not (bad == -1).all(dim=1).any():
        with pytest.raises(AssertionError, match="without any neighbour"):
            BT.check_probe_table(bad, rows)
    with pytest.raises(AssertionError, match="ragged"):
        BT.probe_table(384, K, rows[:20], 0.3, seed=5)
    with pytest.raises(AssertionError, match="do not fit"):
        BT.probe_table(len(rows), K, rows, 0.3, seed=5)


def test_window_table_is_empty_outside_its_windows():
    n_out, K, n_in = 1000 + 37, 27, 50
    # 16-byte table rows and 64-byte y rows against limits of 4096 / 8192 bytes: crossings at rows 256, 512 (table) and 64, 128 (y)
    wins = BT.tile_windows(n_out, (64, 16), tile=32, limits=TOY_LIMITS)
    assert wins[0] == (0, 32) and wins[-1] == (1024, n_out)
    for r in (63, 64, 127, 128, 255, 256, 511, 512):
        assert any(a <= r < b for a, b in wins), r
    assert all((b - a == 32 and a % 32 == 0) or b == n_out for a, b in wins)
    t = BT.window_table(n_out, K, n_in, wins, seed=9, device="cpu")
    inside = torch.zeros(n_out, dtype=torch.bool)
    inside[BT.window_rows(wins)] = True
    assert t.dtype == torch.int32 and (t[~inside] == -1).all()
    assert int(t.max()) < n_in and int(t.min()) == -1
    for a, b in wins:
        assert (t[a] >= 0).all() and (t[a + 1] == -1).all()
        frac = float((t[a:b] == -1).float().mean())
        assert 0.1 < frac < 0.6, (a, b, frac)
    assert torch.equal(t, BT.window_table(n_out, K, n_in, wins, seed=9, device="cpu"))


def test_fill_rows_pads_with_nan_and_rounds_on_request():
    x = BT.fill_rows(1000, 28, 32, seed=4, device="cpu", chunk=300)
    assert tuple(x.shape) == (1000, 28) and x.stride(0) == 32 and torch.isfinite(x).all()
    whole = torch.as_strided(x, (1000, 32), (32, 1))
    assert torch.isnan(whole[:, 28:]).all()
    assert 0.9 < float(x.std()) < 1.1 and abs(float(x.mean())) < 0.05
    assert torch.equal(x, BT.fill_rows(1000, 28, 32, seed=4, device="cpu", chunk=300))
    xb = BT.fill_rows(1000, 28, 28, seed=4, device="cpu", bf16=True, chunk=300)
    assert xb.is_contiguous() and torch.equal(xb, xb.bfloat16().float()) and not torch.equal(xb, x)
    assert torch.equal(xb, x.bfloat16().float())


def _toy(seed=0, n_in=300, n_out=333, K=27, cin=8, cout=12):
    g = torch.Generator().manual_seed(seed)
    rows = BT.probe_rows(n_in, cin, 4, t24=TOY24, limits=TOY_LIMITS, n_random=30, seed=seed)
    table = BT.probe_table(n_out, K, rows, 0.3, seed=seed)
    x = torch.randn(n_in, cin, generator=g)
    w = torch.randn(K, cin, cout, generator=g) * 0.1
    dy = torch.randn(n_out, cout, generator=g)
    bias = torch.randn(cout, generator=g)
    return rows, table, x, w, dy, bias


def test_reference_equals_float64_over_the_whole_operand():
    """Forward (with and without bias), both data-gradient forms and the weight gradient, from the gathered rows alone, against
    layerwise's plain float64 operators on the full operands and against autograd through a dense float64 restatement."""
    rows, table, x, w, dy, bias = _toy()
    K, cin, cout = w.shape
    named, local = BT.gathered(table)
    assert torch.equal(named, torch.from_numpy(rows))  # the table names exactly the probe rows
    assert torch.equal(torch.where(local >= 0, named[local.clamp_min(0)], torch.tensor(-1)), table.long())
    xs = x[named]
    y, dw = BT.reference(xs, local, w=w, dy=dy, bias=bias)
    assert torch.allclose(y, LW.conv_fwd(x, w, table) + bias.double(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dw, LW.conv_wgrad(x, dy, table), rtol=1e-12, atol=1e-12)
    dead = table.shape[0] // 2
    assert torch.equal(y[dead], bias.double())  # exactly: what the GPU test compares such rows with
    assert torch.equal(BT.reference(xs, local, w=w)[0][dead], torch.zeros(cout, dtype=torch.float64))
    # autograd of a dense restatement: one-hot gather matrices, nothing shared with the index arithmetic above
    xa, wa = x.double().requires_grad_(), w.double().requires_grad_()
    ya = sum(torch.nn.functional.one_hot(table[:, k].long().clamp_min(0), x.shape[0]).double().mul((table[:, k] >= 0)[:, None]) @ xa @ wa[k]
             for k in range(K))
    gx_auto, gw_auto = torch.autograd.grad(ya, (xa, wa), dy.double())
    assert torch.allclose(y - bias.double(), ya.detach(), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dw, gw_auto, rtol=1e-12, atol=1e-12)
    # the data gradients as the kernels compute them: a gather of dY rows through a table with n_in = rows of dY.  flip_k form:
    # the table of a centred stride-1 kernel read backwards; class-permuted form: the transposed table, offsets as they are
    gtab = BT.probe_table(301, K, BT.probe_rows(table.shape[0], cout, 4, t24=TOY24, limits=TOY_LIMITS, n_random=30, seed=1), 0.3, seed=2)
    gnamed, glocal = BT.gathered(gtab)
    for flip in (True, False):
        gx, _ = BT.reference(dy[gnamed], glocal, w=w, w_transposed=True, flip_k=flip)
        assert torch.allclose(gx, LW.conv_dgrad_gather(dy, w, gtab, flip_k=flip), rtol=1e-12, atol=1e-12), flip
    # ... and that gather IS the gradient of the forward when the tables belong together (scatter form, autograd)
    assert torch.allclose(LW.conv_dgrad(dy, w, table, x.shape[0]), gx_auto, rtol=1e-12, atol=1e-12)
    perm = class_perm(torch.randint(0, 8, (301,), generator=torch.Generator().manual_seed(5)))
    LW.conv_dgrad_gather(dy, w, gtab, perm=perm)  # (the permutation helper the GPU cases use visits every row once)


@pytest.mark.parametrize("fault", ["row wraps at 2^24", "-1 reads the row behind the last", "table read one limit early", "pad column read"])
def test_the_comparison_flags_wrapped_addressing(fault):
    """The negative control (as tests/test_layerwise_cpu.py proves its checker sees an off-by-one): a 'kernel' with one
    addressing fault of the kind this suite is for, on the full toy operands, against the gathered-rows reference under the
    GPU test's bounds.  The faithful kernel passes; each fault is flagged, in the forward and in the weight gradient."""
    rows, table, x, w, dy, bias = _toy(seed=7, n_in=300)
    named, local = BT.gathered(table)
    ref_y, ref_dw = BT.reference(x[named], local, w=w, dy=dy)

    def kernel(tab, xop):
        return LW.conv_fwd(xop, w, tab).float(), LW.conv_wgrad(xop, dy, tab).float()

    y, dw = kernel(table, x)
    assert BT.worst_over_bound(y, ref_y, ATOL, RTOL) <= 1.0 and BT.worst_over_bound(dw, ref_dw, ATOL, RTOL) <= 1.0
    bad, xop = table.clone(), x
    if fault == "row wraps at 2^24":  # ONE probe row, the first at or past the toy 2^24, read at its alias row & (2^24 - 1)
        assert TOY24 in rows
        bad[bad == TOY24] = TOY24 & (TOY24 - 1)
    elif fault == "-1 reads the row behind the last":  # the sentinel offset lands inside the operand: a missing neighbour of one row reads data
        o, k = (int(v) for v in torch.nonzero(table[: table.shape[0] // 2] == -1)[0])
        bad[o, k] = x.shape[0] - 1
    elif fault == "table read one limit early":  # the table row past the toy 2^31-byte limit read that many bytes early
        first = -(-TOY_LIMITS[0] // (4 * table.shape[1]))
        assert first < table.shape[0]
        bad[first] = table[0]
    else:  # a pitched operand whose pad column is read for the last channel: NaN reaches the output
        xop = x.clone()
        xop[int(rows[3]), -1] = float("nan")
    y, dw = kernel(bad, xop)
    assert BT.worst_over_bound(y, ref_y, ATOL, RTOL) > 1.0, fault
    assert BT.worst_over_bound(dw, ref_dw, ATOL, RTOL) > 1.0, fault
    # rows without any neighbour are compared exactly: a single stray product there is flagged however small
    dead = table.shape[0] // 2
    assert torch.equal(ref_y[dead], torch.zeros_like(ref_y[dead]))
    stray = ref_y.clone()
    stray[dead, 0] = 1e-30
    assert not torch.equal(stray[dead], ref_y[dead])


def test_the_planner_answers_the_gates_this_suite_found():
    """Host arithmetic only (the launch queries of tests/test_conv_dispatch_cpu.py).  The flat stem path reads the table through a
    32-bit descriptor: it ends where the table reaches 2^32 bytes, not where n_out K reaches 2^31.  The buffer-offset weight
    gradient forms "no neighbour" as the low 32 bits of 0xFFFFFF * 4 ldx: for ldx > 64 that wraps, and the gate compares the
    wrapped offset with the size of x."""
    from nerf_downstream_amd import _lib

    L, kind = _lib.lib(), _lib.constants("MINK_KERNEL_")

    def flat(n_out):
        rc, info = LW.ask_gather_launch(L, 1000, 32, 28, False, False, n_out, 27, False, 0, 16, 16, 1)
        assert rc == 0 and info.kernel == kind["GATHER2"]
        return info.targ[2]

    last = (1 << 32) // 108  # the last n_out whose table of 27 columns stays under 2^32 bytes
    assert 108 * last < (1 << 32) <= 108 * (last + 1) and (last + 1) * 27 < (1 << 31)
    assert flat(last) == 28 and flat(last + 1) == 0 and flat((1 << 31) // 108 + 1) == 28

    def buf(cin, ldx, n_in):
        rc, info = LW.ask_wgrad_launch(L, n_in, ldx, cin, 64, 64, 1000, 27)
        assert rc == 0 and info.kernel == kind["WGRAD"]
        return info.targ[3]

    for cin, ldx in ((64, 68), (64, 80), (96, 96), (128, 160), (20, 20), (64, 64), (128, 128), (256, 256)):
        none32 = (0xFFFFFF * 4 * ldx) % (1 << 32)  # what __umul24(0xFFFFFFFF, 4 ldx) returns
        fits = min(none32 // (4 * ldx), (1 << 31) // (4 * ldx) - (1 if (1 << 31) % (4 * ldx) == 0 else 0), (1 << 24) - 1)
        assert 4 * ldx * fits <= none32 and 4 * ldx * fits < (1 << 31)
        assert buf(cin, ldx, fits) == 1, (cin, ldx, fits)
        assert buf(cin, ldx, fits + 1) == 0, (cin, ldx, fits + 1)
    assert buf(64, 68, 986_894) == 1 and buf(64, 68, 986_895) == 0  # 2^28 - 272 bytes
    assert buf(96, 96, 5_592_404) == 1 and buf(96, 96, 5_592_405) == 0  # 2^31 - 384 bytes
