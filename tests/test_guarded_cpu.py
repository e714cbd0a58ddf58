"""CPU: the guard-band harness of tests/guarded.py has teeth.  Fake "kernels" on CPU tensors, each with ONE deliberate defect of the
kind tests/test_gpu_guard.py exists to catch, must every one be flagged -- and the correct fake accepted."""
import pytest
import torch

from guarded import ALIGN, MIN_BAND, GuardError, Guarded, assert_finite, check_all

N, C, LD = 5, 3, 4  # a [5, 3] matrix at row pitch 4: one pad column


def _operands():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(N, C, generator=g)
    return Guarded.input(x, ld=LD, name="x"), Guarded((N, LD), cols=C, name="y"), x


def _scale(xg, yg, rows=N, cols=C):
    """The correct fake: y[r][c] = 2 x[r][c] over the logical extents, through the padded views."""
    yg.t[:rows, :cols] = 2.0 * xg.t[:rows, :cols]


def test_layout():
    for shape, dtype in (((N, LD), torch.float32), ((7,), torch.int32), ((3, 2, 5), torch.float64), (1001, torch.float32), (6, torch.float64)):
        g = Guarded(shape, dtype, written="any" if isinstance(shape, int) else None)
        assert g.ptr % ALIGN == 0 and g.band >= MIN_BAND
        assert g.buf.numel() == 2 * g.band + g.nbytes  # the back band starts at the first byte after the payload
        assert g.buf.data_ptr() + g.band == g.ptr
    wide = Guarded((2, 300))
    assert wide.band >= 128 * 300 * 4  # one full 128-row tile of this leading dimension
    f = Guarded((4,), torch.float32)
    assert f.t.view(torch.int32).tolist() == [0x7FC0BEEF] * 4 and bool(torch.isnan(f.t).all())
    assert bool(torch.isnan(Guarded((4,), torch.float64).t).all())
    assert Guarded((4,), torch.int32).t.tolist() == [0x5A5A5A5A] * 4
    xg, _, x = _operands()
    assert torch.equal(xg.logical(), x) and bool(torch.isnan(xg.t[:, C:]).all())
    whole, at = xg.whole()
    assert bool(torch.isnan(whole[:at]).all()) and bool(torch.isnan(whole[at + N * LD :]).all())


@pytest.mark.parametrize("skew", [4, 8, 12, 252])
def test_skewed_payload_keeps_every_check(skew):
    """A payload that starts `skew` bytes behind the 256-byte boundary (a pointer that is not 16-byte aligned): the bands still touch
    the payload at both ends, the sentinel stays element-aligned, and all three checks still fire."""
    def pair():
        g = torch.Generator().manual_seed(0)
        x = torch.randn(N, C, generator=g)
        return Guarded.input(x, ld=LD, name="x", skew=skew), Guarded((N, LD), cols=C, name="y", skew=skew), x

    xg, yg, x = pair()
    for g in (xg, yg):
        assert g.ptr % ALIGN == skew and (g.ptr % 16 != 0) == (skew % 16 != 0)
        assert g.buf.numel() == 2 * g.band + g.nbytes and g.buf.data_ptr() + g.band == g.ptr == g.t.data_ptr()
        whole, at = g.whole()
        assert whole[:at].view(torch.int32).unique().tolist() == [0x7FC0BEEF]  # element-aligned sentinel up to the payload
        assert whole[at + N * LD :].view(torch.int32).unique().tolist() == [0x7FC0BEEF]
    assert yg.t.view(torch.int32).unique().tolist() == [0x7FC0BEEF]
    assert torch.equal(xg.logical(), x) and bool(torch.isnan(xg.t[:, C:]).all())
    _scale(xg, yg)
    check_all(xg, yg)
    assert torch.equal(yg.logical(), 2 * x)
    # one element past the end, one before the start
    whole, at = yg.whole()
    whole[at + N * LD] = 1.0
    with pytest.raises(GuardError, match=rf"back band.*offset {N * LD * 4} .*4 byte"):
        yg.check()
    xg, yg, _ = pair()
    _scale(xg, yg)
    whole, at = yg.whole()
    whole[at - 1] = 1.0
    with pytest.raises(GuardError, match="front band.*offset -4 "):
        yg.check()
    # a stale element
    xg, yg, _ = pair()
    _scale(xg, yg, rows=N - 1)
    with pytest.raises(GuardError, match=rf"still holds the sentinel.*offset {(N - 1) * LD * 4} .*{C * 4} byte"):
        yg.check()
    # a touched pad column, and a modified input
    xg, yg, _ = pair()
    _scale(xg, yg)
    yg.t[2, C] = 0.0
    with pytest.raises(GuardError, match=rf"must not write.*offset {(2 * LD + C) * 4} "):
        yg.check()
    xg.t[N - 1, C - 1] = 9.0
    with pytest.raises(GuardError, match="x: .*must not write"):
        xg.check()
    # a byte workspace and an int64 buffer skew too
    ws = Guarded(1001, torch.uint8, written="any", skew=skew)
    ws.check()
    ws.buf[ws.band + 1001] = 0
    with pytest.raises(GuardError, match="back band.*offset 1001 .*1 byte"):
        ws.check()
    if skew % 8 == 0:
        h = Guarded((3,), torch.int64, skew=skew)
        assert h.ptr % ALIGN == skew and h.t.tolist() == [0x5A5A5A5A5A5A5A5A] * 3


def test_skew_must_keep_elements_aligned():
    with pytest.raises(AssertionError):
        Guarded((4,), torch.float32, skew=2)
    with pytest.raises(AssertionError):
        Guarded((4,), torch.float64, skew=4)
    with pytest.raises(AssertionError):
        Guarded((4,), torch.float32, skew=256)


def test_correct_kernel_is_accepted():
    xg, yg, x = _operands()
    _scale(xg, yg)
    check_all(xg, yg)
    assert_finite(yg.logical())
    assert torch.equal(yg.logical(), 2 * x)
    # a kernel that computes a NaN of its own wrote the element: not "untouched"
    yg2 = Guarded((N, LD), cols=C)
    yg2.t[:, :C] = float("nan")
    yg2.check()
    # a workspace may be written anywhere inside, or not at all
    ws = Guarded(1001, torch.float32, written="any")
    ws.check()
    ws.t[:] = 3
    ws.check()


def test_write_one_element_past_the_payload():
    xg, yg, _ = _operands()
    _scale(xg, yg)
    whole, at = yg.whole()
    whole[at + N * LD] = 1.0
    with pytest.raises(GuardError, match=rf"back band.*offset {N * LD * 4} .*4 byte"):
        yg.check()
    ws = Guarded(1001, torch.uint8, written="any")  # a workspace overrun by ONE byte (no rounding slack)
    ws.buf[ws.band + 1001] = 0
    with pytest.raises(GuardError, match="back band.*offset 1001 .*1 byte"):
        ws.check()


def test_write_one_element_before_the_payload():
    xg, yg, _ = _operands()
    _scale(xg, yg)
    whole, at = yg.whole()
    whole[at - 1] = 1.0
    with pytest.raises(GuardError, match="front band.*offset -4 "):
        yg.check()


def test_last_row_left_unwritten():
    xg, yg, _ = _operands()
    _scale(xg, yg, rows=N - 1)
    with pytest.raises(GuardError, match=rf"still holds the sentinel.*offset {(N - 1) * LD * 4} .*{C * 4} byte"):
        yg.check()


def test_pad_column_written():
    xg, yg, _ = _operands()
    _scale(xg, yg)
    yg.t[2, C] = 0.0
    with pytest.raises(GuardError, match=rf"must not write.*offset {(2 * LD + C) * 4} "):
        yg.check()


def test_unvisited_row_of_an_accumulate_target_touched():
    g = torch.Generator().manual_seed(1)
    init = torch.randn(N, C, generator=g)
    visited = torch.tensor([True, False, True, True, False])
    ok = Guarded((N, LD), cols=C, init=init, written=visited[:, None].expand(N, C))
    ok.t[visited, :C] += 1.0
    ok.check()
    assert torch.equal(ok.logical()[~visited], init[~visited])
    bad = Guarded((N, LD), cols=C, init=init, written=visited[:, None].expand(N, C))
    bad.t[visited, :C] += 1.0
    bad.t[1, 0] += 0.0  # (same bits: adding zero is no store the harness could see, and need not be)
    bad.check()
    bad.t[1, 0] += 1.0
    with pytest.raises(GuardError, match=rf"must not write.*offset {LD * 4} "):
        bad.check()


def test_input_modified():
    xg, yg, _ = _operands()
    _scale(xg, yg)
    xg.t[0, 0] = 9.0
    with pytest.raises(GuardError, match="x: .*must not write"):
        xg.check()


def test_pad_column_let_into_a_sum():
    xg, _, x = _operands()
    s = Guarded((N,), name="row sums")
    s.t[:] = (xg.t * torch.tensor([1.0, 1.0, 1.0, 0.0])).sum(1)  # the pad column "multiplied by zero"
    with pytest.raises(GuardError, match="non-finite"):
        assert_finite(s.t, "row sums")  # the value check sees the poisoned read ...
    with pytest.raises(GuardError, match="still holds the sentinel"):
        s.check()  # ... and so does check(): arithmetic hands a NaN's payload on, the sum IS the sentinel
    s2 = Guarded((N,))
    s2.t[:] = xg.logical().sum(1)
    s2.check()
    assert_finite(s2.t)
    # an entry point whose contract asks for finite pads: large finite values instead of NaN
    xf = Guarded.input(x, ld=LD, pad=2.0 ** 100)
    assert bool((xf.t[:, C:] == 2.0 ** 100).all())
    assert_finite((xf.t * torch.tensor([1.0, 1.0, 1.0, 0.0])).sum(1))


def test_statistics_rows_past_the_reported_count():
    st = Guarded((8, 2, C), torch.float64, name="stats_out")
    st.t[:3] = 1.0
    rows = torch.zeros(8, 2, C, dtype=torch.bool)
    rows[:3] = True
    st.set_written(rows)
    st.check()
    st.t[3, 0, 0] = 0.0
    with pytest.raises(GuardError, match=rf"must not write.*offset {3 * 2 * C * 8} "):
        st.check()
