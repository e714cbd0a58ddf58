"""-m gpu: the segmentation tail of csrc/seghead.hip (mink_seg_ce_forward / _backward) inside guard bands (tests/guarded.py),
by the rules of tests/test_gpu_guard.py: called through the C ABI with lse, pred, hist, the 40 bytes of stats, the loss word, dz
and a workspace of exactly mink_seg_ce_workspace_bytes() as Guarded buffers, and the logits (row pitch ldz, NaN pad columns
where ldz > C), labels, class weights, lse, stats and grad_loss of the backward as Guarded.input.  After the call every
buffer is checked, then the values: pred, hist and the three counts equal seghead_restate's, the loss, num, den and dz lie
within the bounds of test_gpu_seghead._check_against_restatement (imported), lse within the per-row bound that test's
docstring derives the loss bound from.

The kernels stage 16-byte runs when ldz == C and the logits are 16-byte aligned, dwords otherwise: every C runs contiguous
and aligned, with ldz > C, and contiguous with the logits (forward) or dz (backward) 4 bytes behind a 16-byte boundary.  C
sits on both sides of SEG_HIST_LDS_C = 64 (the workgroup's private histogram in LDS, or global atomics).  Nothing here is
meant to fault."""
import numpy as np
import pytest
import torch

import seghead_restate as R
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu

IGNORE = 255
SEG_MAX_GRID = 2048


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


def _tile_rows(C):
    return 256 if C <= 40 else (128 if C <= 80 else 64)


def _run_empty(L, check, C, ldz, want_hist):
    ghist = _gout((C, C), torch.int64, name="hist") if want_hist else None
    gstats, gloss = _gout((5,), torch.int64, name="stats"), _gout((1,), name="loss")
    need = L.mink_seg_ce_workspace_bytes(0, C)
    assert need == 40
    ws = Guarded(int(need), torch.uint8, _dev(), written="any", name="workspace")
    check(L.mink_seg_ce_forward(None, ldz, None, 1, None, IGNORE, 0, C, None, None, _ptr(ghist), gstats.ptr, gloss.ptr, ws.ptr, ws.nbytes, _st()))
    torch.cuda.synchronize()
    check_all(ghist, gstats, gloss, ws)
    assert np.isnan(float(gloss.t[0])) and bool((gstats.t == 0).all())  # (the doubles' zero is all bits clear too)
    assert ghist is None or bool((ghist.t == 0).all())
    check(L.mink_seg_ce_backward(None, ldz, None, 1, None, IGNORE, None, gstats.ptr, None, 0, C, None, _st()))  # nothing to write
    torch.cuda.synchronize()
    check_all(gstats)


def _run(n, C, ldz, int64, weighted, want_pred, want_hist, seed, skew_z=0, skew_dz=0):
    import test_gpu_seghead as TS
    from nerf_downstream_amd._lib import check, lib

    assert TS.IGNORE == IGNORE
    L = lib()
    z, labels, w = R.make_case(n, C, seed, ignore=IGNORE, weighted=weighted, ties=True, bad=3 if n >= 257 else 0)
    if n == 1:
        labels[:] = 1 % C  # (the one row is valid: the mean is over something)
    if n == 0:  # no rows: the header lets logits, labels and lse be NULL; stats, loss, hist and the workspace are still written
        return _run_empty(L, check, C, ldz, want_hist)
    gz = _gin(torch.from_numpy(z).reshape(n, C), ld=ldz, name="z", skew=skew_z)
    gl = _gin(torch.from_numpy(labels if int64 else labels.astype(np.int32)), name="labels")
    gw = _gin(torch.from_numpy(w), name="w") if w is not None else None
    glse = _gout((n,), name="lse")
    gpred = _gout((n,), torch.int32, name="pred") if want_pred else None
    ghist = _gout((C, C), torch.int64, name="hist") if want_hist else None
    gstats = _gout((5,), torch.int64, name="stats")  # 40 bytes: two doubles, three int64
    gloss = _gout((1,), name="loss")
    need = L.mink_seg_ce_workspace_bytes(n, C)
    assert need == 40 * max(1, min(-(-n // _tile_rows(C)), SEG_MAX_GRID)) and gstats.nbytes == 40
    ws = Guarded(int(need), torch.uint8, _dev(), written="any", name="workspace")
    vec_fwd = ldz == C and gz.ptr % 16 == 0
    assert vec_fwd == (ldz == C and skew_z == 0)
    check(L.mink_seg_ce_forward(gz.ptr, ldz, gl.ptr, int(int64), _ptr(gw), IGNORE, n, C, glse.ptr, _ptr(gpred), _ptr(ghist), gstats.ptr, gloss.ptr,
                                ws.ptr, ws.nbytes, _st()))
    torch.cuda.synchronize()
    check_all(gz, gl, gw, glse, gpred, ghist, gstats, gloss, ws)
    tag = f"guard {n}x{C} ld{ldz} {'i64' if int64 else 'i32'} {'w' if weighted else '-'}"
    stats = gstats.t.cpu()
    st = {"num": float(stats[:2].view(torch.float64)[0]), "den": float(stats[:2].view(torch.float64)[1]), "n_valid": int(stats[2]),
          "n_ignored": int(stats[3]), "n_bad": int(stats[4])}
    valid, ignored, bad = R.classify(labels, C, IGNORE)
    assert (st["n_valid"], st["n_ignored"], st["n_bad"]) == (int(valid.sum()), int(ignored.sum()), int(bad.sum())), tag
    pred = R.argmax_first(z) if n else np.zeros(0, dtype=np.int64)
    if want_pred:
        assert np.array_equal(gpred.t.cpu().numpy(), pred), tag
    if want_hist:
        assert np.array_equal(ghist.t.cpu().numpy(), R.fast_hist(pred, labels, C, IGNORE)), tag
    assert n < 257 or int(bad.sum()) == 3
    # backward: lse and stats as the forward left them, now inputs
    g = 0.75
    glse_in, gstats_in = _gin(glse.t.clone(), name="lse (in)"), _gin(gstats.t.clone(), name="stats (in)")
    gg = _gin(torch.tensor([g]), name="grad_loss")
    gdz = _gout((n, C), name="dz", skew=skew_dz)
    vec_bwd = ldz == C and gz.ptr % 16 == 0 and gdz.ptr % 16 == 0
    assert vec_bwd == (ldz == C and skew_z == 0 and skew_dz == 0)
    check(L.mink_seg_ce_backward(gz.ptr, ldz, gl.ptr, int(int64), _ptr(gw), IGNORE, glse_in.ptr, gstats_in.ptr, gg.ptr, n, C, gdz.ptr, _st()))
    torch.cuda.synchronize()
    check_all(gz, gl, gw, glse_in, gstats_in, gg, gdz)
    assert_finite(glse.t, "lse"), assert_finite(gdz.t, "dz"), assert_finite(gloss.t, "loss")
    ref = TS._check_against_restatement(z, labels, w, {"loss": gloss.t[0], "st": st, "dz": gdz.t}, g=g, tag=tag)
    bound = (C + 8) * 2.0 ** -24 * max(1.0, float(np.abs(z).max()))  # the per-row bound the loss inherits (test_gpu_seghead)
    assert float(np.abs(glse.t.cpu().numpy().astype(np.float64) - ref["lse"]).max()) <= bound, tag


@pytest.mark.parametrize("n", [0, 1, 257, 5000])
@pytest.mark.parametrize("C", [2, 20, 64, 65, 128])
def test_seg_ce_stays_inside_its_buffers(C, n):
    i = [2, 20, 64, 65, 128].index(C) + [0, 1, 257, 5000].index(n)
    for j, ldz in enumerate((C, C + 3, C + 4)):  # 16-byte runs; dwords through a pitch, odd and a multiple of 4
        v = i + j
        _run(n, C, ldz, int64=bool(v & 1), weighted=bool(v & 2), want_pred=j != 1 or bool(v & 4), want_hist=j != 2 or not bool(v & 4),
             seed=7000 + 10 * C + n + j)


@pytest.mark.parametrize("C", [20, 65])
def test_seg_ce_without_prediction_and_histogram(C):
    _run(257, C, C, int64=True, weighted=True, want_pred=False, want_hist=False, seed=7100 + C)
    _run(257, C, C + 1, int64=False, weighted=False, want_pred=False, want_hist=True, seed=7101 + C)
    _run(257, C, C, int64=False, weighted=False, want_pred=True, want_hist=False, seed=7102 + C)


@pytest.mark.parametrize("which", ["z", "dz"])
@pytest.mark.parametrize("C", [20, 128])
def test_seg_ce_with_one_pointer_off_16_bytes_takes_dword_loads(C, which):
    _run(257, C, C, int64=True, weighted=True, want_pred=True, want_hist=True, seed=7200 + C, **{"skew_" + which: 4})
