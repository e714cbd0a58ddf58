"""Non-finite footprints: one NaN, +inf or -inf written into otherwise O(1) data, and where it may and must come out.

The footprint of a tensor is the mask of its non-finite elements.  An operator is held to the footprint of its float64
reference: a poisoned value that the reference lets through must come through (a swallowed NaN lets training go on with
dead channels and a finite loss), and a poisoned value in a row the operator has no business reading must appear nowhere
(0 x NaN is NaN: a clamped re-read of row 0 or a zero-weight multiply shows).

Poison pattern.  Rows 0, n - 1, and 63 / 64 where they exist (either side of a wave / tile boundary) plus, for gather
operators, rows the table does not name (`extra`).  Channels 0, C - 1 and 3 (the last lane of the first 16-byte group), cut
down so that they cover at most half the channels (one channel when C == 1).

same_footprint(got, ref, tol, what, behind=None)
    footprint(got) == footprint(ref); where ref is +-inf, got is the same infinity unless `behind` names one of the two
    written exception classes (ANY_NON_FINITE), where any non-finite value is accepted; the finite elements meet `tol`, the
    tolerance of the operator's existing test: a dict(atol, rtol) as torch.allclose takes it, a tensor of elementwise bounds,
    a (relative L2, relative max) pair in the manner of test_gpu_reduced_math._errs, or None for bitwise equality.
no_swallow(got, ref, what)
    every element non-finite in ref is non-finite in got -- the weaker form for reductions over all rows into a small result
    (dW, dgamma, dbeta, column statistics), where a zero-filled absent neighbour times a NaN legitimately differs from a
    reference that skips the pair.
visible(refs, what) / visible_reduction(refs, what)
    asserted on the reference alone, before the kernel's result is looked at: at least one checked output of the case (one
    operator form under one poison value, experiments (a) and (b)) has a non-empty footprint that covers less than half of
    it (else neither a swallowed nor a leaked value could be seen); for the row-reduction outputs only non-empty.  An output
    that has a single row of which every element mixes all input channels (a one-row GEMM) is all or nothing by
    construction: `visible` then asks for non-empty.
Reached
    the launch forms / cases a test names must all be reached (as Judge.finish of test_gpu_reduced_math.py)."""
import math

import torch

POISONS = {"nan": float("nan"), "+inf": float("inf"), "-inf": float("-inf")}

# the two written exception classes: behind these, a reference infinity may come out as any non-finite value
#   * a normalisation subtracts a mean that is itself infinite: inf - inf = NaN, in an order the formula does not fix
#   * bf16x3 math splits v = hi + lo with hi = rne(v), lo = rne(v - hi): hi = inf, lo = inf - inf = NaN
ANY_NON_FINITE = ("batch norm", "instance norm", "layer norm", "bf16x3")


def poison_rows(n, extra=()):
    """Rows 0, n - 1, 63, 64 (those that exist) and `extra`, ascending, unique."""
    return sorted({r for r in (0, n - 1, 63, 64) if 0 <= r < n} | {int(r) for r in extra})


def poison_channels(C):
    """Channels 0, C - 1, 3 (those that exist), at most half of the channels, at least one."""
    out = []
    for c in (0, C - 1, 3):
        if 0 <= c < C and c not in out and len(out) < max(1, C // 2):
            out.append(c)
    return sorted(out)


def poison(t, value, rows, channels=None):
    """A copy of t [n, C] with `value` at rows x channels (all of poison_channels(C) by default)."""
    out = t.clone()
    if len(rows) == 0:
        return out
    ch = poison_channels(t.shape[1]) if channels is None else list(channels)
    r = torch.as_tensor(list(rows), dtype=torch.long, device=t.device)
    c = torch.as_tensor(ch, dtype=torch.long, device=t.device)
    out[r[:, None], c[None, :]] = value
    return out


def footprint(t):
    return ~torch.isfinite(t)


def _cpu64(t):
    return t.detach().double().cpu()


def visible(refs, what):
    """refs: {name: float64 reference output}.  At least one has 0 < |footprint| < half of it."""
    seen = []
    for name, r in refs.items():
        k, n = int(footprint(r).sum()), r.numel()
        seen.append(f"{name}: {k} of {n}")
        one_row = r.dim() == 2 and r.shape[0] == 1  # (all or nothing, see the module docstring)
        if k > 0 and (2 * k < n or (one_row and k == n)):
            return
    raise AssertionError(f"{what}: no reference footprint is non-empty and below half of its output ({'; '.join(seen)})")


def visible_reduction(refs, what):
    for name, r in refs.items():
        assert int(footprint(r).sum()) > 0, f"{what}: the reference footprint of {name} is empty"


def _finite_close(got, ref, fin, tol, what):
    zero = torch.zeros((), dtype=torch.float64)
    g, r = torch.where(fin, got, zero), torch.where(fin, ref, zero)
    if tol is None:
        assert torch.equal(g, r), f"{what}: finite elements differ (max |err| {float((g - r).abs().max()):.3e})"
    elif isinstance(tol, dict):
        assert torch.allclose(g, r, **tol), f"{what}: finite elements off by {float((g - r).abs().max()):.3e} (tolerance {tol})"
    elif isinstance(tol, tuple):
        tol_rel, tol_max = tol
        d = g - r
        rel = float(d.norm() / r.norm().clamp_min(1e-300))
        mx = float(d.abs().max() / r.abs().max().clamp_min(1e-300)) if r.numel() else 0.0
        assert rel <= tol_rel and mx <= tol_max, f"{what}: finite elements rel {rel:.2e} > {tol_rel:.2e} or max {mx:.2e} > {tol_max:.2e}"
    else:
        bound = torch.where(fin, _cpu64(tol), zero)
        bad = (g - r).abs() > bound
        assert not bool(bad.any()), f"{what}: {int(bad.sum())} finite elements outside their bound (max |err| {float((g - r).abs().max()):.3e})"


def same_footprint(got, ref, tol, what, behind=None):
    assert behind is None or behind in ANY_NON_FINITE, f"{behind!r} is not one of the written exception classes {ANY_NON_FINITE}"
    got, ref = _cpu64(got), _cpu64(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    fg, fr = footprint(got), footprint(ref)
    if not torch.equal(fg, fr):
        swallowed, leaked = fr & ~fg, fg & ~fr
        where = lambda m: m.nonzero()[:4].tolist()  # noqa: E731
        raise AssertionError(f"{what}: footprint differs from the float64 reference's: {int(swallowed.sum())} swallowed "
                             f"(first at {where(swallowed)}), {int(leaked.sum())} leaked (first at {where(leaked)}); "
                             f"reference footprint {int(fr.sum())} of {fr.numel()}")
    if behind is None:
        inf = torch.isinf(ref)
        assert torch.equal(got[inf], ref[inf]), f"{what}: a reference infinity came out as another non-finite value"
    _finite_close(got, ref, ~fr, tol, what)


def no_swallow(got, ref, what):
    got, ref = _cpu64(got), _cpu64(ref)
    assert got.shape == ref.shape, (what, tuple(got.shape), tuple(ref.shape))
    swallowed = footprint(ref) & ~footprint(got)
    assert not bool(swallowed.any()), f"{what}: {int(swallowed.sum())} non-finite reference elements came out finite (first at {swallowed.nonzero()[:4].tolist()})"


def untouched(got, clean, keep, what):
    """The elements of `got` under the mask `keep` are finite and bitwise those of the un-poisoned run `clean`: a region the
    operator must not let the poison reach (another sample, another column, rows beyond n)."""
    got, clean = got.detach().cpu(), clean.detach().cpu()
    keep = keep.expand_as(got) if keep.shape != got.shape else keep
    assert bool(torch.isfinite(got[keep]).all()), f"{what}: a non-finite value leaked where the operator must not read"
    assert torch.equal(got[keep], clean[keep]), f"{what}: the poison changed elements it cannot reach"


class Reached:
    """The cases / launch forms a test names; finish() fails for one that was never reached."""

    def __init__(self, expected):
        self.expected, self.seen = list(expected), {}

    def reach(self, form):
        self.seen[form] = self.seen.get(form, 0) + 1

    def finish(self, title):
        print(f"\n{title}: " + ", ".join(f"{f} x{k}" for f, k in sorted(self.seen.items())))
        missing = set(self.expected) - set(self.seen)
        assert not missing, f"{title}: not reached: {sorted(missing)}"


def is_nan(v):
    return isinstance(v, float) and math.isnan(v)
