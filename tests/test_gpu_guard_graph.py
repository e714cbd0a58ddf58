"""-m gpu: mink_knn, the edge-convolution kernels (csrc/graph.hip) and PAConv (csrc/paconv.hip) inside guard bands
(tests/guarded.py), by the rules of tests/test_gpu_guard.py and tests/test_gpu_guard_match.py: called through the C ABI, every
output, partial and workspace buffer a Guarded of exactly the size include/mink_hip.h, mink_edge_stats_rows() or
mink_edge_bwd_workspace_bytes() names, every input (idx, members, seg and the offsets included) a Guarded.input.  After the call
every buffer is checked, then the values against the float64 restatements:

  mink_knn     integer features: the table equals the restatement's (dgcnn_restate.sq_dists, a stable sort), -1 in the slots
               a sample of fewer than k rows cannot fill.
  edge conv    dgcnn_restate.edge_conv / edge_bounds, the bounds of test_gpu_dgcnn, on a layer whose two GEMMs are identities:
               features x = [P | Q] and W1 = [I 0], W2 = [I I] make X W1^T = P and X (W2 - W1)^T = Q exactly, so the
               restatement's y, batch statistics, dgamma and dbeta are those of the kernels' operands and its dx is [dP | dQ].
  PAConv       paconv_restate.paconv_grads / paconv_bounds, the bounds of test_gpu_paconv, on a DGCNN-flavour bank of O = 2 M Cin
               outputs whose [Wn ; -Wc] is the identity: y = [A | CX], and dy = [dA | dCX].

Index values the header promises to tolerate are in every table: -1 and n.  The edge kernels clamp such a slot to row 0 or
n - 1 (the restatement is handed the clamped table, and the incoming-edge lists are those of the clamped table); PAConv
skips it (its lists keep such slots behind the last segment, as functional.index_csr builds them).  Nothing here is meant to
fault."""
import pytest
import torch

import dgcnn_restate as DG
import paconv_restate as PA
from guarded import Guarded, assert_finite, check_all

pytestmark = pytest.mark.gpu


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


def _lib():
    from nerf_downstream_amd._lib import check, lib

    return lib(), check


def _done(*bufs):
    torch.cuda.synchronize()
    check_all(*bufs)


def _randn(shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def _within(got, ref, bound, what):
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert_finite(got, what)
    err = (got.double() - ref).abs()
    assert bool((err <= bound).all()), (what, float(err.max()), float((err - bound).max()))


def _csr(idx, n, clamp):
    """(members, seg) of the flat slot ids grouped by idx, ascending inside a segment (a stable sort).  clamp: a slot outside
    [0, n) belongs to row 0 or n - 1; otherwise it lies behind the last segment (functional.index_csr)."""
    flat = idx.reshape(-1).long()
    key = flat.clamp(0, n - 1) if clamp else torch.where((flat >= 0) & (flat < n), flat, torch.full_like(flat, n))
    members = torch.sort(key, stable=True).indices
    seg = torch.zeros(n + 1, dtype=torch.int64)
    seg[1:] = torch.cumsum(torch.bincount(key, minlength=n + 1)[:n], 0)
    return members.int(), seg.int()


def _table(n, k, seed):
    """idx [n][k] of random rows with some slots -1 and some n (about 6 % each once the table is large enough)."""
    g = torch.Generator().manual_seed(seed)
    idx = torch.randint(0, n, (n, k), generator=g)
    r = torch.rand(n, k, generator=g)
    idx[r < 0.06] = -1
    idx[r > 0.94] = n
    if n * k >= 2:
        idx.view(-1)[0], idx.view(-1)[-1] = n, -1
    return idx


# ================================================================================================ kNN
@pytest.mark.parametrize("k", [1, 20, 64])
@pytest.mark.parametrize("C", [3, 32, 33, 256])
def test_knn_stays_inside_its_buffers(C, k):
    """Samples: 193 rows (the boundaries fall inside a 32-row query tile and the sample straddles a 128-row candidate tile),
    an empty one, one of k - 1 rows (fewer than k: the last slot of its rows is -1), 131 rows.  Integer features with |x| <= 8:
    every norm and inner product is an integer below 2^24, the fp32 ranking score is exact and the table must equal the
    restatement's."""
    L, check = _lib()
    off = [0, 193, 193, 193 + k - 1, 193 + k - 1 + 131]
    n, B = off[-1], 4
    g = torch.Generator().manual_seed(100 * C + k)
    x = torch.randint(-8, 9, (n, C), generator=g).float()
    x[30:55] = x[30]  # equal distances: the lower row first
    ref = torch.full((n, k), -1, dtype=torch.int64)
    for b in range(B):
        lo, hi = off[b], off[b + 1]
        if hi > lo:
            m = min(k, hi - lo)
            ref[lo:hi, :m] = torch.sort(DG.sq_dists(x, lo, hi), dim=1, stable=True).indices[:, :m] + lo
    big = [0, 193, 193 + k - 1, n]
    assert torch.equal(ref[:193], DG.knn(x[:193], [0, 193], k)) and torch.equal(ref[big[2]:] - big[2], DG.knn(x[big[2]:], [0, 131], k))
    ldx = C + 5
    gx, goff, gidx = _gin(x, ld=ldx, name="x"), _gin(torch.tensor(off, dtype=torch.int32), name="batch_offsets"), _gout((n, k), torch.int32, name="idx")
    check(L.mink_knn(gx.ptr, n, ldx, C, goff.ptr, B, k, gidx.ptr, _st()))
    _done(gx, goff, gidx)
    got = gidx.t.cpu().long()
    assert torch.equal(got, ref), (C, k, int((got != ref).sum()))
    if k > 1:
        assert bool((got[193:193 + k - 1, k - 1] == -1).all()) and bool((got[193:193 + k - 1, :k - 1] >= 193).all())


# ================================================================================================ edge convolution
def _edge_layer(n, C, k, seed):
    """Operands P, Q [n][C] as the features x = [P | Q] of a layer whose weights select them: W = [W1 | W2], W1 = [I 0], W2 = [I I]."""
    x = _randn((n, 2 * C), seed)
    eye, zero = torch.eye(C), torch.zeros(C, C)
    W = torch.cat([torch.cat([eye, zero], 1), torch.cat([eye, eye], 1)], 1)  # [C][2 * 2C]
    gamma = torch.rand(C, generator=torch.Generator().manual_seed(seed + 2)) + 0.5
    beta = _randn((1, C), seed + 3)[0] * 0.3
    rm = _randn((1, C), seed + 4)[0] * 0.2
    rv = torch.rand(C, generator=torch.Generator().manual_seed(seed + 5)) + 0.5
    dy = _randn((n, C), seed + 6)
    return x, W, gamma, beta, rm, rv, dy


EDGE_CASES = [(n, C, k) for n in (1, 41) for C in (3, 64, 65) for k in (1, 20, 64)] + [(4133, 3, 20), (4133, 65, 1)]


@pytest.mark.parametrize("n,C,k", EDGE_CASES)
def test_edge_conv_stays_inside_its_buffers(n, C, k):
    """n = 4 m + 1 leaves the last workgroup of the four-row kernels one live row; n = 4133 > 256 * 16 caps the chunked
    reductions at 256 partial rows of 17 rows each."""
    L, check = _lib()
    x, W, gamma, beta, rm, rv, dy = _edge_layer(n, C, k, 8000 + 100 * C + k + n)
    P, Q = x[:, :C].contiguous(), x[:, C:].contiguous()
    idx = _table(n, k, 8001 + C + k + n)
    cl = idx.clamp(0, n - 1)  # what the kernels follow
    assert n * k < 2 or (int((idx < 0).sum()) > 0 and int((idx >= n).sum()) > 0)
    M = n * k
    gP, gQ, gidx = _gin(P, name="P"), _gin(Q, name="Q"), _gin(idx.int(), name="idx")
    rows = L.mink_edge_stats_rows(n)
    assert rows == max(1, min(-(-n // 16), 256))
    gpart = _gout((rows, 2, C), torch.float64, name="partial")
    assert gpart.nbytes == rows * 2 * C * 8
    check(L.mink_edge_stats(gP.ptr, gQ.ptr, gidx.ptr, n, k, C, gpart.ptr, gpart.nbytes, _st()))
    _done(gP, gQ, gidx, gpart)
    part = gpart.t.cpu()
    assert_finite(part, "edge_stats partials")
    s, ss = part[:, 0].sum(0), part[:, 1].sum(0)
    mean_b, var_b = s / M, (ss / M - (s / M) ** 2).clamp_min(0)
    members, seg = _csr(idx, n, clamp=True)
    gm, gs = _gin(members, name="members"), _gin(seg, name="seg")
    gga, gbe, gdy = _gin(gamma, name="gamma"), _gin(beta, name="beta"), _gin(dy, name="dy")
    need = L.mink_edge_bwd_workspace_bytes(n, C)
    assert need == -(-n * C * 4 // 256) * 256 + -(-rows * 2 * C * 8 // 256) * 256
    for training in (1, 0):
        what = f"edge n={n} C={C} k={k} training={training}"
        stats = None if training else (rm.double(), rv.double())
        leaves = [t.double().requires_grad_(True) for t in (x, W, gamma, beta)]
        ry, rarg, (mean, var) = DG.edge_conv(*leaves, cl, stats)
        ry.backward(dy.double())
        bounds = DG.edge_bounds(x, W, gamma, beta, cl, dy, stats)
        mean, var = mean.detach(), var.detach()
        if training:  # the batch statistics of the partials (mink_bn_stats_from_partials: mean, 1 / sqrt(biased var + eps))
            _within(mean_b, mean, bounds["mean"], what + " mean of the partials")
            _within(var_b, var, bounds["var"], what + " var of the partials")
            mu32, is32 = mean_b.float(), (1.0 / torch.sqrt(var_b + DG.BN_EPS)).float()
        else:
            mu32, is32 = rm, (1.0 / torch.sqrt(rv.double() + DG.BN_EPS)).float()
        gmu, gis = _gin(mu32, name="mean"), _gin(is32, name="invstd")
        gy, garg = _gout((n, C), name="y"), _gout((n, C), torch.uint8, name="arg")
        check(L.mink_edge_fwd(gP.ptr, gQ.ptr, gidx.ptr, n, k, C, gmu.ptr, gis.ptr, gga.ptr, gbe.ptr, gy.ptr, garg.ptr, _st()))
        _done(gP, gQ, gidx, gmu, gis, gga, gbe, gy, garg)
        assert torch.equal(garg.t.cpu().long(), rarg), (what, int((garg.t.cpu().long() != rarg).sum()))
        _within(gy.t.cpu(), ry.detach(), bounds["y"], what + " y")
        gain = _gin(rarg.to(torch.uint8), name="arg (in)")
        gdP, gdQ, gdga, gdbe = _gout((n, C), name="dP"), _gout((n, C), name="dQ"), _gout((C,), name="dgamma"), _gout((C,), name="dbeta")
        ws = Guarded(int(need), torch.uint8, _dev(), written="any", name="edge_bwd workspace")
        check(L.mink_edge_bwd(gdy.ptr, gP.ptr, gQ.ptr, gidx.ptr, gain.ptr, n, k, C, gmu.ptr, gis.ptr, gga.ptr, gbe.ptr, training, gm.ptr, gs.ptr,
                              gdP.ptr, gdQ.ptr, gdga.ptr, gdbe.ptr, ws.ptr, ws.nbytes, _st()))
        _done(gdy, gP, gQ, gidx, gain, gmu, gis, gga, gbe, gm, gs, gdP, gdQ, gdga, gdbe, ws)
        _within(torch.cat([gdP.t.cpu(), gdQ.t.cpu()], 1), leaves[0].grad, bounds["dx"], what + " [dP | dQ]")
        _within(gdga.t.cpu(), leaves[2].grad, bounds["dgamma"], what + " dgamma")
        _within(gdbe.t.cpu(), leaves[3].grad, bounds["dbeta"], what + " dbeta")
        if training and n == 41:
            # the lists functional.index_csr builds: the slots outside [0, n) behind the last segment.  dQ, dgamma and dbeta do
            # not read the lists; dP differs only in rows 0 and n - 1, where the clamped slots arrive.
            m2, s2 = _csr(idx, n, clamp=False)
            assert int(s2[-1]) < M
            gm2, gs2 = _gin(m2, name="members"), _gin(s2, name="seg")
            hP, hQ, hga, hbe = _gout((n, C), name="dP"), _gout((n, C), name="dQ"), _gout((C,), name="dgamma"), _gout((C,), name="dbeta")
            ws2 = Guarded(int(need), torch.uint8, _dev(), written="any", name="edge_bwd workspace")
            check(L.mink_edge_bwd(gdy.ptr, gP.ptr, gQ.ptr, gidx.ptr, gain.ptr, n, k, C, gmu.ptr, gis.ptr, gga.ptr, gbe.ptr, training, gm2.ptr,
                                  gs2.ptr, hP.ptr, hQ.ptr, hga.ptr, hbe.ptr, ws2.ptr, ws2.nbytes, _st()))
            _done(gdy, gP, gQ, gidx, gain, gmu, gis, gga, gbe, gm2, gs2, hP, hQ, hga, hbe, ws2)
            assert_finite(hP.t, what + " dP")
            assert torch.equal(hQ.t, gdQ.t) and torch.equal(hga.t, gdga.t) and torch.equal(hbe.t, gdbe.t) and torch.equal(hP.t[1:-1], gdP.t[1:-1])


# ================================================================================================ PAConv
def _identity_bank(M, cin):
    """matrice [2 Cin][M * O], O = 2 M Cin, of the DGCNN flavour ([K1 ; K2], Wn = K1 + K2, Wc = K1) with
    Wn[c][m][o] = [o == m Cin + c] and -Wc[c][m][o] = [o == M Cin + m Cin + c]: y = [A | CX] flattened over (m, c)."""
    O = 2 * M * cin
    Wn, Wc = torch.zeros(cin, M, O), torch.zeros(cin, M, O)
    c, m = torch.meshgrid(torch.arange(cin), torch.arange(M), indexing="ij")
    Wn[c, m, m * cin + c] = 1.0
    Wc[c, m, M * cin + m * cin + c] = -1.0
    return torch.cat([Wc, Wn - Wc], 0).reshape(2 * cin, M * O)


PACONV_CASES = [  # (M, Cin, k, ldz): "tight" = M Cin, "double" = the halves of one [n][2 M Cin] buffer, "odd" = M Cin + 1
    (1, 3, 1, "tight"), (3, 4, 20, "double"), (4, 64, 20, "double"), (8, 65, 20, "odd"), (12, 4, 1, "tight"), (16, 3, 20, "double"),
    (4, 260, 20, "double"), (16, 4, 20, "odd"), (8, 260, 1, "tight"), (1, 65, 20, "double"), (3, 64, 1, "odd"), (12, 64, 1, "double"),
    (8, 4, 20, "tight"), (16, 65, 1, "tight"), (4, 3, 20, "odd"), (1, 260, 20, "tight"),
]


def _run_paconv(M, cin, k, ldz_kind, seed, skew=None):
    L, check = _lib()
    n = 70 if M * M * cin * k <= 50000 else 37  # (the restatement forms [n][k][M][2 M Cin] doubles)
    MC = M * cin
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cin, generator=g)
    s = torch.softmax(torch.randn(n, k, M, generator=g), 2) + 0.5
    dy = torch.randn(n, 2 * MC, generator=g)  # = [dA | dCX]
    idx = _table(n, k, seed + 1)
    bank = _identity_bank(M, cin)
    ref = PA.paconv_grads(x, bank, s, idx, "dgcnn", dy)
    bounds = PA.paconv_bounds(x, bank, s, idx, "dgcnn", dy)
    ok = (idx >= 0) & (idx < n)
    S_ref = (s.double() * ok[..., None]).sum(1)
    what = f"paconv M={M} Cin={cin} k={k} ldz {ldz_kind}"
    sk = lambda name: 4 if skew == name else 0  # noqa: E731
    gx, gsc, gidx = _gin(x, name="x", skew=sk("x")), _gin(s, name="s"), _gin(idx.int(), name="idx")
    double = ldz_kind == "double"
    ldz = {"tight": MC, "double": 2 * MC, "odd": MC + 1}[ldz_kind]

    def pair(name, init=None):
        """A and CX (dA and dCX): the halves of one guarded [n][2 M Cin] buffer, or two buffers of pitch ldz with their own pads."""
        if double:
            if init is None:
                both = _gout((n, 2 * MC), name=name, skew=sk("A"))
            else:
                both = _gin(init, name=name, skew=sk("dA"))
            return [both], both.ptr, both.ptr + MC * 4
        if init is None:
            a, b = _gout((n, ldz), cols=MC, name=name + " A", skew=sk("A")), _gout((n, ldz), cols=MC, name=name + " CX")
        else:
            a, b = _gin(init[:, :MC], ld=ldz, name=name + " dA", skew=sk("dA")), _gin(init[:, MC:], ld=ldz, name=name + " dCX")
        return [a, b], a.ptr, b.ptr

    def read(bufs):
        return bufs[0].t.cpu() if double else torch.cat([bufs[0].logical().cpu(), bufs[1].logical().cpu()], 1)

    # gather: A, CX and S in one pass
    out, pA, pCX = pair("[A | CX]")
    gS = _gout((n, M), name="S")
    vec = cin % 4 == 0 and ldz % 4 == 0 and all(p % 16 == 0 for p in (gx.ptr, pA, pCX))
    assert vec == (cin % 4 == 0 and ldz_kind != "odd" and skew not in ("x", "A")), what
    check(L.mink_paconv_gather(gx.ptr, gsc.ptr, gidx.ptr, n, k, M, cin, pA, pCX, ldz, gS.ptr, _st()))
    _done(gx, gsc, gidx, gS, *out)
    _within(read(out), ref["y"], bounds["y"], what + " [A | CX]")
    _within(gS.t.cpu(), S_ref, k * PA.U32 * S_ref.abs(), what + " S")  # k plain additions of non-negative scores (paconv_bounds: "S = sum_j s: k")
    # ... and A alone: the same bits, nothing else written
    if double:
        only = [_gout((n, 2 * MC), cols=MC, name="A alone", skew=sk("A"))]
    else:
        only = [_gout((n, ldz), cols=MC, name="A alone", skew=sk("A"))]
    check(L.mink_paconv_gather(gx.ptr, gsc.ptr, gidx.ptr, n, k, M, cin, only[0].ptr, None, ldz, None, _st()))
    _done(gx, gsc, gidx, *only)
    assert torch.equal(only[0].logical(), (out[0].t[:, :MC] if double else out[0].logical())), what + " A alone"
    # score gradient
    gin, pdA, pdCX = pair("[dA | dCX]", dy)
    gds = _gout((n, k, M), name="ds")
    check(L.mink_paconv_score_bwd(pdA, pdCX, ldz, gx.ptr, gidx.ptr, n, k, M, cin, gds.ptr, _st()))
    _done(gx, gidx, gds, *gin)
    _within(gds.t.cpu(), ref["ds"], bounds["ds"], what + " ds")
    assert bool((gds.t.cpu()[~ok] == 0).all()), what + ": a slot outside [0, n) gets ds == 0"
    # feature gradient, through the lists of functional.index_csr
    members, seg = _csr(idx, n, clamp=False)
    assert int(seg[-1]) < n * k
    gm, gs, gSin = _gin(members, name="members"), _gin(seg, name="seg"), _gin(gS.t.clone(), name="S (in)")
    gdx = _gout((n, cin), name="dx", skew=sk("dx"))
    check(L.mink_paconv_scatter_bwd(pdA, pdCX, ldz, gsc.ptr, gSin.ptr, gm.ptr, gs.ptr, n, k, M, cin, gdx.ptr, _st()))
    _done(gsc, gSin, gm, gs, gdx, *gin)
    _within(gdx.t.cpu(), ref["dx"], bounds["dx"], what + " dx")


@pytest.mark.parametrize("M,cin,k,ldz", PACONV_CASES)
def test_paconv_stays_inside_its_buffers(M, cin, k, ldz):
    _run_paconv(M, cin, k, ldz, 9000 + 100 * M + cin + k)


@pytest.mark.parametrize("which", ["x", "A", "dA", "dx"])
def test_paconv_with_one_pointer_off_16_bytes_takes_dword_lanes(which):
    """Cin % 4 == 0 and every pitch a multiple of 4: an input (x, dA) or an output (A, dx) 4 bytes behind a 16-byte boundary."""
    _run_paconv(4, 8, 20, "double" if which in ("A", "dA") else "tight", 9100, skew=which)
