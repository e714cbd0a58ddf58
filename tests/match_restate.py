"""float64 restatement of the cross-cloud nearest-neighbour search (csrc/graph.hip mink_knn_cross,
nerf_downstream_amd/minkowski/graph.py knn_cross) and of the radius matching built on it, independent of the backend: direct
squared differences and a stable sort.  Nothing here calls the code under test.

Row i of q belongs to sample b when q_off[b] <= i < q_off[b + 1]; its neighbours are the rows j of c with
c_off[b] <= j < c_off[b + 1] and the smallest sum_ch (q_i[ch] - c_j[ch])^2, ascending, equal distances in ascending row order.
A sample with m < k candidates fills m slots; the others hold -1 (distance +inf).

Validity on data where fp32 cannot reproduce the float64 order.  The kernel ranks by s_ij = fl(||c_j||^2 - 2 q_i . c_j); the
derivation of tests/test_gpu_dgcnn.py::test_knn_validity_on_normal_data carries over with q_i in place of x_i:
|s^_ij - s_ij| <= (C + 2) u (||q_i|| + max_j ||c_j||)^2 =: e_i, u = 2^-24, and tau_i = 2 e_i: every chosen j has
d64 <= d_(k') + tau_i and every unchosen j of the sample d64 >= d_(k') - tau_i, k' = min(k, m)."""
import torch

F64 = torch.float64
U32 = 2.0 ** -24


def offsets(k):
    """The samples every GPU case uses: (q_off, c_off).  Sample 0: 193 queries, 150 candidates (the boundaries fall inside a
    32-row query tile and a 128-row candidate tile); sample 1: empty on both sides; sample 2: k queries and fewer than k
    candidates (k - 1, or 1 for k = 1); sample 3: 67 queries, 131 candidates."""
    m = k - 1 if k > 1 else 1
    return [0, 193, 193, 193 + k, 260 + k], [0, 150, 150, 150 + m, 150 + m + 131]


def cross_sq_dists(q, c, qlo, qhi, clo, chi):
    """float64 [qhi - qlo, chi - clo] by direct differences."""
    return ((q[qlo:qhi].to(F64)[:, None, :] - c[clo:chi].to(F64)[None, :, :]) ** 2).sum(-1)


def knn_cross(q, c, q_off, c_off, k):
    """-> (idx int64 [nq, k] of global rows of c, -1 past the sample's candidate count; dist float64 [nq, k], +inf there)."""
    idx = torch.full((q.shape[0], k), -1, dtype=torch.int64)
    dist = torch.full((q.shape[0], k), float("inf"), dtype=F64)
    for b in range(len(q_off) - 1):
        qlo, qhi, clo, chi = q_off[b], q_off[b + 1], c_off[b], c_off[b + 1]
        m = min(k, chi - clo)
        if qhi == qlo or m == 0:
            continue
        s = torch.sort(cross_sq_dists(q, c, qlo, qhi, clo, chi), dim=1, stable=True)
        idx[qlo:qhi, :m] = s.indices[:, :m] + clo
        dist[qlo:qhi, :m] = s.values[:, :m]
    return idx, dist


def cross_tau(q, c, qlo, qhi, clo, chi):
    """tau [qhi - qlo] = 2 (C + 2) u (||q_i|| + max_j ||c_j||)^2 over the candidates of the sample."""
    nq = q[qlo:qhi].to(F64).norm(dim=1)
    nc = c[clo:chi].to(F64).norm(dim=1)
    return 2.0 * (q.shape[1] + 2) * U32 * (nq + nc.max()) ** 2


def cross_violations(q, c, q_off, c_off, idx, k):
    """-> (rows with an index outside their sample or a -1 in the wrong place, rows with a repeated index, the largest
    (d64 - d_(k') - tau_i) over the chosen, the largest (d_(k') - tau_i - d64) over the unchosen); valid when the first two are
    0 and the last two <= 0 (-inf where there is nothing to compare)."""
    idx = idx.long()
    outside = repeated = 0
    worst_in = worst_out = -float("inf")
    for b in range(len(q_off) - 1):
        qlo, qhi, clo, chi = q_off[b], q_off[b + 1], c_off[b], c_off[b + 1]
        if qhi == qlo:
            continue
        m = min(k, chi - clo)
        rows = idx[qlo:qhi]
        bad = (rows[:, m:] != -1).any(1)
        if m == 0:
            outside += int(bad.sum())
            continue
        loc = rows[:, :m] - clo
        bad |= ((loc < 0) | (loc >= chi - clo)).any(1)
        outside += int(bad.sum())
        loc = loc.clamp(0, chi - clo - 1)
        repeated += int((torch.sort(loc, dim=1).values.diff(dim=1) == 0).any(1).sum())
        d = cross_sq_dists(q, c, qlo, qhi, clo, chi)
        tau = cross_tau(q, c, qlo, qhi, clo, chi)
        dk = torch.sort(d, dim=1).values[:, m - 1]
        chosen = torch.zeros_like(d, dtype=torch.bool).scatter_(1, loc, True)
        worst_in = max(worst_in, float((d - (dk + tau)[:, None])[chosen].max()))
        if bool((~chosen).any()):
            worst_out = max(worst_out, float(((dk - tau)[:, None] - d)[~chosen].max()))
    return outside, repeated, worst_in, worst_out


def matching_indices(source, target, trans, radius, K=None):
    """int64 [m, 2]: the pairs (i, j) with |trans(source_i) - target_j| <= radius in float64, i ascending, per i distance
    ascending (equal distances in ascending j), at most K per i."""
    s = source.to(F64) @ trans[:3, :3].to(F64).t() + trans[:3, 3].to(F64)
    d = ((s[:, None, :] - target.to(F64)[None, :, :]) ** 2).sum(-1)
    order = torch.sort(d, dim=1, stable=True)
    out = []
    for i in range(d.shape[0]):
        js = order.indices[i][order.values[i] <= radius ** 2]
        out += [(i, int(j)) for j in (js if K is None else js[:K])]
    return torch.tensor(out, dtype=torch.int64).reshape(-1, 2)
