"""CPU: DGCNN_cls in the registry with the reference's state-dict layout, the config, the argument checks of the graph entries
of the C ABI (no GPU: every check comes before the first launch), and the float64 restatement of tests/dgcnn_restate.py
against the neighbour sets the reference's own `knn` returned (tests/golden/dgcnn_knn_v1.npz, scripts/make_dgcnn_golden.py)
and against the P / Q form of the edge convolution and its explicit backward, which is what csrc/graph.hip evaluates."""
import os

import numpy as np
import pytest
import torch

import dgcnn_restate as DG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")
BN = ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")


def _expected_state(in_channel=3, out_channel=40, emb=1024, channels=(64, 64, 128, 256), head=(512, 256)):
    """The reference's keys and shapes (dgcnn.py:48-79), in registration order."""
    out, cin = [], in_channel
    bn = lambda name, c: [(f"{name}.{k}", () if k == "num_batches_tracked" else (c,)) for k in BN]  # noqa: E731
    for i, c in enumerate(channels, start=1):
        out += [(f"conv{i}.0.weight", (c, 2 * cin, 1, 1))] + bn(f"conv{i}.1", c)
        cin = c
    out += [("conv5.0.weight", (emb, sum(channels), 1))] + bn("conv5.1", emb)
    out += [("linear1.weight", (head[0], 2 * emb))] + bn("bn6", head[0])
    out += [("linear2.weight", (head[1], head[0])), ("linear2.bias", (head[1],))] + bn("bn7", head[1])
    out += [("linear3.weight", (out_channel, head[1])), ("linear3.bias", (out_channel,))]
    return out


def test_registry_and_reference_state_dict_layout():
    from nerf_downstream_amd.co3d_3d.src.models import MODELS, get_model

    assert "DGCNN_cls" in MODELS
    model = get_model("DGCNN_cls", 3, 40)
    assert type(model).__name__ == "DGCNN_cls" and model.k == 20
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == _expected_state()
    assert _expected_state()[0] == ("conv1.0.weight", (64, 6, 1, 1)) and _expected_state()[24] == ("conv5.0.weight", (1024, 512, 1))
    small = MODELS["DGCNN_cls"](5, 7, k=4, emb_dims=32, channels=(8, 12, 16, 24), head=(16, 12))
    assert [(k, tuple(v.shape)) for k, v in small.state_dict().items()] == _expected_state(5, 7, 32, (8, 12, 16, 24), (16, 12))
    # torch's default initialisation for layers of those shapes: kaiming uniform with a = sqrt(5), i.e. U(+-1 / sqrt(fan_in))
    w = model.conv4[0].weight.detach()
    assert float(w.abs().max()) <= 1 / 256 ** 0.5 and abs(float(w.std()) * (3 * 256) ** 0.5 - 1) < 0.02
    assert bool((model.bn6.weight == 1).all()) and bool((model.bn6.bias == 0).all())
    assert model.knn_indices == []


def test_config_selects_the_model_after_modelnet40():
    from nerf_downstream_amd import gin_lite as gin
    from nerf_downstream_amd.co3d_3d.src.models import MODELS

    gin.clear_config()
    try:
        gin.parse_config_files_and_bindings([os.path.join(CONFIGS, "modelnet40_cls.gin"), os.path.join(CONFIGS, "dgcnn.gin")], [])
        q = gin.query_parameter
        assert MODELS[q("get_model.name")].__name__ == "DGCNN_cls"
        assert (q("get_model.in_channel"), q("get_model.out_channel"), q("DGCNN_cls.k")) == (3, 40, 20)
    finally:
        gin.clear_config()


def test_graph_entries_validate_arguments_without_a_gpu():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced: every check comes before the first launch
    err = lambda: L.mink_last_error()  # noqa: E731
    # kNN
    assert L.mink_knn(None, 100, 3, 3, P, 2, 20, P, None) == -1 and b"NULL" in err()
    assert L.mink_knn(P, 100, 3, 3, None, 2, 20, P, None) == -1 and b"NULL" in err()
    assert L.mink_knn(P, 100, 3, 3, P, 2, 20, None, None) == -1 and b"NULL" in err()
    assert L.mink_knn(P, 100, 3, 3, P, 2, 65, P, None) == -1 and b"k = 65" in err()
    assert L.mink_knn(P, 100, 3, 3, P, 2, 0, P, None) == -1 and b"k = 0" in err()
    assert L.mink_knn(P, 100, 257, 257, P, 2, 20, P, None) == -1 and b"C = 257" in err()
    assert L.mink_knn(P, 100, 2, 3, P, 2, 20, P, None) == -1 and b"ldx" in err()
    assert L.mink_knn(P, 1 << 26, 3, 3, P, 2, 64, P, None) == -1 and b"2^31" in err()
    # edge statistics: the partial rows are an argument with its size
    n, k, C = 260, 20, 64
    rows = L.mink_edge_stats_rows(n)
    assert 1 <= rows <= 256 and L.mink_edge_stats_rows(1 << 20) == 256 and L.mink_edge_stats_rows(1) == 1
    need = rows * 2 * C * 8
    assert L.mink_edge_stats(P, P, P, n, k, C, P, need - 1, None) == -1
    assert b"workspace" in err() and str(need).encode() in err()
    assert L.mink_edge_stats(None, P, P, n, k, C, P, need, None) == -1 and b"NULL" in err()
    assert L.mink_edge_stats(P, P, P, n, 65, C, P, need, None) == -1 and b"k 65" in err()
    # forward
    assert L.mink_edge_fwd(P, P, None, n, k, C, P, P, P, P, P, P, None) == -1 and b"NULL" in err()
    assert L.mink_edge_fwd(P, P, P, n, 65, C, P, P, P, P, P, P, None) == -1 and b"k 65" in err()
    assert L.mink_edge_fwd(P, P, P, n, k, 0, P, P, P, P, P, P, None) == -1 and b"bad shape" in err()
    # backward
    need = L.mink_edge_bwd_workspace_bytes(n, C)
    assert need >= n * C * 4 + rows * 2 * C * 8
    args = (P, P, P, P, P, n, k, C, P, P, P, P, 1, P, P, P, P, P, P)
    assert L.mink_edge_bwd(*args, P, need - 1, None) == -1
    assert b"workspace" in err() and str(need).encode() in err()
    assert L.mink_edge_bwd(*args, None, need, None) == -1 and b"NULL" in err()
    assert L.mink_edge_bwd(*args[:13], None, *args[14:], P, need, None) == -1 and b"NULL" in err()
    assert L.mink_edge_bwd(*args[:6], 65, *args[7:], P, need, None) == -1 and b"k 65" in err()


def test_restatement_reproduces_the_reference_neighbour_sets():
    g = np.load(os.path.join(ROOT, "tests", "golden", "dgcnn_knn_v1.npz"))
    x, k, sets = torch.from_numpy(g["x"]), int(g["k"]), g["sets"]
    B, N, C = x.shape
    assert (B, N, C, k) == (2, 40, 3, 20) and sets.shape == (B, N, k)
    assert bool((x * 8 == (x * 8).round()).all())  # the 1/8 lattice: every distance is exact
    off = [0, N, 2 * N]
    idx = DG.knn(x.reshape(B * N, C), off, k)
    for b in range(B):
        mine = np.sort((idx[b * N:(b + 1) * N] - b * N).numpy(), axis=1)
        assert np.array_equal(mine, sets[b].astype(np.int64)), b
    # ... in ascending distance, the row itself first, equal distances in ascending row order
    d = DG.sq_dists(x.reshape(B * N, C), 0, N)
    dd = d.gather(1, idx[:N])
    assert bool((dd.diff(dim=1) >= 0).all()) and idx[:N, 0].tolist() == list(range(N))
    assert bool(((dd.diff(dim=1) > 0) | (idx[:N].diff(dim=1) > 0)).all())
    assert DG.knn_valid(x.reshape(B * N, C), off, idx, k)
    with pytest.raises(ValueError, match="sample 1 holds only 10 points"):
        DG.knn(x.reshape(B * N, C)[:50], [0, 40, 50], k)


def test_knn_restatement_ties_and_validity_helper():
    x = torch.tensor([[0.0], [1.0], [1.0], [2.0], [-1.0], [5.0], [5.0], [5.0]])
    idx = DG.knn(x, [0, 5, 5, 8], 3)  # an empty sample in the middle
    assert idx[0].tolist() == [0, 1, 2] and idx[1].tolist() == [1, 2, 0] and idx[3].tolist() == [3, 1, 2]
    assert idx[5:].tolist() == [[5, 6, 7]] * 3  # identical points: the lower row first, not the row itself
    assert DG.knn_valid(x, [0, 5, 5, 8], idx, 3)
    bad = idx.clone()
    bad[0, 2] = 3  # distance 4 instead of 1
    assert not DG.knn_valid(x, [0, 5, 5, 8], bad, 3)
    bad = idx.clone()
    bad[0, 2] = 1  # repeated
    assert DG.knn_violations(x, [0, 5, 5, 8], bad, 3)[1] == 1
    bad = idx.clone()
    bad[6, 0] = 4  # another sample's row
    assert DG.knn_violations(x, [0, 5, 5, 8], bad, 3)[0] == 1


@pytest.mark.parametrize("training", [True, False])
def test_pq_form_and_explicit_backward_equal_autograd(training):
    """The form the kernels evaluate -- e = P[idx] + Q[i], and the backward through per-row sums over outgoing (dQ) and
    incoming (dP) edges -- against autograd of the plain restatement, in float64."""
    g = torch.Generator().manual_seed(11)
    n, cin, cout, k = 60, 5, 7, 6
    x = torch.randn(n, cin, generator=g, dtype=torch.float64)
    off = [0, 41, 60]
    idx = DG.knn(x, off, k)
    W = torch.randn(cout, 2 * cin, generator=g, dtype=torch.float64) * 0.4
    gamma, beta = torch.rand(cout, generator=g, dtype=torch.float64) + 0.5, torch.randn(cout, generator=g, dtype=torch.float64) * 0.3
    dy = torch.randn(n, cout, generator=g, dtype=torch.float64)
    stats = None if training else (torch.randn(cout, generator=g, dtype=torch.float64) * 0.2, torch.rand(cout, generator=g, dtype=torch.float64) + 0.5)
    leaves = [t.clone().requires_grad_(True) for t in (x, W, gamma, beta)]
    y, arg, (mean, var) = DG.edge_conv(*leaves, idx, stats)
    y.backward(dy)
    mean, var = mean.detach(), var.detach()
    W1, W2 = W[:, :cin], W[:, cin:]
    P, Q = x @ W1.t(), x @ (W2 - W1).t()
    e = P[idx] + Q[:, None, :]
    assert torch.allclose(e, DG.edges(x, W, idx), atol=1e-13)
    inv = 1 / torch.sqrt(var + DG.BN_EPS)
    xhat = (e - mean) * inv
    pick = lambda t: t.gather(1, arg[:, None, :])[:, 0, :]  # noqa: E731
    gg = dy * torch.where(gamma * pick(xhat) + beta > 0, torch.tensor(1.0, dtype=torch.float64), torch.tensor(0.2, dtype=torch.float64))
    dbeta, dgamma = gg.sum(0), (gg * pick(xhat)).sum(0)
    M = n * k
    t = 1.0 if training else 0.0
    onehot = torch.zeros(n, k, cout, dtype=torch.float64).scatter_(1, arg[:, None, :], 1.0)
    de = gamma * inv * (onehot * gg[:, None, :] - t * dbeta / M - t * xhat * dgamma / M)
    dQ = de.sum(1)
    dP = torch.zeros(n, cout, dtype=torch.float64).index_add_(0, idx.reshape(-1), de.reshape(-1, cout))
    dx = dP @ W1 + dQ @ (W2 - W1)
    dW = torch.cat([dP.t() @ x - dQ.t() @ x, dQ.t() @ x], 1)
    for got, ref in zip((dx, dW, dgamma, dbeta), (l.grad for l in leaves)):
        assert float((got - ref).abs().max()) < 1e-12
    # the bounds of the GPU test are finite, positive and far below the values they bound
    b = DG.edge_bounds(x, W, gamma, beta, idx, dy, stats)
    assert all(bool(torch.isfinite(v).all()) and bool((v >= 0).all()) for v in b.values())
    refs = dict(zip(("dx", "dW", "dgamma", "dbeta"), (l.grad for l in leaves)), y=y.detach())
    assert ("mean" in b) == training
    for name, v in ((k_, v_) for k_, v_ in b.items() if k_ in refs):  # worst-case bounds at n = 60: below a hundredth of the largest value
        assert float(v.max()) < 1e-2 * float(refs[name].abs().max()), (name, float(v.max()), float(refs[name].abs().max()))
    assert b["dW"].shape == W.shape and b["dx"].shape == x.shape


def test_running_statistics_restatement_matches_torch():
    g = torch.Generator().manual_seed(2)
    v = torch.randn(50, 4, generator=g, dtype=torch.float64)
    bn = torch.nn.BatchNorm1d(4).double().train()
    bn(v)
    rm, rv = DG.running_update(torch.zeros(4, dtype=torch.float64), torch.ones(4, dtype=torch.float64), v.mean(0),
                               ((v - v.mean(0)) ** 2).mean(0), 50)
    assert torch.allclose(rm, bn.running_mean, atol=1e-14) and torch.allclose(rv, bn.running_var, atol=1e-14)
