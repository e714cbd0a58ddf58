"""-m gpu: the dynamic graph layers (csrc/graph.hip, minkowski/graph.py) and DGCNN_cls against the float64 restatement of
tests/dgcnn_restate.py, on the sample sizes of the shared two-clouds case (193 + 67 rows: a 32-row query tile and a 128-row
candidate tile end inside a sample, and the sample boundary falls inside a tile).  Every bound is derived from the number
format and the restatement's own terms (dgcnn_restate.edge_bounds, knn_tau); the whole-network criteria are those of
tests/test_gpu_point.py."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dgcnn_restate as DG
import point_restate as PT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = [0, 193, 260]


@functools.lru_cache(None)
def _case():
    return PT.two_clouds()


def _boff(off):
    return torch.tensor(off, dtype=torch.int32).cuda()


def _randn(n, C, seed):
    return torch.randn(n, C, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ 1. kNN, exact
@pytest.mark.parametrize("k", [1, 5, 20, 64])
@pytest.mark.parametrize("C", [3, 12, 64, 128])
def test_knn_exact_on_integer_lattice(C, k):
    """Integer features with |x| <= 8: every product, norm and sum is an integer below 2^24 (at most 128 * 16^2 = 32,768), so
    the fp32 score is exact in expanded and direct form alike and the table must equal the restatement's element for element:
    ascending distance, equal distances in ascending row order.  Samples: 193 rows with a cluster of 25 identical rows, an
    empty sample, a sample of exactly k rows, 67 rows."""
    from nerf_downstream_amd.minkowski import graph as G

    off = [0, 193, 193, 193 + k, 260 + k]
    g = torch.Generator().manual_seed(100 * C + k)
    x = torch.randint(-8, 9, (off[-1], C), generator=g).float()
    x[30:55] = x[30]
    ref = DG.knn(x, off, k)
    idx = G.knn(x.cuda(), _boff(off), k)
    assert idx.dtype == torch.int32 and idx.shape == (off[-1], k)
    got = idx.cpu().long()
    sample = torch.repeat_interleave(torch.arange(4), torch.tensor(off).diff())
    assert bool((sample[got.clamp(0, off[-1] - 1)] == sample[:, None]).all()) and int(got.min()) >= 0  # no index leaves its sample
    assert torch.equal(got, ref), (C, k, int((got != ref).sum()))
    indeg = torch.bincount(ref.reshape(-1), minlength=off[-1])
    if k < 25:
        assert int(indeg[30:55].min()) == 0  # the cluster's later rows are never chosen: rows of in-degree 0
    assert torch.equal(got[193:193 + k].sort(1).values, torch.arange(193, 193 + k).expand(k, k))  # the sample of exactly k rows


# ------------------------------------------------------------------------------------------------ 2. kNN, validity
@pytest.mark.parametrize("C", [3, 12, 64, 128])
def test_knn_validity_on_normal_data(C):
    """Normal features: the table need not equal the float64 one where two distances differ by less than the fp32 error, but
    with d64 the float64 distances and d_(k) the k-th smallest of row i, every chosen j has d64 <= d_(k) + tau_i, every
    unchosen j of the sample has d64 >= d_(k) - tau_i, and the indices of a row are distinct.

    tau_i for the expanded form the kernel ranks by, s_ij = fl(n_j - 2 p_ij) with n_j = ||x_j||^2 and p_ij = x_i . x_j each a
    chain of C fused multiply-adds (u = 2^-24, gamma_C = C u / (1 - C u)):
        |n^_j - n_j| <= gamma_C ||x_j||^2,   |p^_ij - p_ij| <= gamma_C sum_c |x_ic x_jc| <= gamma_C ||x_i|| ||x_j||,
        the last fused multiply-add rounds once more: u |n_j - 2 p_ij| (1 + gamma_C),
    so |s^_ij - s_ij| <= (gamma_C + u (1 + gamma_C)) (||x_j||^2 + 2 ||x_i|| ||x_j||) <= (C + 2) u (||x_i|| + max_j ||x_j||)^2 =: e_i
    for C <= 256.  s_ij + ||x_i||^2 is the distance, and the row's constant does not change its ranking.  If a chosen j had
    d_j > d_(k) + 2 e_i, some unchosen j' has d_j' <= d_(k) (k rows do, and not all of them were chosen), yet ranked behind j:
    s^_j <= s^_j', i.e. d_j - e_i <= d_j' + e_i, a contradiction; the unchosen side is symmetric.  tau_i = 2 e_i."""
    from nerf_downstream_amd.minkowski import graph as G

    k = 20
    x = _randn(260, C, 7 + C)
    idx = G.knn(x.cuda(), _boff(OFF), k).cpu()
    outside, repeated, worst_in, worst_out = DG.knn_violations(x, OFF, idx, k)
    agree = float((idx.long() == DG.knn(x, OFF, k)).float().mean())
    print(f"[dgcnn] knn C={C}: {agree:.4f} of the slots equal the float64 table; chosen over by {worst_in:.3e}, unchosen under by "
          f"{worst_out:.3e} (both <= 0 required; tau_0 = {float(DG.knn_tau(x, 0, 193)[0]):.3e})")
    assert outside == 0 and repeated == 0
    assert worst_in <= 0 and worst_out <= 0


# ------------------------------------------------------------------------------------------------ 3. edge convolution
def _edge_inputs(cin, cout, k):
    seed = 1000 * cin + 10 * cout + k
    x = _randn(260, cin, seed)
    W = _randn(cout, 2 * cin, seed + 1) * (0.7 / (2 * cin) ** 0.5)
    gamma = torch.rand(cout, generator=torch.Generator().manual_seed(seed + 2)) + 0.5
    beta = _randn(1, cout, seed + 3)[0] * 0.3
    rm = _randn(1, cout, seed + 4)[0] * 0.2
    rv = torch.rand(cout, generator=torch.Generator().manual_seed(seed + 5)) + 0.5
    dy = _randn(260, cout, seed + 6)
    idx = DG.knn(x, OFF, k)
    return x, W, gamma, beta, rm, rv, dy, idx


def _run_edge(x, W, gamma, beta, rm, rv, dy, idx, training):
    from nerf_downstream_amd.minkowski import graph as G

    leaves = [t.clone().cuda().requires_grad_(True) for t in (x, W.reshape(W.shape[0], -1, 1, 1), gamma, beta)]
    rmc, rvc = rm.clone().cuda(), rv.clone().cuda()
    y, arg = G.EdgeConvFunction.apply(*leaves, rmc, rvc, idx.int().cuda(), training, 0.1, DG.BN_EPS)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "arg": arg.cpu(), "dx": leaves[0].grad.cpu(), "dW": leaves[1].grad.cpu().reshape(W.shape),
            "dgamma": leaves[2].grad.cpu(), "dbeta": leaves[3].grad.cpu(), "rm": rmc.cpu(), "rv": rvc.cpu()}


@pytest.mark.parametrize("k", [1, 5, 20])
@pytest.mark.parametrize("cout", [12, 64])
@pytest.mark.parametrize("cin", [3, 8, 64])
def test_edge_conv_forward_and_backward(cin, cout, k):
    """One edge layer under the restatement's neighbour table, train and eval mode: the arg slots equal the restatement's
    (normal inputs: a tie of the maximum has probability zero), y / dx / dW / dgamma / dbeta lie within the first-order fp32
    bounds of dgcnn_restate.edge_bounds, the running statistics move with the count n k and the unbiased variance, and a second
    run gives the same bits."""
    x, W, gamma, beta, rm, rv, dy, idx = _edge_inputs(cin, cout, k)
    n, M = x.shape[0], x.shape[0] * k
    for training in (True, False):
        stats = None if training else (rm.double(), rv.double())
        leaves = [t.double().requires_grad_(True) for t in (x, W, gamma, beta)]
        ry, rarg, (mean, var) = DG.edge_conv(*leaves, idx, stats)
        ry.backward(dy.double())
        ref = {"y": ry.detach(), "dx": leaves[0].grad, "dW": leaves[1].grad, "dgamma": leaves[2].grad, "dbeta": leaves[3].grad}
        bounds = DG.edge_bounds(x, W, gamma, beta, idx, dy, stats)
        got = _run_edge(x, W, gamma, beta, rm, rv, dy, idx, training)
        assert got["arg"].dtype == torch.uint8 and torch.equal(got["arg"].long(), rarg), int((got["arg"].long() != rarg).sum())
        for name in ("y", "dx", "dW", "dgamma", "dbeta"):
            err = (got[name].double() - ref[name]).abs()
            ratio = float((err / bounds[name].clamp_min(1e-300)).max())
            print(f"[dgcnn] edge cin={cin} cout={cout} k={k} {'train' if training else 'eval'} {name}: max err {float(err.max()):.3e}, "
                  f"largest bound {float(bounds[name].max()):.3e}, max err / bound {ratio:.3f}")
            assert bool((err <= bounds[name]).all()), (name, training, float(err.max()), ratio)
        if training:
            mean, var = mean.detach(), var.detach()
            want_rm, want_rv = DG.running_update(rm.double(), rv.double(), mean, var, M)
            tol_rm = 0.1 * bounds["mean"] + 3 * DG.U32 * (rm.double().abs() + mean.abs())
            tol_rv = 0.1 * bounds["var"] * M / max(M - 1, 1) + 3 * DG.U32 * (rv.double() + var * 2)
            assert bool(((got["rm"].double() - want_rm).abs() <= tol_rm).all())
            assert bool(((got["rv"].double() - want_rv).abs() <= tol_rv).all())
            # the count is n k, not n: with the per-point count the unbiased factor would differ by 1 / (n - 1) - 1 / (n k - 1)
            if k > 1:
                wrong = DG.running_update(rm.double(), rv.double(), mean, var, n)[1]
                assert bool(((wrong - want_rv).abs() > 4 * tol_rv).any())
        else:
            assert torch.equal(got["rm"], rm) and torch.equal(got["rv"], rv)
        again = _run_edge(x, W, gamma, beta, rm, rv, dy, idx, training)
        for name in got:
            assert torch.equal(got[name], again[name]), (name, training)


# ------------------------------------------------------------------------------------------------ 4. no edge-sized tensor
def test_edge_layer_allocates_no_edge_sized_tensor():
    """n = 4,096 rows (two samples of 2,048), Cin 64 -> Cout 128, k = 20: across forward + backward of one edge layer the peak
    of torch's allocator rises by less than ONE edge tensor, n k Cout 4 bytes = 41.9 MB (the reference's composition holds the
    [B, 2 Cin, N, k] graph feature and the [B, Cout, N, k] output, and their gradients).  What the design needs -- P, Q, y, dP, dQ,
    g (n Cout floats each), arg, dx, the incoming-edge lists and their sort -- adds up to well under half of that.  A small
    layer runs first, so that the GEMM library's one-off workspace is not counted as the layer's."""
    from nerf_downstream_amd.minkowski import graph as G

    def layer(n_half, cin, cout, k, seed):
        x = _randn(2 * n_half, cin, seed).cuda().requires_grad_(True)
        W = (_randn(cout, 2 * cin, seed + 1) * 0.1).cuda().requires_grad_(True)
        gamma, beta = torch.ones(cout).cuda().requires_grad_(True), torch.zeros(cout).cuda().requires_grad_(True)
        rm, rv = torch.zeros(cout).cuda(), torch.ones(cout).cuda()
        idx = G.knn(x, _boff([0, n_half, 2 * n_half]), k)
        dy = _randn(2 * n_half, cout, seed + 2).cuda()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y, _ = G.EdgeConvFunction.apply(x, W, gamma, beta, rm, rv, idx, True, 0.1, 1e-5)
        y.backward(dy)
        torch.cuda.synchronize()
        assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (x, W, gamma, beta))
        return torch.cuda.max_memory_allocated() - base

    layer(64, 64, 128, 20, 1)
    n, cout, k = 4096, 128, 20
    rise = layer(n // 2, 64, cout, k, 2)
    edge = n * k * cout * 4
    print(f"[dgcnn] peak rise of one edge layer (n {n}, 64 -> {cout}, k {k}): {rise / 1e6:.1f} MB; one edge tensor {edge / 1e6:.1f} MB")
    assert rise < edge, (rise, edge)


# ------------------------------------------------------------------------------------------------ 5. the whole network
def _build():
    from nerf_downstream_amd.co3d_3d.src.models import MODELS

    torch.manual_seed(3)
    net = MODELS["DGCNN_cls"](3, 5, k=20, emb_dims=32, dropout=0.0, channels=(8, 12, 16, 24), head=(16, 12))
    return net.cuda().train()


def test_network_matches_float64_restatement():
    coords, feats = _case()
    net = _build()
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.named_parameters()}
    wts = _randn(2, 5, 9)
    out = net(net.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
    tables = [t.cpu() for t in net.knn_indices]
    assert len(tables) == 4 and all(t.dtype == torch.int32 and t.shape == (260, 20) for t in tables)
    ref, _, inputs = DG.dgcnn_forward(params, feats, OFF, 20, forced_idx=tables)  # under the HIP run's neighbour tables
    assert out.shape == (2, 5) == ref.shape
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    print(f"[dgcnn] DGCNN_cls: logits max |err| {err:.3e}")
    assert err <= 1e-3, err
    for i, (table, x64) in enumerate(zip(tables, inputs)):  # each table is a valid kNN of the restatement's own layer input
        v = DG.knn_violations(x64, OFF, table, 20)
        print(f"[dgcnn] layer {i + 1} table: outside {v[0]}, repeated {v[1]}, chosen over by {v[2]:.3e}, unchosen under by {v[3]:.3e}")
        assert v[0] == 0 and v[1] == 0 and v[2] <= 0 and v[3] <= 0, (i, v)
    (out * wts.cuda()).sum().backward()
    (ref * wts.double()).sum().backward()
    hp = dict(net.named_parameters())
    assert all(p.grad is not None for p in hp.values())
    rel = {k: float((hp[k].grad.cpu().double() - params[k].grad).norm() / params[k].grad.norm().clamp_min(1e-12)) for k in hp}
    errs = sorted(rel.values())
    print(f"[dgcnn] DGCNN_cls: parameter-gradient relative error median {errs[len(errs) // 2]:.3e}, max {errs[-1]:.3e} "
          f"({max(rel, key=rel.get)})")
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
    # swapping the two samples of the batch swaps the logit rows
    order = torch.cat([torch.arange(193, 260), torch.arange(0, 193)])
    swapped = coords[order].clone()
    swapped[:, 0] = 1.0 - swapped[:, 0]
    with torch.no_grad():
        out2 = net(net.process_input({"coordinates": swapped.cuda(), "features": feats[order].cuda()}))
    assert torch.allclose(out2.flip(0), out.detach(), atol=1e-5), float((out2.flip(0) - out.detach()).abs().max())
    # a sample with fewer points than k is refused by name
    short = torch.cat([coords[:193], coords[193:203]])
    with pytest.raises(ValueError, match="sample 1 holds only 10 points"):
        net(net.process_input({"coordinates": short.cuda(), "features": feats[:203].cuda()}))


# ------------------------------------------------------------------------------------------------ 6. the trainer CLI
def _train_cli(tmp_path, data_root, tag):
    cfg = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "nerf_downstream_amd.co3d_3d.train", "--ginc", os.path.join(cfg, "modelnet40_cls.gin"),
           "--ginc", os.path.join(cfg, "dgcnn.gin"), "--save_path", str(tmp_path / tag),
           "--ginb", f"ModelNet40H5Dataset.data_root='{data_root}'", "--ginb", "train.batch_size=4", "--ginb", "train.val_batch_size=4",
           "--ginb", "train.max_steps=3", "--ginb", "train.loggers=[]", "--ginb", "train.log_every_n_steps=1",
           "--ginb", "train.train_num_workers=0", "--ginb", "train.val_num_workers=0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    losses = re.findall(r"step \d+: train/loss=(\S+)", r.stdout)
    assert len(losses) == 3, r.stdout[-3000:]
    return losses


def test_trainer_cli_runs_dgcnn(tmp_path):
    """Three optimiser steps of modelnet40_cls.gin + dgcnn.gin on 256-point .npz shards with batch 4, in a fresh process: finite,
    distinct losses, and a second run prints the same three strings (fixed-order sums everywhere in the new kernels)."""
    root = tmp_path / "shards"
    root.mkdir()
    rng = np.random.default_rng(4)
    for phase, m in (("train", 32), ("test", 8)):
        np.savez(root / f"ply_data_{phase}0.npz", data=rng.uniform(-1, 1, size=(m, 256, 3)).astype(np.float32),
                 label=rng.integers(0, 40, size=(m, 1)).astype(np.int64))
    first = _train_cli(tmp_path, str(root), "first")
    vals = [float(v) for v in first]
    assert all(np.isfinite(vals)) and len(set(first)) == 3, first
    second = _train_cli(tmp_path, str(root), "second")
    assert first == second, (first, second)
