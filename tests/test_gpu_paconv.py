"""-m gpu: PAConv (csrc/paconv.hip, minkowski/paconv.py), ScoreNet and the two PAConv classifiers against the float64
restatement of tests/paconv_restate.py, on the sample sizes of the shared two-clouds case (193 + 67 rows).  The op is exact on
a lattice, within the restatement's running-error bounds on normal data, bitwise reproducible, and forms nothing of the size
of the reference's transformed or gathered tensors; the whole-network criteria are those of tests/test_gpu_dgcnn.py."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import dgcnn_restate as DG
import paconv_restate as PA
import point_restate as PT

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFF = [0, 193, 260]
N = OFF[-1]
NAMES = ("y", "ds", "dx", "dm")


def _gen(seed):
    return torch.Generator().manual_seed(seed)


@functools.lru_cache(None)
def _lattice_table(k):
    """The restatement's kNN of 260 integer points, rows 30..54 identical: row 30 is a hub of large in-degree, and for k < 25
    the cluster's last rows are chosen by nobody (equal distances go to the lower row)."""
    pts = torch.randint(-8, 9, (N, 3), generator=_gen(77)).float()
    pts[30:55] = pts[30]
    return DG.knn(pts, OFF, k)


def _run(x, matrice, s, idx, mode, dy):
    from nerf_downstream_amd.minkowski import paconv as P

    leaves = [t.clone().cuda().requires_grad_(True) for t in (x, matrice, s)]
    y = P.paconv(*leaves, idx.int().cuda(), mode)
    y.backward(dy.cuda())
    torch.cuda.synchronize()
    return {"y": y.detach().cpu(), "dx": leaves[0].grad.cpu(), "dm": leaves[1].grad.cpu(), "ds": leaves[2].grad.cpu()}


# ------------------------------------------------------------------------------------------------ 1. exact on a lattice
LATTICE = [  # (Cin, M, k, O, mode, with a -1 slot)
    (3, 1, 1, 4, "dgcnn", False), (3, 8, 20, 64, "dgcnn", False), (3, 3, 5, 4, "pointnet", False),
    (6, 3, 5, 4, "pointnet", False), (6, 16, 20, 4, "dgcnn", False), (6, 8, 1, 64, "pointnet", False),
    (64, 8, 20, 64, "pointnet", False), (64, 16, 5, 4, "dgcnn", False), (64, 1, 5, 64, "pointnet", False), (64, 8, 5, 64, "dgcnn", True),
    (128, 8, 20, 64, "dgcnn", False), (128, 3, 1, 64, "pointnet", False), (128, 16, 20, 64, "pointnet", False), (128, 1, 20, 4, "dgcnn", False),
]


@pytest.mark.parametrize("cin,M,k,O,mode,hole", LATTICE)
def test_exact_on_a_lattice(cin, M, k, O, mode, hole):
    """x integers with |x| <= 4, scores multiples of 1/4 in [0, 1], matrice and dy integers with |.| <= 2: every product is a
    multiple of 1/4, and once the largest absolute-value sum behind any output stays below 2^24 quarter units (asserted first,
    from the restatement's own sums) every partial sum of every evaluation order is exact in fp32.  y, ds, dx and d matrice must
    then equal the float64 restatement element for element.  The table has a hub (rows 30..54 coincide) and, for k < 25, rows
    nobody chooses; `hole`: one slot is -1, contributes nothing, and its ds is 0."""
    g = _gen(1000 * cin + 100 * M + 10 * k + O)
    x = torch.randint(-4, 5, (N, cin), generator=g).float()
    s = torch.randint(0, 5, (N, k, M), generator=g).float() / 4
    matrice = torch.randint(-2, 3, (2 * cin if mode == "dgcnn" else cin, M * O), generator=g).float()
    dy = torch.randint(-2, 3, (N, O), generator=g).float()
    idx = _lattice_table(k).clone()
    indeg = torch.bincount(idx.reshape(-1), minlength=N)
    assert int(indeg[30]) >= 25 and (k >= 25 or int(indeg[30:55].min()) == 0)
    if hole:
        idx[7, 2] = -1
    worst = PA.lattice_partial_sum_bound(x, matrice, s, idx, mode, dy)
    assert worst < 2.0 ** 24 / 4, worst
    ref = PA.paconv_grads(x, matrice, s, idx, mode, dy)
    got = _run(x, matrice, s, idx, mode, dy)
    for name in NAMES:
        assert got[name].dtype == torch.float32 and got[name].shape == ref[name].shape
        assert torch.equal(got[name].double(), ref[name]), (name, int((got[name].double() != ref[name]).sum()),
                                                            float((got[name].double() - ref[name]).abs().max()))
    if hole:
        assert float(got["ds"][7, 2].abs().max()) == 0.0
        closed = idx.clone()
        closed[7, 2] = 7  # the same table with the slot filled changes row 7's output and the target's dx
        other = PA.paconv_grads(x, matrice, s, closed, mode, dy)
        assert not torch.equal(other["y"][7], ref["y"][7])


# ------------------------------------------------------------------------------------------------ 2. normal data
def _normal_case(cin, M, k, O, mode):
    seed = 2000 * cin + 100 * M + 10 * k + O
    g = _gen(seed)
    x = torch.randn(N, cin, generator=g)
    s = torch.softmax(torch.randn(N, k, M, generator=g), 2) + (0.5 if mode == "dgcnn" else 0.0)
    rows = 2 * cin if mode == "dgcnn" else cin
    matrice = torch.randn(rows, M * O, generator=g) * (2.0 / (rows * O)) ** 0.5
    dy = torch.randn(N, O, generator=g)
    idx = DG.knn(torch.randn(N, 3, generator=g), OFF, k)
    return x, matrice, s, idx, dy


@pytest.mark.parametrize("cin,M,k,O,mode", [(3, 8, 20, 64, "dgcnn"), (6, 3, 5, 4, "pointnet"), (64, 8, 20, 64, "pointnet"),
                                            (64, 16, 5, 12, "dgcnn"), (128, 8, 20, 64, "dgcnn"), (128, 1, 1, 64, "pointnet")])
def test_normal_data_within_running_error_bounds(cin, M, k, O, mode):
    """Normal features and weights, softmax scores (plus the DGCNN variant's 0.5): forward and the three gradients lie within
    the first-order fp32 bounds of paconv_restate.paconv_bounds -- L u times the restatement's absolute-value sums."""
    x, matrice, s, idx, dy = _normal_case(cin, M, k, O, mode)
    ref = PA.paconv_grads(x, matrice, s, idx, mode, dy)
    bounds = PA.paconv_bounds(x, matrice, s, idx, mode, dy)
    got = _run(x, matrice, s, idx, mode, dy)
    for name in NAMES:
        err = (got[name].double() - ref[name]).abs()
        ratio = float((err / bounds[name].clamp_min(1e-300)).max())
        print(f"[paconv] {mode} cin={cin} M={M} k={k} O={O} {name}: max err {float(err.max()):.3e}, largest bound "
              f"{float(bounds[name].max()):.3e}, max err / bound {ratio:.4f}")
        assert bool((err <= bounds[name]).all()), (name, float(err.max()), ratio)


# ------------------------------------------------------------------------------------------------ 3. reproducibility
@pytest.mark.parametrize("cin,M,k,O,mode", [(3, 8, 20, 64, "dgcnn"), (64, 8, 20, 64, "pointnet"), (128, 16, 5, 12, "dgcnn")])
def test_two_runs_give_the_same_bits(cin, M, k, O, mode):
    x, matrice, s, idx, dy = _normal_case(cin, M, k, O, mode)
    idx = _lattice_table(k)  # the hub: the longest incoming list
    first = _run(x, matrice, s, idx, mode, dy)
    second = _run(x, matrice, s, idx, mode, dy)
    for name in NAMES:
        assert torch.equal(first[name], second[name]), name


# ------------------------------------------------------------------------------------------------ 4. memory
def test_layer_allocates_no_transformed_or_gathered_tensor():
    """n = 4,096 rows (two samples of 2,048), Cin 64, M 8, O 128, k 20: across forward + backward of one layer the peak of
    torch's allocator rises by less than one transformed tensor plus its gathered form, (n M O + n k O) 4 bytes = 58.7 MB --
    the reference's composition holds two transformed tensors, and their gradients.  What the design needs: [A | S x] and its
    gradient (2 n M Cin floats each), the incoming-edge lists and their sort, y, S, ds, dx and the bank's two forms.  A small
    layer runs first, so that the GEMM library's one-off workspace is not counted as the layer's."""
    from nerf_downstream_amd.minkowski import graph as G
    from nerf_downstream_amd.minkowski import paconv as P

    def layer(n_half, cin, M, O, k, seed):
        g = _gen(seed)
        x = torch.randn(2 * n_half, cin, generator=g).cuda().requires_grad_(True)
        matrice = (torch.randn(2 * cin, M * O, generator=g) * 0.05).cuda().requires_grad_(True)
        s = torch.softmax(torch.randn(2 * n_half, k, M, generator=g), 2).cuda().requires_grad_(True)
        idx = G.knn(torch.randn(2 * n_half, 3, generator=g).cuda(), torch.tensor([0, n_half, 2 * n_half], dtype=torch.int32).cuda(), k)
        dy = torch.randn(2 * n_half, O, generator=g).cuda()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = P.paconv(x, matrice, s, idx, "dgcnn")
        y.backward(dy)
        torch.cuda.synchronize()
        assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (x, matrice, s))
        return torch.cuda.max_memory_allocated() - base

    layer(64, 64, 8, 128, 20, 1)
    n, M, O, k = 4096, 8, 128, 20
    rise = layer(n // 2, 64, M, O, k, 2)
    limit = (n * M * O + n * k * O) * 4
    print(f"[paconv] peak rise of one layer (n {n}, Cin 64, M {M}, O {O}, k {k}): {rise / 1e6:.1f} MB; one transformed tensor plus its "
          f"gathered form {limit / 1e6:.1f} MB")
    assert rise < limit, (rise, limit)


# ------------------------------------------------------------------------------------------------ 5. the whole networks
NETS = {"PAConvPointNet": (dict(channels=(8, 12, 16, 24), emb_dims=32, head=16, num_matrices=(2, 3, 4)), PA.pointnet_forward),
        "PAConvDGCNN": (dict(channels=(8, 12, 16, 24), emb_dims=32, head=(16, 12), num_matrices=(1, 2, 3, 4)), PA.dgcnn_forward)}


@pytest.mark.parametrize("name", list(NETS))
def test_network_matches_float64_restatement(name):
    from nerf_downstream_amd.co3d_3d.src.models import MODELS

    coords, feats = PT.two_clouds()
    kw, restate = NETS[name]
    torch.manual_seed(3)
    net = MODELS[name](3, 5, k=20, dropout=0.0, **kw).cuda().train()
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.named_parameters()}
    wts = torch.randn(2, 5, generator=_gen(9))
    out = net(net.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
    assert len(net.knn_indices) == 1
    table = net.knn_indices[0].cpu()
    assert table.dtype == torch.int32 and table.shape == (N, 20)
    v = DG.knn_violations(feats, OFF, table, 20)  # a valid kNN of the xyz, one table for every layer
    print(f"[paconv] {name} table: outside {v[0]}, repeated {v[1]}, chosen over by {v[2]:.3e}, unchosen under by {v[3]:.3e}")
    assert v[0] == 0 and v[1] == 0 and v[2] <= 0 and v[3] <= 0, v
    ref, _ = restate(params, feats, OFF, 20, idx=table)  # under the HIP run's neighbour table
    assert out.shape == (2, 5) == ref.shape
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    print(f"[paconv] {name}: logits max |err| {err:.3e}")
    assert err <= 1e-3, err
    (out * wts.cuda()).sum().backward()
    (ref * wts.double()).sum().backward()
    hp = dict(net.named_parameters())
    unused = sorted(k for k in hp if params[k].grad is None)  # ScoreNet's batch norm after the output layer (last_bn = False)
    assert unused == sorted(k for k in hp if hp[k].grad is None) and all(".mlp_bns_hidden.1." in k for k in unused)
    rel = {k: float((hp[k].grad.cpu().double() - params[k].grad).norm() / params[k].grad.norm().clamp_min(1e-12)) for k in hp if k not in unused}
    errs = sorted(rel.values())
    print(f"[paconv] {name}: parameter-gradient relative error median {errs[len(errs) // 2]:.3e}, max {errs[-1]:.3e} ({max(rel, key=rel.get)})")
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
def _train_cli(tmp_path, data_root, config, tag):
    cfg = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs")
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "nerf_downstream_amd.co3d_3d.train", "--ginc", os.path.join(cfg, "modelnet40_cls.gin"),
           "--ginc", os.path.join(cfg, config), "--save_path", str(tmp_path / tag),
           "--ginb", f"ModelNet40H5Dataset.data_root='{data_root}'", "--ginb", "train.batch_size=4", "--ginb", "train.val_batch_size=4",
           "--ginb", "train.max_steps=3", "--ginb", "train.loggers=[]", "--ginb", "train.log_every_n_steps=1",
           "--ginb", "train.train_num_workers=0", "--ginb", "train.val_num_workers=0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    losses = re.findall(r"step \d+: train/loss=(\S+)", r.stdout)
    assert len(losses) == 3, r.stdout[-3000:]
    return losses


@pytest.mark.parametrize("config", ["paconv_pointnet.gin", "paconv_dgcnn.gin"])
def test_trainer_cli_runs_paconv(tmp_path, config):
    """Three optimiser steps of modelnet40_cls.gin + the model's config on 256-point .npz shards with batch 4, in a fresh
    process: finite, distinct losses, and a second run prints the same three strings (fixed-order sums in the new kernels)."""
    root = tmp_path / "shards"
    root.mkdir()
    rng = np.random.default_rng(4)
    for phase, m in (("train", 32), ("test", 8)):
        np.savez(root / f"ply_data_{phase}0.npz", data=rng.uniform(-1, 1, size=(m, 256, 3)).astype(np.float32),
                 label=rng.integers(0, 40, size=(m, 1)).astype(np.int64))
    first = _train_cli(tmp_path, str(root), config, "first")
    vals = [float(v) for v in first]
    assert all(np.isfinite(vals)) and len(set(first)) == 3, first
    second = _train_cli(tmp_path, str(root), config, "second")
    assert first == second, (first, second)
