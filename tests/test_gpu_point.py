"""-m gpu: the point stage of the point-based classifiers (csrc/field.hip and the TensorField side of minkowski/) and the three
networks built on it, against the float64 restatement of tests/point_restate.py on the shared two-clouds case (2 samples of
193 and 67 points with duplicate voxels, a point on a cell boundary and one at x = -0.25).  Every bound is derived from the
restatement's own terms or from the number format; the whole-network criteria are those of tests/test_gpu_unet.py."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import point_restate as PT
import pool_restate as PR
from helpers import misaligned

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = PT.EPS32
TINY = 2.0 ** -149
STRIDES = (1, 2, 8, 128)


@functools.lru_cache(None)
def _case():
    return PT.two_clouds()


def _field(feats=None):
    """A fresh TensorField of the two clouds with its levels up to tensor stride 128."""
    from nerf_downstream_amd import minkowski as ME

    coords, f = _case()
    tf = ME.TensorField(coordinates=coords.cuda(), features=(f if feats is None else feats).cuda())
    m, key = tf.coordinate_manager, ME.CoordinateMapKey(1)
    while key.get_tensor_stride()[0] < 128:
        key = m.stride(key, 2)
    return ME, tf, m


def _randn(n, C, seed):
    return torch.randn(n, C, generator=torch.Generator().manual_seed(seed))


# ------------------------------------------------------------------------------------------------ 1. field map
def test_field_map_equals_restatement():
    ME, tf, m = _field()
    coords = _case()[0]
    vox1, _ = PT.quantise(coords)
    assert vox1.shape[0] < coords.shape[0]
    for ts in (1, 2, 4, 8, 16, 32, 64, 128):
        assert int(torch.bincount(PT.level(coords, ts)[:, 0], minlength=2).min()) >= 2
    for ts in STRIDES:
        key = ME.CoordinateMapKey(ts)
        vox = m.get_coordinates(key).cpu().long()
        assert sorted(map(tuple, vox.tolist())) == sorted(map(tuple, PT.level(coords, ts).tolist())), ts
        idx, csr_fn = m.field_map(key, tf.C)
        assert idx.dtype == torch.int32 and torch.equal(idx.cpu().long(), PT.field_map(coords, vox, ts)), ts
        assert m.field_map(key, tf.C)[0] is idx  # kept on the manager
        members, seg = csr_fn()
        members, seg = members.cpu().long(), seg.cpu().long()
        assert seg[0] == 0 and seg[-1] == coords.shape[0] and torch.equal(idx.cpu().long()[members], torch.repeat_interleave(torch.arange(vox.shape[0]), seg.diff()))
        assert all(bool((members[seg[u]:seg[u + 1]].diff() > 0).all()) for u in range(vox.shape[0]))  # ascending row order
    # a batch index without voxels finds nothing; a voxel that is not there neither
    q = torch.cat([coords[:5], torch.tensor([[7.0, 1.0, 1.0, 1.0], [0.0, 30000.5, 0.0, 0.0]])]).cuda()
    idx, _ = m.field_map(ME.CoordinateMapKey(8), q)
    vox8 = m.get_coordinates(ME.CoordinateMapKey(8)).cpu().long()
    assert idx.cpu().tolist()[5:] == [-1, -1] and torch.equal(idx.cpu().long(), PT.field_map(q.cpu(), vox8, 8))
    for bad in ([0.0, float("nan"), 0.0, 0.0], [0.0, 0.0, float("inf"), 0.0], [0.0, 0.0, 0.0, 40000.0], [float("nan"), 0.0, 0.0, 0.0],
                [0.0, -1e9, 0.0, 0.0]):
        q = torch.cat([coords[:70], torch.tensor([bad])]).cuda()
        with pytest.raises(ValueError, match="outside the supported range"):
            m.field_map(ME.CoordinateMapKey(2), q)


# ------------------------------------------------------------------------------------------------ 2. strided slice
@pytest.mark.parametrize("C", [3, 8])
def test_strided_slice_forward_and_backward(C):
    ME, tf, m = _field()
    coords = _case()[0]
    for ts in STRIDES[1:]:
        key = ME.CoordinateMapKey(ts)
        n = m.get_coordinates(key).shape[0]
        idx = m.field_map(key, tf.C)[0].cpu().long()
        x, dy = _randn(n, C, 10 * ts + C), _randn(coords.shape[0], C, 20 * ts + C)
        grads = []
        for _ in range(2):
            leaf = x.clone().cuda().requires_grad_(True)
            out = ME.SparseTensor(leaf, key, m).slice(tf)
            assert isinstance(out, ME.TensorField) and out.coordinate_manager is m and out.C is tf.C
            assert torch.equal(out.F.detach().cpu(), x[idx]), ts  # bitwise F[idx]
            out.F.backward(dy.cuda())
            grads.append(leaf.grad.cpu())
        assert torch.equal(grads[0], grads[1]), ts  # fixed summation order
        ref = PT.gather_bwd(dy, idx, n)
        absum, longest = PT.gather_bwd_abs(dy, idx, n)
        err, bound = (grads[0].double() - ref).abs(), longest * EPS * absum
        print(f"[point] slice ts={ts} C={C}: longest segment {longest}, max err / bound "
              f"{float((err[bound > 0] / bound[bound > 0]).max()):.3f}")
        assert bool((err <= bound).all()), (ts, float(err.max()))
    with pytest.raises(ValueError, match="slice"):  # a tensor on another manager is still refused
        ME2, tf2, m2 = _field()
        ME.SparseTensor(torch.zeros(m2.get_coordinates(ME.CoordinateMapKey(2)).shape[0], C).cuda(), ME.CoordinateMapKey(2), m2).slice(tf)


def test_fused_cat_of_slices_equals_torch_cat():
    ME, tf, m = _field()
    coords = _case()[0]
    widths = dict(zip((2, 8, 32, 128), (12, 16, 24, 32)))
    for extra in (0, 1):  # 16-byte lanes; dword lanes (one width no multiple of 4)
        xs = {ts: _randn(m.get_coordinates(ME.CoordinateMapKey(ts)).shape[0], C + extra * (ts == 8), ts) for ts, C in widths.items()}
        dy = _randn(coords.shape[0], sum(x.shape[1] for x in xs.values()), 77)
        res = []
        for fused in (True, False):
            leaves = {ts: x.clone().cuda().requires_grad_(True) for ts, x in xs.items()}
            parts = [ME.SparseTensor(leaves[ts], ME.CoordinateMapKey(ts), m).slice(tf) for ts in widths]
            if fused:
                assert all(p._F is None for p in parts)  # pending: one launch writes the concatenated rows
                out = ME.cat(*parts)
                assert all(p._F is None for p in parts)
            else:
                for p in parts:
                    p.F  # materialised one by one: ME.cat takes torch.cat
                out = ME.cat(*parts)
            assert isinstance(out, ME.TensorField) and out.coordinate_manager is m and out.C is tf.C
            out.F.backward(dy.cuda())
            res.append((out.F.detach().cpu(), [leaves[ts].grad.cpu() for ts in widths]))
        assert torch.equal(res[0][0], res[1][0])
        assert torch.equal(res[0][0], torch.cat([xs[ts][m.field_map(ME.CoordinateMapKey(ts), tf.C)[0].cpu().long()] for ts in widths], 1))
        for a, b in zip(res[0][1], res[1][1]):
            assert torch.equal(a, b)
    st = ME.SparseTensor(torch.zeros(m.get_coordinates(ME.CoordinateMapKey(1)).shape[0], 4).cuda(), ME.CoordinateMapKey(1), m)
    with pytest.raises(ValueError, match="mixed"):
        ME.cat(st, tf)


def test_misaligned_rows_take_the_dword_kernels():
    """Widths that are multiples of 4 but rows that start 4 bytes off a 16-byte boundary: one source of the fused cat, and
    the dy of the .sparse() backward.  Bitwise torch.cat of the slices; one rounding of the division."""
    from nerf_downstream_amd.minkowski import functional as Fn

    ME, tf, m = _field()
    coords, C = _case()[0], 8
    maps, xs = [], []
    for ts in (2, 8):
        key = ME.CoordinateMapKey(ts)
        maps.append(m.field_map(key, tf.C))
        xs.append(_randn(m.get_coordinates(key).shape[0], C, 600 + ts))
    _, xv = misaligned(xs[1])
    assert xv.data_ptr() % 16 == 4
    y = Fn.FieldGatherCatFunction.apply(maps, xs[0].cuda(), xv)
    assert torch.equal(y.cpu(), torch.cat([x[idx.cpu().long()] for x, (idx, _) in zip(xs, maps)], 1))
    # .sparse() of learned features, as test_sparse_backward_of_learned_features, with the gradient rows misaligned
    vox, inv = PT.quantise(coords)
    leaf = _randn(coords.shape[0], C, 620).cuda().requires_grad_(True)
    st = ME.TensorField(coordinates=coords.cuda(), features=leaf).sparse()
    assert type(st.F.grad_fn).__name__ == "SegmentMeanFunctionBackward"
    order = PT.field_map(st.C.cpu().float(), vox, 1)
    dy = _randn(vox.shape[0], C, 621)
    _, dyv = misaligned(dy)
    seen = []
    st.F.register_hook(lambda g: seen.append(g.data_ptr()))
    assert dyv.data_ptr() % 16 == 4
    st.F.backward(dyv)
    assert seen == [dyv.data_ptr()]  # mink_segment_mean_bwd was handed the misaligned rows themselves
    dy_ref = torch.zeros(vox.shape[0], C, dtype=torch.float64)
    dy_ref[order] = dy.double()
    ref = PT.mean_bwd(dy_ref, inv, vox.shape[0])
    assert bool(((leaf.grad.cpu().double() - ref).abs() <= 2.0 ** -23 * ref.abs()).all())  # one rounding of the division


# ------------------------------------------------------------------------------------------------ 3. .sparse() backward
@pytest.mark.parametrize("C", [3, 8])
def test_sparse_backward_of_learned_features(C):
    from nerf_downstream_amd import minkowski as ME

    coords = _case()[0]
    vox, inv = PT.quantise(coords)
    f, wts = _randn(coords.shape[0], C, 300 + C), _randn(vox.shape[0], C, 310 + C)
    leaf = f.clone().cuda().requires_grad_(True)
    st = ME.TensorField(coordinates=coords.cuda(), features=leaf).sparse()
    hv = st.C.cpu().long()
    order = PT.field_map(hv.float(), vox, 1)  # the restatement's row of every backend row
    assert st.F.shape == (vox.shape[0], C) and int(order.min()) >= 0
    ref_y = PT.voxel_mean(f.double(), inv, vox.shape[0])[order]
    cnt = torch.bincount(inv, minlength=vox.shape[0])[order]
    absum = torch.zeros(vox.shape[0], C, dtype=torch.float64).index_add(0, inv, f.double().abs())[order]
    assert bool(((st.F.detach().cpu().double() - ref_y).abs() <= (cnt[:, None] + 1) * EPS * absum / cnt[:, None]).all())
    (st.F * wts.cuda()).sum().backward()
    dy_ref = torch.zeros(vox.shape[0], C, dtype=torch.float64)
    dy_ref[order] = wts.double()
    ref = PT.mean_bwd(dy_ref, inv, vox.shape[0])
    err = (leaf.grad.cpu().double() - ref).abs()
    print(f"[point] sparse() backward C={C}: max relative error {float((err / ref.abs().clamp_min(TINY)).max()):.3e}")
    assert bool((err <= 2.0 ** -23 * ref.abs()).all())  # one rounding of the division
    # no duplicate voxels: a view of the input, the gradient passes through unchanged
    uniq = torch.cat([coords[:1], coords[200:203]])
    uniq[:, 1:] = torch.tensor([[0.5, 0.5, 0.5], [3.5, -2.5, 1.0], [9.0, 9.0, 9.0], [-7.25, 0.0, 4.0]])
    leaf = _randn(4, C, 5).cuda().requires_grad_(True)
    st = ME.TensorField(coordinates=uniq.cuda(), features=leaf).sparse()
    assert st.F.data_ptr() == leaf.data_ptr()
    dy = _randn(4, C, 6).cuda()
    st.F.backward(dy)
    assert torch.equal(leaf.grad, dy)


# ------------------------------------------------------------------------------------------------ 4. modules on fields
def _field_modules(ME, C):
    return {
        "MinkowskiLinear": lambda: ME.MinkowskiLinear(C, 12, bias=True),
        "MinkowskiBatchNorm": lambda: ME.MinkowskiBatchNorm(C),
        "MinkowskiSyncBatchNorm": lambda: ME.MinkowskiSyncBatchNorm(C),
        "MinkowskiInstanceNorm": lambda: ME.MinkowskiInstanceNorm(C),
        "MinkowskiReLU": lambda: ME.MinkowskiReLU(),
        "MinkowskiLeakyReLU": lambda: ME.MinkowskiLeakyReLU(),
        "MinkowskiELU": lambda: ME.MinkowskiELU(),
        "MinkowskiCELU": lambda: ME.MinkowskiCELU(),
        "MinkowskiSELU": lambda: ME.MinkowskiSELU(),
        "MinkowskiGELU": lambda: ME.MinkowskiGELU(),
        "MinkowskiPReLU": lambda: ME.MinkowskiPReLU(C),
        "MinkowskiDropout": lambda: ME.MinkowskiDropout(p=0.0),
    }


@pytest.mark.parametrize("name", list(_field_modules(None, 8)))
def test_modules_on_fields_return_fields(name):
    """Fails on the parent commit, where these modules return a SparseTensor whatever they are given."""
    from nerf_downstream_amd import minkowski as ME

    C = 8
    coords = _case()[0]
    f = _randn(coords.shape[0], C, 400)
    mod = _field_modules(ME, C)[name]().cuda().train()
    tf = ME.TensorField(coordinates=coords.cuda(), features=f.cuda())
    out = mod(tf)
    assert isinstance(out, ME.TensorField), type(out)
    assert out.coordinate_manager is tf.coordinate_manager and out.C is tf.C
    # the same module on a SparseTensor holding the same F: the same kernel, bitwise.  Instance norm reads per-sample row
    # ranges, so its sparse tensor lives on a map with the field's rows per sample: distinct voxels, one per point.
    grid = torch.cat([coords[:, :1], torch.arange(coords.shape[0], dtype=torch.float32)[:, None], torch.zeros(coords.shape[0], 2)], 1)
    st = ME.TensorField(coordinates=grid.cuda(), features=f.cuda()).sparse()
    assert st.F.shape == f.shape and torch.equal(st.F.cpu(), f)
    ref = mod(st)
    assert isinstance(ref, ME.SparseTensor)
    assert torch.equal(out.F.detach(), ref.F.detach()), name
    # .sparse() of the result works as on the original field (same manager, same voxels)
    sp = out.sparse()
    assert sp.coordinate_manager is tf.coordinate_manager and sp.F.shape[0] == PT.quantise(coords)[0].shape[0]


# ------------------------------------------------------------------------------------------------ 5. global pooling of a field
@pytest.mark.parametrize("C", [3, 32])
def test_global_pooling_of_a_field(C):
    from nerf_downstream_amd import minkowski as ME

    coords = _case()[0]
    off = PR.offsets_of(coords, 2)
    n = coords.shape[0]
    x, dy = _randn(n, C, 500 + C), _randn(2, C, 510 + C)
    outs = {}
    for cls in (ME.MinkowskiGlobalMaxPooling, ME.MinkowskiGlobalSumPooling, ME.MinkowskiGlobalAvgPooling):
        if cls is ME.MinkowskiGlobalAvgPooling and C % 4:
            continue  # (mink_global_avg_fwd: C % 4 == 0, as for sparse tensors)
        leaf = x.clone().cuda().requires_grad_(True)
        tf = ME.TensorField(coordinates=coords.cuda(), features=leaf)
        o = cls()(tf)
        assert isinstance(o, ME.SparseTensor) and o.coordinate_map_key == ME.CoordinateMapKey(0) and o.F.shape == (2, C)
        assert o.coordinate_manager is tf.coordinate_manager
        o.F.backward(dy.cuda())
        outs[cls.__name__] = (o.F.detach().cpu().double(), leaf.grad.cpu().double())
    ry, rarg = PR.global_max_fwd(x, off)
    y, dx = outs["MinkowskiGlobalMaxPooling"]
    assert torch.equal(y, ry) and torch.equal(dx, PR.global_max_bwd(dy, rarg, n))
    y, dx = outs["MinkowskiGlobalSumPooling"]
    ref = PR.global_sum_fwd(x, off)
    assert bool(((y - ref).abs() <= EPS * ref.abs() + TINY).all())
    assert torch.equal(dx, PR.global_sum_bwd(dy, off))
    if "MinkowskiGlobalAvgPooling" in outs:
        y, dx = outs["MinkowskiGlobalAvgPooling"]
        cnt = torch.tensor([off[b + 1] - off[b] for b in range(2)], dtype=torch.float64)[:, None]
        absum = PR.global_sum_fwd(x.abs(), off)
        # a fixed-order fp32 sum of cnt terms and one division: (cnt + 1) roundings of the sum of |terms|
        assert bool(((y - PR.global_avg_fwd(x, off)).abs() <= (cnt + 1) * EPS * absum / cnt).all())
        ref_dx = PR.global_sum_bwd(dy.double() / cnt, off)
        assert bool(((dx - ref_dx).abs() <= (2 * EPS + EPS * EPS) * ref_dx.abs() + TINY).all())  # dy * (1 / cnt): two roundings
    # a batch column that is not non-decreasing is refused, not sorted
    bad = coords.clone()
    bad[100, 0] = 1.0
    tf = ME.TensorField(coordinates=bad.cuda(), features=x.cuda())
    with pytest.raises(ValueError, match="non-decreasing"):
        ME.MinkowskiGlobalMaxPooling()(tf)


# ------------------------------------------------------------------------------------------------ 6. whole networks
def _build(name):
    from nerf_downstream_amd.co3d_3d.src.models.mink.fcnn import MinkowskiFCNN, MinkowskiSplatFCNN
    from nerf_downstream_amd.co3d_3d.src.models.mink.pointnet import MinkowskiPointNet

    torch.manual_seed(3)
    if name == "MinkowskiPointNet":
        net = MinkowskiPointNet(3, 5, embedding_channel=32)
    else:
        net = {"MinkowskiFCNN": MinkowskiFCNN, "MinkowskiSplatFCNN": MinkowskiSplatFCNN}[name](
            3, 5, embedding_channel=32, channels=(8, 12, 16, 24, 32))
    for m in net.modules():
        if type(m).__name__ == "MinkowskiDropout":
            m.p = 0.0
    return net.cuda().train()


def _restated(name, params, coords, feats):
    if name == "MinkowskiPointNet":
        return PT.pointnet_forward(params, coords, feats)
    return PT.fcnn_forward(params, coords, feats, splat=name == "MinkowskiSplatFCNN")


@pytest.mark.parametrize("name", ["MinkowskiFCNN", "MinkowskiSplatFCNN", "MinkowskiPointNet"])
def test_networks_match_float64_restatement(name):
    coords, feats = _case()
    net = _build(name)
    params = {k: v.detach().cpu().double().requires_grad_(True) for k, v in net.named_parameters()}
    wts = _randn(2, 5, 9)
    out = net(net.process_input({"coordinates": coords.cuda(), "features": feats.cuda()}))
    ref = _restated(name, params, coords, feats)
    assert out.shape == (2, 5) == ref.shape
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    print(f"[point] {name}: logits max |err| {err:.3e}")
    assert err <= 1e-3, err
    (out * wts.cuda()).sum().backward()
    (ref * wts.double()).sum().backward()
    hp = dict(net.named_parameters())
    assert all(p.grad is not None for p in hp.values())
    rel = {k: float((hp[k].grad.cpu().double() - params[k].grad).norm() / params[k].grad.norm().clamp_min(1e-12)) for k in hp}
    errs = sorted(rel.values())
    print(f"[point] {name}: parameter-gradient relative error median {errs[len(errs) // 2]:.3e}, max {errs[-1]:.3e} "
          f"({max(rel, key=rel.get)})")
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
    # swapping the two samples of the batch swaps the logit rows
    order = torch.cat([torch.arange(193, 260), torch.arange(0, 193)])
    swapped = coords[order].clone()
    swapped[:, 0] = 1.0 - swapped[:, 0]
    with torch.no_grad():
        out2 = net(net.process_input({"coordinates": swapped.cuda(), "features": feats[order].cuda()}))
    assert torch.allclose(out2.flip(0), out.detach(), atol=1e-5), float((out2.flip(0) - out.detach()).abs().max())


# ------------------------------------------------------------------------------------------------ 7. the trainer CLI
def _train_cli(tmp_path, data_root, tag, env_extra):
    gin = os.path.join(ROOT, "nerf_downstream_amd", "co3d_3d", "configs", "modelnet40_cls.gin")
    cmd = ["timeout", "-k", "10", "150", sys.executable, "-m", "nerf_downstream_amd.co3d_3d.train", "--ginc", gin, "--save_path", str(tmp_path / tag),
           "--ginb", f"ModelNet40H5Dataset.data_root='{data_root}'", "--ginb", "train.batch_size=4", "--ginb", "train.val_batch_size=4",
           "--ginb", "train.max_steps=3", "--ginb", "train.loggers=[]", "--ginb", "train.log_every_n_steps=1",
           "--ginb", "train.train_num_workers=0", "--ginb", "train.val_num_workers=0"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **env_extra)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    losses = re.findall(r"step \d+: train/loss=(\S+)", r.stdout)
    assert len(losses) == 3, r.stdout[-3000:]
    return losses


def test_trainer_cli_with_and_without_prepare_ahead(tmp_path):
    """Three optimiser steps of modelnet40_cls.gin on a 40-shape .npz shard set, in a fresh process: the maps of every batch but
    the first are prepared ahead on the side stream, and the FCNN calls .sparse() on fields DERIVED from the one that holds
    them -- the hand-over must happen there.  The losses equal those of a run that builds every map on the compute stream."""
    root = tmp_path / "shards"
    root.mkdir()
    rng = np.random.default_rng(4)
    for phase, m in (("train", 32), ("test", 8)):
        np.savez(root / f"ply_data_{phase}0.npz", data=rng.uniform(-1, 1, size=(m, 256, 3)).astype(np.float32),
                 label=rng.integers(0, 40, size=(m, 1)).astype(np.int64))
    ahead = _train_cli(tmp_path, str(root), "ahead", {})
    vals = [float(v) for v in ahead]
    assert all(np.isfinite(vals)) and len(set(ahead)) == 3, ahead
    lazy = _train_cli(tmp_path, str(root), "lazy", {"MINK_PREPARE_AHEAD": "0"})
    assert ahead == lazy, (ahead, lazy)
