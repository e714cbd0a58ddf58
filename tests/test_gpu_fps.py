"""-m gpu: mink_fps_scenes against the numpy float32 restatement (tests/fps_restate.py).  The outputs are row indices, so every
comparison is exact equality.  Integer voxel coordinates have squared distances that are integers below 2^24: every
arithmetic order agrees on them and only the tie rule (lowest row) can go wrong; float coordinates with a large offset make
the rounding order matter.  Scene sizes straddle the wave, the workgroup and every residency threshold of include/mink_hip.h;
the large ones take 8 picks so that the whole file runs in a few seconds."""
import numpy as np
import pytest
import torch

import fps_restate as FR

pytestmark = pytest.mark.gpu


def _lib():
    from nerf_downstream_amd import _lib

    return _lib


def _thresholds():
    L = _lib()
    return L.FPS_XYZ_REG_ROWS_SMALL, L.FPS_XYZ_REG_ROWS, L.FPS_DIST_REG_ROWS


def _offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _run(xyz, sizes, m, start, **kw):
    """xyz: a host float tensor [n, 3]; -> picks int64 [B, m] on the host."""
    from nerf_downstream_amd.minkowski.utils import farthest_point_sample

    off = torch.tensor(_offsets(sizes), dtype=torch.int32)
    out = farthest_point_sample(xyz.cuda(), off.cuda(), m, torch.tensor(start, dtype=torch.int32).cuda(), **kw)
    assert out.dtype == torch.int64 and out.is_cuda and tuple(out.shape) == (len(sizes), m)
    return out.cpu().numpy()


def _compare(xyz, sizes, m, start, **kw):
    got = _run(xyz, sizes, m, start, **kw)
    want = FR.fps_batch(xyz.numpy(), _offsets(sizes), m, start)
    for b, n in enumerate(sizes):
        assert np.array_equal(got[b], want[b]), (f"scene {b} of {n} rows, start {start[b]}: first difference at pick "
                                                 f"{int(np.nonzero(got[b] != want[b])[0][0])}: {got[b][:12]} vs {want[b][:12]}")
    return got


def _lattice(n, seed, side=48):
    """n voxel coordinates on an integer grid (distances^2 <= 3 * 47^2 < 2^24), many of them at equal distances."""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(0, side, (n, 3), generator=g).float()


def test_integer_coordinates_at_every_boundary():
    small, xyz_reg, dist_reg = _thresholds()
    sizes = [1, 2, 63, 64, 65, 1023, 1024, 1025, small - 1, small, small + 1, xyz_reg - 1, xyz_reg, xyz_reg + 1, dist_reg - 1,
             dist_reg, dist_reg + 1]
    xyz = _lattice(sum(sizes), 0)
    start = [(7 * n) // 11 for n in sizes]
    _compare(xyz, sizes, 8, start)


@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (1e3, 1e4)])
def test_float_coordinates(scale, shift):
    small, xyz_reg, dist_reg = _thresholds()
    sizes = [65, 1025, small - 500, xyz_reg - 3000, dist_reg - 30000, dist_reg + 3000]
    g = torch.Generator().manual_seed(int(scale))
    xyz = torch.randn(sum(sizes), 3, generator=g) * scale + shift
    _compare(xyz, sizes, 16, [n // 3 for n in sizes])


def test_small_scenes_fewer_points_than_picks_coincident_and_duplicated_rows():
    pts = _lattice(40, 1)
    scenes = [pts[:3],                                  # N < m: the tail is local row 0
              pts[:12],                                 # N == m
              pts[5:6].repeat(20, 1),                   # all points coincident: start, then row 0 for ever
              torch.cat([pts[:9], pts[:9], pts[:9]]),   # every row three times: a copy is never picked while a new position remains
              torch.tensor([[0.0, 0, 0], [1, 0, 0], [3, 0, 0]])]
    sizes = [len(s) for s in scenes]
    got = _compare(torch.cat(scenes), sizes, 12, [1, 11, 7, 20, 1])
    off = _offsets(sizes)
    assert (got[0][3:] == off[0]).all() and sorted(got[0][:3] - off[0]) == [0, 1, 2]
    assert sorted(got[1] - off[1]) == list(range(12))
    assert got[2].tolist() == [off[2] + 7] + [off[2]] * 11
    firsts = got[3][:9] - off[3]
    assert len({int(r) % 9 for r in firsts}) == 9 and (got[3][9:] == off[3]).all()
    assert (got[4] - off[4]).tolist() == [1, 2, 0] + [0] * 9


@pytest.mark.parametrize("ld", [3, 4])
@pytest.mark.parametrize("where", ["first", "last"])
def test_mixed_batch_start_rows_and_leading_dimension(ld, where):
    from nerf_downstream_amd.minkowski.utils import farthest_point_sample

    small, xyz_reg, dist_reg = _thresholds()
    sizes = [small - 548, dist_reg + 2656, xyz_reg - 3192, 3, dist_reg - 37344]  # one call, every residency
    xyz = _lattice(sum(sizes), 2, side=128)
    start = [0 if where == "first" else n - 1 for n in sizes]
    want = FR.fps_batch(xyz.numpy(), _offsets(sizes), 8, start)
    off = torch.tensor(_offsets(sizes), dtype=torch.int32).cuda()
    first = torch.tensor(start, dtype=torch.int32).cuda()
    if ld == 3:
        src = xyz.cuda()
    else:  # columns 1..3 of float (batch, x, y, z) rows, as process_input passes them: no copy, a pointer one float in
        full = torch.cat([torch.full((len(xyz), 1), float("nan")), xyz], 1).cuda()
        src = full[:, 1:4]
        assert src.stride(0) == 4 and src.data_ptr() == full.data_ptr() + 4
    got = farthest_point_sample(src, off, 8, first, n_max=max(sizes)).cpu().numpy()
    assert np.array_equal(got, want)
    again = farthest_point_sample(src, off, 8, first).cpu().numpy()  # (the default bound: all rows) -- and repeatable
    assert np.array_equal(again, want)


def test_int32_coordinates_are_converted():
    from nerf_downstream_amd.minkowski.utils import farthest_point_sample

    xyz = _lattice(700, 4)
    coords = torch.cat([torch.zeros(700, 1), xyz], 1).int().cuda()
    got = farthest_point_sample(coords[:, 1:4], torch.tensor([0, 300, 700], dtype=torch.int32).cuda(), 10, torch.tensor([5, 6])).cpu().numpy()
    assert np.array_equal(got, FR.fps_batch(xyz.numpy(), [0, 300, 700], 10, [5, 6]))


def test_two_calls_give_identical_output():
    sizes = [5000, 70, 30000]
    xyz = _lattice(sum(sizes), 5)
    a = _run(xyz, sizes, 32, [1, 2, 3])
    b = _run(xyz, sizes, 32, [1, 2, 3])
    assert np.array_equal(a, b)


def test_empty_scene_and_bad_start_raise_and_leave_the_rest_sampled():
    from nerf_downstream_amd.minkowski.utils import SampleSceneError, farthest_point_sample, fps_status_check

    xyz = _lattice(300, 6)
    dev = torch.device("cuda", 0)
    for off, start, word, bad in (([0, 100, 100, 300], [0, 0, 0], "empty scene", 1), ([0, 100, 200, 300], [0, 100, 5], "first pick outside", 1),
                                  ([0, 100, 200, 300], [0, -1, 5], "first pick outside", 1), ([0, 100, 200, 400], [0, 0, 0], "empty scene", 2)):
        o, s = torch.tensor(off, dtype=torch.int32, device=dev), torch.tensor(start, dtype=torch.int32, device=dev)
        with pytest.raises(SampleSceneError, match=word):
            farthest_point_sample(xyz.cuda(), o, 6, s)
        idx, (host, ev) = farthest_point_sample(xyz.cuda(), o, 6, s, status_async=True)
        ev.synchronize()
        with pytest.raises(SampleSceneError, match=word):
            fps_status_check(host)
        idx = idx.cpu().numpy()
        assert (idx[bad] == -1).all()
        for b in range(3):
            if b != bad:
                assert np.array_equal(idx[b], off[b] + FR.fps_scene(xyz.numpy()[off[b]:off[b + 1]], 6, start[b]))
    with pytest.raises(SampleSceneError, match="n_max"):
        farthest_point_sample(xyz.cuda(), torch.tensor([0, 100, 300], dtype=torch.int32, device=dev), 6, torch.tensor([0, 0]), n_max=150)


# ------------------------------------------------------------------------------------------------------------ end to end
def _tree(tmp_path):
    from test_sampling_cpu import coords_of, write_scenes

    raw = write_scenes(tmp_path, sizes=(3000, 2500))
    return raw, np.concatenate([coords_of(r["links"]) for r in raw])


@pytest.mark.parametrize("which", ["FarthestPointSample", "RandomSample"])
def test_compact_dataset_through_process_input_and_dgcnn(tmp_path, monkeypatch, which):
    from nerf_downstream_amd import gin_lite as gin
    from nerf_downstream_amd.co3d_3d.src.data.co3d import Co3DDataset
    from nerf_downstream_amd.co3d_3d.src.data.utils import collate_mink
    from nerf_downstream_amd.co3d_3d.src.models import MODELS

    raw, xyz = _tree(tmp_path)
    monkeypatch.chdir(tmp_path)
    gin.clear_config()
    try:
        gin.parse_config(f"{which}.num_points = 64")
        ds = Co3DDataset(phase="train", data_root=str(tmp_path / "data"), features=["density", "sh"], compact=True,
                         train_transformations=[which, "RandomRotation", "RandomFeatureJitter"])
        host = collate_mink([ds[0], ds[1]])
    finally:
        gin.clear_config()
    assert "links" in host and host["sample_points"] == 64
    if which == "RandomSample":
        want = host["sample_rows"].numpy()
    else:
        want = FR.fps_batch(xyz, [0, 3000, 5500], 64, host["fps_start"].tolist())
    batch = {k: (v.cuda() if torch.is_tensor(v) and k != "aug_params" else v) for k, v in host.items()}
    torch.manual_seed(0)
    net = MODELS["DGCNN_cls"](28, 51, k=20, emb_dims=64, dropout=0.0, channels=(16, 16, 32, 32), head=(32, 16)).cuda().train()
    seen = {}
    augment = net._augment

    def spy(b, **kw):  # what the augmentation program is handed: the sampled batch, still untransformed
        seen["coords"], seen["offsets"], seen["density"] = b["coordinates"].clone(), b["scene_offsets"].clone(), b["features"][:, 0].clone()
        return augment(b, **kw)

    monkeypatch.setattr(net, "_augment", spy)
    field = net.process_input(batch)
    assert seen["offsets"].tolist() == [0, 64, 128]
    got = seen["coords"].cpu().numpy()
    assert got.shape == (128, 4) and np.array_equal(got[:, 0], np.repeat([0, 1], 64))
    assert np.array_equal(got[:, 1:].astype(np.float32), xyz[want.reshape(-1)])  # the rows it kept: the picks, in pick order
    dens = np.concatenate([r["density"].reshape(-1) for r in raw])
    assert np.array_equal(seen["density"].cpu().numpy(), dens[want.reshape(-1)])
    assert field.C.shape[0] == 128 and (field.C[:, 0] == 0).sum() == 64 and field.F.shape == (128, 28)
    assert np.array_equal(field.F[:, 0].cpu().numpy(), dens[want.reshape(-1)])  # (the jitter leaves the density column alone)
    out = net(field)
    loss = torch.nn.functional.cross_entropy(out, batch["labels"])
    loss.backward()
    assert out.shape == (2, 51) and bool(torch.isfinite(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())
    # the deferred path the trainer takes: the same rows, the status word looked at with the next batch
    pend = net.process_input(batch, defer=True)
    field2 = net.finish_input(pend)
    assert field2.C.shape[0] == 128 and np.array_equal(seen["coords"].cpu().numpy(), got)
    if net._sampler_status is not None:  # (the farthest-point sampler: a clean status word)
        net._check_sampler_status()
