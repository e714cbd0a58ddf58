"""CPU: the registration stack away from the kernels -- the ResUNet2 registry and state-dict layout (against a fixture spelled
out from the reference constructor, scripts/make_resunet_keys.py), an oracle-backed forward + backward of the BN and IN
variants, the host-side geometry helpers, and the argument checks of mink_knn_cross (refused before any launch)."""
import json
import os

import numpy as np
import pytest
import torch

from helpers import batch_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = [f"ResUNet{n}2{s}" for n in ("BN", "IN") for s in ("", "B", "C", "D", "E")]


def test_ten_variants_are_registered_and_the_base_is_abstract():
    from nerf_downstream_amd.co3d_3d.src.models import MODELS
    from nerf_downstream_amd.co3d_3d.src.models.mink.resunet import ResUNet2
    from oracle import me_cpu as OME

    assert all(n in MODELS for n in VARIANTS) and "ResUNet2" not in MODELS
    with pytest.raises(ValueError, match="base class"):
        ResUNet2(3, 32, ME=OME)
    for n in VARIANTS:
        assert MODELS[n].BLOCK_NORM_TYPE == ("IN" if "IN" in n else "BN") and MODELS[n].NORM_TYPE == "BN"
    assert MODELS["ResUNetIN2E"].CHANNELS == [None, 128, 128, 128, 256] and MODELS["ResUNetIN2E"].TR_CHANNELS == [None, 64, 128, 128, 128]
    assert MODELS["ResUNetBN2"].TR_CHANNELS == [None, 32, 64, 64, 128] and MODELS["ResUNetBN2B"].TR_CHANNELS == [None, 64, 64, 64, 64]


@pytest.mark.parametrize("name,entries", [("ResUNetBN2C", 129), ("ResUNetIN2C", 87)])
def test_state_dict_layout_matches_reference(name, entries):
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from oracle import me_cpu as OME

    want = json.load(open(os.path.join(ROOT, "tests", "golden", "resunet_state_keys_v1.json")))[name]
    model = get_model(name, 3, 32, ME=OME)
    got = [[k, list(v.shape)] for k, v in model.state_dict().items()]
    assert len(got) == entries == len(want)
    assert got == want
    assert sum(p.numel() for p in model.parameters()) == 8_752_000
    assert tuple(model.conv1_tr.kernel.shape) == (96, 64) and tuple(model.final.bias.shape) == (1, 32)


def test_get_block_takes_the_norm_type_first():
    from nerf_downstream_amd.co3d_3d.src.models.mink.modules.resnet_block import BasicBlock, get_block
    from oracle import me_cpu as OME

    blk = get_block("IN", 8, 8, bn_momentum=0.05, D=3, ME=OME)
    assert type(blk) is BasicBlock and isinstance(blk.norm1, OME.MinkowskiInstanceNorm) and blk.downsample is None
    assert get_block("BN", 8, 8, bn_momentum=0.05, ME=OME).norm2.bn.momentum == 0.05


@pytest.mark.parametrize("name", ["ResUNetBN2C", "ResUNetIN2C"])
@pytest.mark.parametrize("normalize", [False, True])
def test_oracle_backed_forward_backward(name, normalize):
    from nerf_downstream_amd.co3d_3d.src.models import MODELS
    from oracle import me_cpu as OME

    torch.manual_seed(0)
    model = MODELS[name](3, 32, normalize_feature=normalize, ME=OME)
    coords, feats = batch_scenes([31, 32], grid=48, cin=3)
    field = model.process_input({"coordinates": coords, "features": feats})
    seen = {}
    model.block4.register_forward_hook(lambda m, i, o: seen.setdefault("s8", o))
    out = model(field)
    assert isinstance(out, OME.SparseTensor) and out.F.shape == (coords.shape[0], 32) and out.tensor_stride[0] == 1
    assert seen["s8"].tensor_stride[0] == 8 and seen["s8"].F.shape[0] > 0 and seen["s8"].F.shape[1] == 256
    norms = out.F.detach().norm(dim=1)
    if normalize:
        assert float((norms - 1).abs().max()) < 1e-6
    else:
        assert float(norms.min()) > 0.1
    G = torch.randn(out.F.shape, generator=torch.Generator().manual_seed(1))
    ((out.F * G).sum() / out.F.shape[0]).backward()
    for k, p in model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), k
    # a SparseTensor goes in as the reference's forward takes it: same result as the field
    again = model(field.sparse())
    assert torch.allclose(again.F, out.F, atol=1e-5)


def test_rotation_and_random_transform_follow_the_reference_draws():
    from scipy.linalg import expm

    from nerf_downstream_amd.co3d_3d.src.utils import geometry as GE

    axis, theta = np.array([0.3, -1.2, 0.5]), 0.7
    R = GE.M(axis, theta)
    u = axis / np.linalg.norm(axis)
    K = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    rodrigues = np.eye(3) + np.sin(theta) * K + (1 - np.cos(theta)) * K @ K  # the rotation by theta about u, in closed form
    assert np.allclose(R, rodrigues, atol=1e-12) or np.allclose(R, rodrigues.T, atol=1e-12)
    assert np.allclose(R, expm(np.cross(np.eye(3), u * theta)), atol=1e-14)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(R) - 1) < 1e-12 and np.allclose(R @ u, u, atol=1e-12)

    pcd = np.random.RandomState(3).rand(50, 3) * 4 + 1
    T = GE.sample_random_trans(pcd, np.random.RandomState(11), 360)
    rg = np.random.RandomState(11)  # the reference's order: the axis first, then the angle
    ax, ang = rg.rand(3) - 0.5, 360 * np.pi / 180.0 * (rg.rand(1) - 0.5)
    want = expm(np.cross(np.eye(3), ax / np.linalg.norm(ax) * ang))
    assert T.shape == (4, 4) and np.array_equal(T[3], [0, 0, 0, 1]) and np.allclose(T[:3, :3], want, atol=1e-14)
    assert np.allclose(T[:3, :3] @ T[:3, :3].T, np.eye(3), atol=1e-12) and abs(np.linalg.det(T[:3, :3]) - 1) < 1e-12
    assert np.allclose(T[:3, :3] @ pcd.mean(0) + T[:3, 3], 0, atol=1e-12)  # the centroid maps to the origin
    assert np.allclose(GE.sample_random_trans(torch.from_numpy(pcd), np.random.RandomState(11)), T)
    small = GE.sample_random_trans(pcd, np.random.RandomState(11), 10)
    assert np.arccos((np.trace(small[:3, :3]) - 1) / 2) <= 5 * np.pi / 180 + 1e-9


def test_pdist_and_corr_dist_by_hand():
    from nerf_downstream_amd.co3d_3d.src.utils import geometry as GE

    A, B = torch.tensor([[0.0, 0.0], [3.0, 4.0]]), torch.tensor([[0.0, 0.0], [0.0, 4.0], [6.0, 8.0]])
    assert torch.equal(GE.pdist(A, B, "SquareL2"), torch.tensor([[0.0, 16.0, 100.0], [25.0, 9.0, 25.0]]))
    assert torch.allclose(GE.pdist(A, B, "L2"), torch.sqrt(torch.tensor([[0.0, 16.0, 100.0], [25.0, 9.0, 25.0]]) + 1e-7))
    with pytest.raises(NotImplementedError):
        GE.pdist(A, B, "L1")
    # est = identity, gth = a translation by (0.3, 0, 0.4) (length 0.5) after a quarter turn about z: the moved points differ by
    # R x + t - x; x = (0,0,0) -> 0.5; x = (1,0,0) -> |(-1+0.3, 1, 0.4)| = sqrt(0.49 + 1 + 0.16) > 1 -> clamped to 1
    est = torch.eye(4)
    gth = torch.eye(4)
    gth[:3, :3] = torch.tensor([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    gth[:3, 3] = torch.tensor([0.3, 0.0, 0.4])
    xyz0 = torch.tensor([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])
    assert abs(float(GE.corr_dist(est, gth, xyz0, None)) - 0.75) < 1e-6
    assert abs(float(GE.corr_dist(est, gth, xyz0, None, max_dist=2)) - (0.5 + 1.65 ** 0.5) / 2) < 1e-6
    assert abs(float(GE.corr_dist(est, gth, xyz0, None, weight=torch.tensor([2.0, 0.0]))) - 0.5) < 1e-6


def test_knn_cross_arguments_are_refused_before_any_launch():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced: every call below is refused before a launch
    ok = dict(q=P, nq=10, ldq=4, c=P, nc=12, ldc=4, C=3, qo=P, co=P, B=1, k=2, idx=P, dist=None)

    def call(**kw):
        a = dict(ok, **kw)
        return L.mink_knn_cross(a["q"], a["nq"], a["ldq"], a["c"], a["nc"], a["ldc"], a["C"], a["qo"], a["co"], a["B"], a["k"], a["idx"],
                                a["dist"], None)

    for kw, word in (({"q": None}, b"NULL"), ({"c": None}, b"NULL"), ({"idx": None}, b"NULL"), ({"qo": None}, b"NULL"),
                     ({"co": None}, b"NULL"), ({"k": 65}, b"k = 65"), ({"k": 0}, b"k = 0"), ({"C": 257}, b"C = 257"),
                     ({"C": 0}, b"C = 0"), ({"ldq": 2}, b"bad shape"), ({"ldc": 2}, b"bad shape"), ({"B": 0}, b"bad shape"),
                     ({"nq": 1 << 30, "k": 2}, b"bad shape"), ({"nq": -1}, b"bad shape")):
        assert call(**kw) == -1, kw
        assert word in L.mink_last_error(), (kw, L.mink_last_error())
    assert call(nq=0, q=None, idx=None) == 0  # no queries: nothing to do, nothing launched
    assert L.mink_abi_version() == 4


def test_get_matching_indices_refuses_more_than_64_slots():
    from nerf_downstream_amd.co3d_3d.src.utils import geometry as GE

    pts = torch.zeros(4, 3)
    for K in (65, 0):
        with pytest.raises(ValueError, match="outside 1..64"):
            GE.get_matching_indices(pts, pts, torch.eye(4), 1.0, K=K)


def test_restatement_of_the_cross_search():
    """The float64 restatement the GPU tests compare against, on a case small enough to read: ties go to the lower row, a sample
    with fewer candidates than k leaves -1 / +inf, and the validity check accepts the exact table and rejects a wrong one."""
    import match_restate as MR

    q = torch.tensor([[0.0], [10.0], [5.0]])
    c = torch.tensor([[1.0], [-1.0], [9.0], [4.0]])
    idx, dist = MR.knn_cross(q, c, [0, 2, 3], [0, 3, 4], 2)
    assert idx.tolist() == [[0, 1], [2, 0], [3, -1]] and dist[0].tolist() == [1.0, 1.0] and dist[2].tolist() == [1.0, float("inf")]
    assert MR.cross_violations(q, c, [0, 2, 3], [0, 3, 4], idx, 2)[:2] == (0, 0)
    out, rep, win, wout = MR.cross_violations(q, c, [0, 2, 3], [0, 3, 4], idx, 2)
    assert win <= 0 and wout <= 0
    wrong = idx.clone()
    wrong[1] = torch.tensor([1, 0])  # row 1 (value 10) given the candidate -1 instead of 9
    assert MR.cross_violations(q, c, [0, 2, 3], [0, 3, 4], wrong, 2)[2] > 0
    wrong = idx.clone()
    wrong[2, 1] = 3
    assert MR.cross_violations(q, c, [0, 2, 3], [0, 3, 4], wrong, 2)[0] == 1
    assert MR.offsets(5) == ([0, 193, 193, 198, 265], [0, 150, 150, 154, 285]) and MR.offsets(1)[1] == [0, 150, 150, 151, 282]
    src, tgt = torch.tensor([[0.0, 0, 0], [5.0, 0, 0]]), torch.tensor([[1.0, 0, 0], [0.0, 0.5, 0], [5.0, 0, 0]])
    assert MR.matching_indices(src, tgt, torch.eye(4), 1.0).tolist() == [[0, 1], [0, 0], [1, 2]]
    assert MR.matching_indices(src, tgt, torch.eye(4), 1.0, K=1).tolist() == [[0, 1], [1, 2]]
