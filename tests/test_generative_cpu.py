"""CPU: the generative layers' public names, constructor refusals, the C entry points' refusals before any launch, and the
ORIENTATION of the generative product (which weight slice belongs to which child) pinned against the oracle's transposed
convolution -- something that is not the new code."""
import os
import re

import numpy as np
import pytest
import torch

import gen_restate as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_names_exist():
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models import MODELS

    assert issubclass(ME.MinkowskiPruning, torch.nn.Module) and issubclass(ME.MinkowskiGenerativeConvolutionTranspose, torch.nn.Module)
    assert callable(ME.generative.occupancy) and callable(ME.CoordinateManager.from_coordinates)
    assert "CompletionNet" in MODELS
    up = ME.MinkowskiGenerativeConvolutionTranspose(5, 7, bias=True)
    assert up.kernel.shape == (8, 5, 7) and up.bias.shape == (1, 7)
    assert float(up.kernel.detach().abs().max()) <= (7 * 8) ** -0.5  # initialised from the OUT channels, like the transposed convolution


@pytest.mark.parametrize("kw", [dict(kernel_size=3), dict(stride=1), dict(dimension=2), dict(dilation=2)])
def test_constructor_refusals(kw):
    from nerf_downstream_amd import minkowski as ME

    with pytest.raises(ValueError, match=r"only kernel_size == stride == 2, dilation == 1, dimension == 3"):
        ME.MinkowskiGenerativeConvolutionTranspose(4, 4, **kw)


def test_header_section_names_generate_hip():
    text = open(os.path.join(ROOT, "include", "mink_hip.h")).read()
    titles = [(m.start(), m.group(1)) for m in re.finditer(r"^/\* -{4,}([^\n]*)", text, flags=re.M)]
    for name in ("mink_generate_children", "mink_prune_workspace_bytes", "mink_prune_compact", "mink_prune_gather", "mink_prune_gather_bwd"):
        pos = re.search(rf"^int(?:64_t)? {name}\(", text, flags=re.M).start()
        title = [t for p, t in titles if p < pos][-1]
        assert "csrc/generate.hip" in title, (name, title)
    src = open(os.path.join(ROOT, "nerf_downstream_amd", "csrc", "generate.hip")).read()
    assert src.count("<<<") == 6  # children, count, scan, scatter, and the two lane forms of the row gather: separate launches


def test_entry_points_refuse_before_any_launch():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    P = 0x10000  # aligned, never dereferenced
    err = L.mink_last_error
    # children: odd tensor stride, NULL, misaligned rows
    assert L.mink_generate_children(P, 10, 3, P, None) == -1 and b"even tensor stride" in err()
    assert L.mink_generate_children(None, 10, 2, P, None) == -1 and b"NULL" in err()
    assert L.mink_generate_children(P + 4, 10, 2, P, None) == -1 and b"16-byte aligned" in err()
    assert L.mink_generate_children(None, 0, 2, None, None) == 0
    # compaction: the workspace travels with its size
    n = 3 * _lib.CONSTANTS["MINK_PRUNE_BLOCK"] + 1
    need = L.mink_prune_workspace_bytes(n)
    assert need >= 4 * 4 and L.mink_prune_workspace_bytes(200_000) >= 4 * (200_000 // _lib.CONSTANTS["MINK_PRUNE_BLOCK"])
    assert L.mink_prune_compact(P, P, n, 2, P, P, P, P, P, P, need - 1, None) == -1
    assert b"workspace" in err() and str(need).encode() in err()
    assert L.mink_prune_compact(P, P, n, 2, P, P, P, P, P, P + 4, need, None) == -1 and b"workspace" in err()
    assert L.mink_prune_compact(None, P, n, 2, P, P, P, P, P, P, need, None) == -1 and b"NULL" in err()
    assert L.mink_prune_compact(P, P, 0, 2, P, P, P, P, P, P, need, None) == -1 and b"at least one row" in err()
    assert L.mink_prune_compact(P, P, n, 0, P, P, P, P, P, P, need, None) == -1
    assert L.mink_prune_compact(P, P + 8, n, 2, P, P, P, P, P, P, need, None) == -1 and b"16-byte aligned" in err()
    # row passes: pitch below the width, NULL
    assert L.mink_prune_gather(P, 3, 10, 4, P, 5, P, 4, None) == -1 and b"bad shape" in err()
    assert L.mink_prune_gather(P, 4, 10, 4, None, 5, P, 4, None) == -1 and b"NULL" in err()
    assert L.mink_prune_gather_bwd(P, 4, 5, 4, P, 10, P, 3, None) == -1 and b"bad shape" in err()
    assert L.mink_prune_gather_bwd(P, 4, 5, 4, P, 10, None, 4, None) == -1 and b"NULL" in err()
    assert L.mink_prune_gather(P, 4, 10, 4, P, 0, P, 4, None) == 0


def test_restated_children_and_offsets_follow_kernel_offsets():
    from nerf_downstream_amd.minkowski.coords import kernel_offsets

    for ts in (2, 4, 16):
        assert np.array_equal(R.child_offsets(ts // 2), kernel_offsets(2, ts // 2))
    c = R.children(np.array([[0, -4, 0, 8], [1, 4, 4, -8]]), 4)
    assert c.shape == (16, 4) and c[0].tolist() == [0, -4, 0, 8] and c[1].tolist() == [0, -2, 0, 8] and c[15].tolist() == [1, 6, 6, -6]


def test_orientation_against_the_oracle_transposed_convolution(oracle_maps):
    """The field of ALL children of a handful of parents -> oracle sparse() -> stride 2 -> MinkowskiConvolutionTranspose(2, 2):
    on that map every fine voxel has exactly one parent, so the oracle's result IS the generative product.  Row for row after
    matching coordinates, float64."""
    from oracle import me_cpu as OME

    torch.manual_seed(3)
    parents = R.random_parents(np.random.default_rng(5), 7, 2, 2)
    kids = R.children(parents, 2)
    cin, cout = 5, 3
    tf = OME.TensorField(coordinates=torch.from_numpy(kids).double(), features=torch.zeros(kids.shape[0], 1, dtype=torch.float64))
    fine = tf.sparse()
    cm = fine.coordinate_manager
    coarse_key = cm.stride(fine.coordinate_map_key, 2)
    coarse = cm.get_coordinates(coarse_key).numpy()
    assert sorted(map(tuple, coarse.tolist())) == sorted(map(tuple, parents.tolist()))
    xp = torch.randn(coarse.shape[0], cin, dtype=torch.float64)  # features on the ORACLE's coarse rows
    up = OME.MinkowskiConvolutionTranspose(cin, cout, kernel_size=2, stride=2, bias=True, dimension=3).double()
    ref = up(OME.SparseTensor(xp, coarse_key, cm))
    row_of = {tuple(r): i for i, r in enumerate(ref.C.numpy().tolist())}
    got = R.gen_product(xp, up.kernel.detach(), up.bias.detach())
    mine = R.children(coarse, 2)
    assert len(row_of) == mine.shape[0] == 8 * coarse.shape[0]
    order = torch.tensor([row_of[tuple(r)] for r in mine.tolist()])
    assert torch.allclose(got, ref.F.detach()[order], atol=1e-13, rtol=0)
    # ... and the weight slices really differ, so a permuted k would have been seen
    assert not torch.allclose(R.gen_product(xp, up.kernel.detach().flip(0), up.bias.detach()), ref.F.detach()[order], atol=1e-3)
