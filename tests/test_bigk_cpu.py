"""No GPU: the Python surface of the 5^3 / 7^3 sparse convolution (csrc/conv_bigk.hip) -- constructor, refusals, header
declarations and bindings, the offset order, the registration network with a 7^3 stem -- and the float64 restatement
(tests/bigk_restate.py) against a dense float64 conv3d on the densified grid."""
import json
import os

import numpy as np
import pytest
import torch

import bigk_restate as BR
from helpers import batch_scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("ks", [5, 7])
def test_convolution_constructs_with_a_cube_kernel(ks, stride):
    from nerf_downstream_amd import minkowski as ME

    torch.manual_seed(0)
    conv = ME.MinkowskiConvolution(3, 32, kernel_size=ks, stride=stride, bias=True, dimension=3)
    K = ks ** 3
    assert conv.kernel.shape == (K, 3, 32) and conv.bias.shape == (1, 32) and conv.kernel_volume == K and not conv.use_mm
    lim = (3 * K) ** -0.5
    assert float(conv.kernel.detach().abs().max()) <= lim and float(conv.kernel.detach().abs().max()) > 0.9 * lim
    assert float(conv.bias.detach().abs().max()) <= lim
    # a list of equal sizes is the cube
    assert ME.MinkowskiConvolution(3, 8, kernel_size=[ks, ks, ks], dimension=3).kernel.shape == (K, 3, 8)


@pytest.mark.parametrize("ks", [4, 6, 9, [5, 5, 3], 0])
def test_other_kernel_sizes_are_refused_by_name(ks):
    from nerf_downstream_amd import minkowski as ME

    with pytest.raises(ValueError, match="1, 2 .*3, 5 and 7"):
        ME.MinkowskiConvolution(3, 32, kernel_size=ks, dimension=3)


def test_what_stays_refused():
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models.mink.modules.sparse_conv import SparseConvMode, WeightSparseConvolution

    with pytest.raises(ValueError, match="transposed convolutions are implemented for kernel sizes 2 and 3"):
        ME.MinkowskiConvolutionTranspose(8, 8, kernel_size=5, stride=2, dimension=3)
    ws = WeightSparseConvolution(4, 8, kernel_size=5, dimension=3, sparse_mode=SparseConvMode.SPARSE)
    with pytest.raises(ValueError, match="27 offsets at most"):
        ws.sparsify()


def test_symbols_declared_and_bound():
    import ctypes

    from nerf_downstream_amd import _lib

    p, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    S = _lib.SIGNATURES
    assert S["mink_kernel_map_cube"] == (ctypes.c_int, [p, i64, p, i64, i32, i32, p, p, p, i64, p])
    assert S["mink_kernel_map_cube_workspace_bytes"] == (i64, [i64])
    assert S["mink_conv_bigk_gather_gemm"] == (ctypes.c_int, [p, i64, i32, i32, p, i32, i32, p, i64, i32, p, i32, i32, p, p])
    assert S["mink_conv_bigk_wgrad_workspace_bytes"] == (i64, [i64, i32, i32, i32])
    assert S["mink_conv_bigk_wgrad"] == (ctypes.c_int, [p, i64, i32, i32, p, i32, i32, p, i64, i32, p, p, i64, p])
    C = _lib.CONSTANTS
    assert C["MINK_BIGK_MAX_K"] == 343 and C["MINK_BIGK_ROW_TILE"] == 64 and C["MINK_BIGK_WGRAD_ROWS"] == 32
    L = _lib.lib()  # dlopen + bind: a declared symbol the library does not export raises here
    for name in ("mink_kernel_map_cube", "mink_conv_bigk_gather_gemm", "mink_conv_bigk_wgrad"):
        assert getattr(L, name).argtypes == S[name][1]
    # host-side refusals and queries need no device
    assert L.mink_conv_bigk_wgrad_workspace_bytes(2000, 343, 1, 32) >= 16
    assert L.mink_kernel_map_cube_workspace_bytes(1000) == 12 * L.mink_table_capacity(1000)
    assert L.mink_conv_bigk_gather_gemm(None, 0, 4, 4, None, 0, 0, None, 0, 27, None, 8, 8, None, None) != 0
    assert b"28..343" in L.mink_last_error()
    assert L.mink_kernel_map_cube(None, 0, None, 0, 6, 1, None, None, None, 0, None) != 0
    assert b"kernel size 6" in L.mink_last_error()
    assert L.mink_kernel_map_cube(None, 0, None, (1 << 31) // 343 + 1, 7, 1, None, None, None, 0, None) != 0
    assert b"overflows int32" in L.mink_last_error()
    # the existing entries keep their limit and their message
    assert L.mink_kernel_map(None, None, 64, None, 0, None, 125, None, None, None) != 0
    assert b"kernel volume 125 unsupported (1..27)" in L.mink_last_error()


@pytest.mark.parametrize("ks,ts,dil", [(5, 1, 1), (7, 1, 1), (5, 2, 1), (7, 4, 1), (5, 1, 2), (7, 2, 3)])
def test_kernel_offsets_match_the_oracle(ks, ts, dil):
    from nerf_downstream_amd.minkowski.coords import kernel_offsets
    from oracle import maps

    got, want = kernel_offsets(ks, ts, dil), maps.kernel_offsets(ks, ts, dil)
    assert got.dtype == np.int32 and got.shape == (ks ** 3, 3) and np.array_equal(got, want)
    r = (ks - 1) // 2
    assert tuple(got[0]) == (-r * ts * dil,) * 3 and tuple(got[ks ** 3 // 2]) == (0, 0, 0)
    assert tuple(got[1] - got[0]) == (ts * dil, 0, 0)  # x fastest
    assert np.array_equal(got, -got[::-1])  # centred: offset K - 1 - k is the negative of offset k


@pytest.mark.parametrize("ks", [5, 7])
def test_resunet_with_a_cube_stem_keeps_the_reference_layout(ks):
    from nerf_downstream_amd.co3d_3d.src.models import MODELS

    torch.manual_seed(0)
    net = MODELS["ResUNetBN2C"](3, 32, conv1_kernel_size=ks)
    assert net.conv1.kernel.shape == (ks ** 3, 3, 32)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "resunet_state_keys_v1.json")))["ResUNetBN2C"]
    got = [[k, list(v.shape)] for k, v in net.state_dict().items()]
    assert [k for k, _ in got] == [k for k, _ in want]
    assert [(k, s) for k, s in got if k != "conv1.kernel"] == [(k, s) for k, s in want if k != "conv1.kernel"]


def test_models_bind_the_kernel_size_through_gin():
    from nerf_downstream_amd import gin_lite as gin
    from nerf_downstream_amd.co3d_3d.src.models import MODELS
    from nerf_downstream_amd.co3d_3d.src.models.mink.fcnn import MinkowskiFCNN

    try:
        gin.parse_config(["ResUNet2.conv1_kernel_size = 7", "MinkowskiFCNN.kernel_size = 5"])
        net = MODELS["ResUNetBN2C"](3, 32)
        assert net.conv1.kernel.shape == (343, 3, 32)
        fc = MinkowskiFCNN(3, 5, embedding_channel=32, channels=(8, 12, 16, 24, 32))
        assert fc.conv1[0].kernel.shape == (125, 8, 12) and fc.conv4[0].kernel.shape == (125, 24, 32)
        assert fc.conv5[0][0].kernel.shape[0] == 27
    finally:
        gin.clear_config()


@pytest.mark.parametrize("ks,stride", [(5, 1), (7, 1), (5, 2)])
def test_restatement_matches_dense_conv3d(oracle_maps, ks, stride):
    """The restatement (and with it the offset order) against torch's float64 conv3d on the densified grid, forward and
    both gradients."""
    coords, feats = batch_scenes([3], grid=12, cin=3)
    c = coords[:, 1:].int().numpy()
    cin, cout, K, r = 3, 4, ks ** 3, (ks - 1) // 2
    g = torch.Generator().manual_seed(ks)
    w = torch.randn(K, cin, cout, generator=g, dtype=torch.float64)
    inc = np.concatenate([np.zeros((c.shape[0], 1), np.int32), c], 1)
    outc = inc if stride == 1 else oracle_maps.stride_map(inc, stride)[0]
    nbr = oracle_maps.kernel_map_table(inc, outc, oracle_maps.kernel_offsets(ks, 1, 1))
    G = 12
    dense = torch.zeros(1, cin, G, G, G, dtype=torch.float64)
    dense[0, :, c[:, 2], c[:, 1], c[:, 0]] = feats.double().t()  # [z][y][x]
    dense.requires_grad_(True)
    wd = w.reshape(ks, ks, ks, cin, cout).permute(4, 3, 0, 1, 2).clone().requires_grad_(True)  # k = x + ks (y + ks z)
    full = torch.nn.functional.conv3d(dense, wd, padding=r)
    oc = outc[:, 1:]
    got = full[0][:, oc[:, 2], oc[:, 1], oc[:, 0]].t()
    y, T, S = BR.forward(feats, w, nbr)
    assert np.abs(y - got.detach().numpy()).max() < 1e-12 and T.max() <= K * cin and (S >= np.abs(y) - 1e-12).all()
    dy = torch.randn(outc.shape[0], cout, generator=g, dtype=torch.float64)
    (got * dy).sum().backward()
    dx, _, _ = BR.dgrad(dy, w, nbr, c.shape[0])
    assert np.abs(dx - dense.grad[0][:, c[:, 2], c[:, 1], c[:, 0]].t().numpy()).max() < 1e-12
    dw, Tw, _ = BR.wgrad(feats, dy, nbr)
    assert np.abs(dw - wd.grad.permute(2, 3, 4, 1, 0).reshape(K, cin, cout).numpy()).max() < 1e-12
    assert Tw.max() <= outc.shape[0]
