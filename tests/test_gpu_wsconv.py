"""GPU: the weight-sparse convolution (csrc/wsconv.hip, minkowski/wsconv.py, modules/sparse_conv.py) against the float64
restatement of tests/wsconv_restate.py, through the C ABI on random tables, through the modules on the manager's own tables,
through a pruned Res16UNet14 and through evaluate() on a pruned checkpoint.

The bound is derived, not measured: an fp32 fma / add chain of T terms in any order satisfies |y - y64| <= gamma_T S with
gamma_T = T u / (1 - T u), u = 2^-24, S = the sum of the absolute values of the terms."""
import functools
import json
import os

import pytest
import torch

import wsconv_restate as R
from guarded import Guarded, assert_finite, check_all
from helpers import batch_scenes
from nerf_downstream_amd import _lib
from nerf_downstream_amd import gin_lite as gin
from nerf_downstream_amd.minkowski import wsconv

pytestmark = pytest.mark.gpu
CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nerf_downstream_amd", "co3d_3d", "configs")


@functools.lru_cache(None)
def _case(n_out, K, cin, cout, density, n_in=None, integer=False, bias=True, seed=0):
    """(x, kernel, nbr, bias, (y64, T, S)) on the host; computed once per shape and shared."""
    n_in = n_in if n_in is not None else max(n_out // 2, 1) + 3
    g = torch.Generator().manual_seed(seed + 7)
    x = torch.randint(-3, 4, (n_in, cin), generator=g).float() if integer else torch.randn(n_in, cin, generator=g)
    w = R.random_kernel(K, cin, cout, density, seed=seed, integer=integer)
    nbr = R.random_table(n_out, K, n_in, seed=seed + 1)
    b = None
    if bias:
        b = torch.randint(-3, 4, (cout,), generator=g).float() if integer else torch.randn(cout, generator=g)
    return x, w, nbr, b, R.restate(x, w, nbr, n_out, b)


def _forward(x, w, nbr, b, n_out=None):
    p = wsconv.pack_csr(w.cuda())
    return wsconv.wsconv_forward(x.cuda(), p, nbr.cuda(), nbr.shape[0] if n_out is None else n_out, None if b is None else b.cuda()).cpu()


def _check_bound(y, ref, what=""):
    y64, T, S = ref
    err, lim = (y.double() - y64).abs(), R.bound(T, S)
    print(f"{what}: max err {float(err.max()) if err.numel() else 0:.3e}, its bound {float(lim.max()) if lim.numel() else 0:.3e}, max T {int(T.max()) if T.numel() else 0}")
    assert torch.isfinite(y).all()
    bad = err > lim
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} element(s) outside gamma_T S, worst ratio {float((err / lim.clamp_min(1e-300)).max()):.3f}"


SHAPES = [(n, K, 28, 64) for n in (1, 63, 64, 65, 130, 257) for K in (8, 27)] + \
         [(130, 27, 3, 32), (130, 27, 64, 1), (130, 27, 160, 96), (130, 8, 96, 20), (100, 27, 2050, 8)]


@pytest.mark.parametrize("density", [1.0, 0.1, "one", 0.0])
@pytest.mark.parametrize("n_out,K,cin,cout", SHAPES)
def test_operator_within_the_fp32_bound(n_out, K, cin, cout, density):
    x, w, nbr, b, ref = _case(n_out, K, cin, cout, density)
    y = _forward(x, w, nbr, b)
    _check_bound(y, ref, f"n_out={n_out} K={K} cin={cin} cout={cout} density={density}")
    if density == 0.0:
        assert torch.equal(y, b.reshape(1, -1).expand(n_out, cout))
        assert torch.equal(_forward(x, w, nbr, None), torch.zeros(n_out, cout))


def test_wide_tile_and_one_input_row():
    """n_out at the row count from which a workgroup owns 256 rows (four per lane), with a ragged last tile; and n_in = 1."""
    n = _lib.WSCONV_WIDE_ROWS + 1
    for n_out in (n - 2, n):  # the last narrow launch, the first wide one
        x, w, nbr, b, ref = _case(n_out, 27, 28, 64, 0.1, n_in=5000)
        _check_bound(_forward(x, w, nbr, b), ref, f"n_out={n_out}")
    x, w, nbr, b, ref = _case(n, 8, 70, 20, 0.3, n_in=3000, integer=True)  # two channel chunks, a ragged channel tile, exact sums
    assert torch.equal(_forward(x, w, nbr, b).double(), ref[0])
    x, w, nbr, b, ref = _case(130, 27, 28, 64, 0.1, n_in=1)
    _check_bound(_forward(x, w, nbr, b), ref, "n_in=1")


def test_degenerate_kernels_and_tables():
    x, w, nbr, b, _ = _case(130, 27, 28, 64, 0.1)
    w = w.clone()
    w[13] = 0  # an empty offset between non-empty ones
    w[:, :, 5] = 0  # an output channel with no nonzero in any offset
    assert 13 not in wsconv.pack_csr(w).valid_kernel
    y = _forward(x, w, nbr, b)
    _check_bound(y, R.restate(x, w, nbr, 130, b), "offset 13 empty, channel 5 empty")
    assert torch.equal(y[:, 5], b[5].expand(130))
    none = torch.full_like(nbr, -1)  # a table of all -1
    assert torch.equal(_forward(x, w, none, b), b.reshape(1, -1).expand(130, 64))
    assert torch.equal(_forward(x, w, none, None), torch.zeros(130, 64))
    assert _forward(x, w, nbr[:0], b, n_out=0).shape == (0, 64)


@pytest.mark.parametrize("n_out,K,cin,cout", [(257, 27, 28, 64), (130, 8, 160, 96), (100, 27, 2050, 8)])
def test_integer_data_is_exact_and_runs_are_identical(n_out, K, cin, cout):
    """Inputs and weights integer-valued in [-3, 3]: every partial sum is an integer below 2^24, exact in fp32."""
    x, w, nbr, b, ref = _case(n_out, K, cin, cout, 0.3, integer=True)
    y1, y2 = _forward(x, w, nbr, b), _forward(x, w, nbr, b)
    assert torch.equal(y1.double(), ref[0])
    assert torch.equal(y1, y2)
    x, w, nbr, b, _ = _case(n_out, K, cin, cout, 0.1)
    assert torch.equal(_forward(x, w, nbr, b).view(torch.int32), _forward(x, w, nbr, b).view(torch.int32))


def test_pruned_means_skipped():
    x, w, nbr, b, _ = _case(130, 27, 28, 64, 0.3)
    w, xn = w.clone(), x.clone()
    w[:, 7, :] = 0  # every weight of input channel 7 pruned
    xn[:, 7] = float("nan")
    x0 = x.clone()
    x0[:, 7] = 0
    y = _forward(xn, w, nbr, b)
    assert torch.isfinite(y).all() and torch.equal(y, _forward(x0, w, nbr, b))
    # a NaN in a channel with a stored weight: exactly the elements the restatement marks
    w2 = torch.zeros_like(w)
    w2[:, :, :] = w
    w2[:, 9, :] = 0
    w2[4, 9, 3], w2[20, 9, 40] = 1.0, -2.0
    xn = x.clone()
    xn[::3, 9] = float("nan")
    y = _forward(xn, w2, nbr, b)
    y64 = R.restate(xn, w2, nbr, 130, b)[0]
    assert bool(torch.isnan(y64).any()) and not bool(torch.isnan(y64).all())
    assert torch.equal(torch.isnan(y), torch.isnan(y64))


def _abi(x_g, n_in, ldx, cin, nbr_g, n_out, K, p, bufs, y_g, ldy, cout, bias_g):
    from nerf_downstream_amd.minkowski import functional as Fn

    _lib.check(_lib.lib().mink_wsconv_fwd(x_g.ptr, n_in, ldx, cin, nbr_g.ptr, n_out, K, bufs["koffs"].ptr, len(p.valid_kernel),
                                          bufs["rowptr"].ptr, bufs["cptr"].ptr, bufs["colidx"].ptr, bufs["vals"].ptr, p.nnz, y_g.ptr, ldy,
                                          cout, None if bias_g is None else bias_g.ptr, Fn._stream()))
    torch.cuda.synchronize()


@pytest.mark.parametrize("n_out,K,cin,cout,skew,pads", [(130, 27, 28, 64, 0, (5, 3)), (65, 8, 160, 96, 0, (5, 3)), (130, 27, 28, 64, 4, (5, 3)),
                                                         (100, 27, 130, 8, 4, (5, 3)), (130, 27, 28, 64, 0, (4, 8)), (130, 27, 28, 64, 4, (4, 8))])
def test_guard_bands(n_out, K, cin, cout, skew, pads):
    """Every operand exact-size inside NaN / sentinel bands: y with ldy = cout + 3 (or + 8) keeps its pads and bands, x with
    ldx = cin + 5 (or + 4) has NaN pads that never reach a result, the sparse operands and the table are not modified; `skew` = 4 puts x and y four
    bytes behind a 16-byte boundary (the dword branch of the 16-byte accesses)."""
    x, w, nbr, b, ref = _case(n_out, K, cin, cout, 0.1)
    p = wsconv.pack_csr(w.cuda())
    ldx, ldy = cin + pads[0], cout + pads[1]  # (pads that are multiples of 4 keep the 16-byte accesses when the pointer allows them)
    x_g = Guarded.input(x.cuda(), ld=ldx, name="x", skew=skew)
    nbr_g = Guarded.input(nbr.cuda(), name="nbr")
    bufs = {k: Guarded.input(getattr(p, k), name=k) for k in ("koffs", "rowptr", "cptr", "colidx", "vals")}
    bias_g = Guarded.input(b.cuda(), name="bias")
    y_g = Guarded((n_out, ldy), device="cuda", cols=cout, name="y", skew=skew)
    _abi(x_g, x.shape[0], ldx, cin, nbr_g, n_out, K, p, bufs, y_g, ldy, cout, bias_g)
    check_all(x_g, nbr_g, bias_g, y_g, *bufs.values())
    y = y_g.logical().cpu()
    assert_finite(y, "y")
    _check_bound(y, ref, f"guarded skew={skew}")
    assert torch.equal(y, _forward(x, w, nbr, b))  # the same bits as the aligned, unpadded call
    # zero density: every logical element of y is written (the bias), nothing else
    pz = wsconv.pack_csr(torch.zeros_like(w).cuda())
    y_z = Guarded((n_out, ldy), device="cuda", cols=cout, name="y (zero density)", skew=skew)
    _lib.check(_lib.lib().mink_wsconv_fwd(x_g.ptr, x.shape[0], ldx, cin, nbr_g.ptr, n_out, K, None, 0, None, None, None, None, 0, y_z.ptr, ldy, cout,
                                          bias_g.ptr, None))
    torch.cuda.synchronize()
    check_all(y_z, x_g, nbr_g)
    assert pz.nnz == 0 and torch.equal(y_z.logical().cpu(), b.reshape(1, -1).expand(n_out, cout))


# ------------------------------------------------------------------------------------------------------------------ modules
@functools.lru_cache(None)
def _scene():
    from nerf_downstream_amd import minkowski as ME

    coords, feats = batch_scenes([0, 1], grid=32, cin=3)
    return ME.TensorField(coordinates=coords.cuda(), features=feats.cuda()).sparse()


def _pair(kind, cin, cout, k, s, bias, density=0.2):
    """(sparse module, dense module) with the same masked weights, on the device."""
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models.mink.modules import sparse_conv as S

    torch.manual_seed(3)
    tr = kind == "tr"
    sp = (S.WeightSparseConvolutionTranspose if tr else S.WeightSparseConvolution)(cin, cout, kernel_size=k, stride=s, bias=bias, dimension=3)
    de = (ME.MinkowskiConvolutionTranspose if tr else ME.MinkowskiConvolution)(cin, cout, kernel_size=k, stride=s, bias=bias, dimension=3)
    with torch.no_grad():
        sp.kernel.mul_((torch.rand_like(sp.kernel) < density).float())
    de.load_state_dict(sp.state_dict())
    sp, de = sp.cuda().eval(), de.cuda().eval()
    sp.sparsify("csr")
    sp.path = "sparse"
    return sp, de


@pytest.mark.parametrize("kind,k,s", [("conv", 3, 1), ("conv", 3, 2), ("conv", 2, 2), ("tr", 2, 2)])
def test_modules_against_dense_and_restatement(kind, k, s):
    from nerf_downstream_amd import minkowski as ME

    st = _scene()
    m = st.coordinate_manager
    if kind == "tr":  # up-sample the stride-2 map onto the encoder map
        coarse_key = m.stride(st.coordinate_map_key, 2)
        torch.manual_seed(5)
        inp = ME.SparseTensor(torch.randn(m.size(coarse_key), 16, device="cuda"), coarse_key, m)
        _, nbr = m.kernel_table(st.coordinate_map_key, coarse_key, k, 1, transposed=True)
        out_key = st.coordinate_map_key
    else:
        torch.manual_seed(5)
        inp = ME.SparseTensor(torch.randn(st.F.shape[0], 16, device="cuda"), st.coordinate_map_key, m)
        out_key = m.stride(st.coordinate_map_key, s)
        nbr, _ = m.kernel_table(st.coordinate_map_key, out_key, k, 1)
    sp, de = _pair(kind, 16, 24, k, s, bias=True)
    with torch.no_grad():
        ys, yd = sp(inp), de(inp)
    assert ys.coordinate_map_key == yd.coordinate_map_key == out_key and not ys.F.requires_grad
    n_out = m.size(out_key)
    assert ys.F.shape == yd.F.shape == (n_out, 24) and nbr.shape[0] == n_out
    ref = R.restate(inp.F, sp.kernel, nbr, n_out, sp.bias)
    _check_bound(ys.F.cpu(), ref, f"sparse {kind} k={k} s={s}")
    _check_bound(yd.F.cpu(), ref, f"dense {kind} k={k} s={s}")  # (the dense kernel's chain has at least these terms; zeros add nothing)
    # the forced dense path and the "strided" layout give the dense module's bits
    sp.path = "dense"
    assert torch.equal(sp(inp).F, yd.F)
    sp.path = None
    sp.sparsify("strided")
    assert torch.equal(sp(inp).F, yd.F)
    sp.sparsify("coo")
    sp.path = "sparse"
    assert torch.equal(sp(inp).F, ys.F)
    # _flops: per valid offset nnz times the pairs of that offset, plus bias.numel() * rows; a 0-dim int64 device tensor
    pairs = (nbr >= 0).sum(0).cpu()
    per = (sp.kernel != 0).reshape(sp.kernel.shape[0], -1).sum(1).cpu()
    assert sp._flops.dtype == torch.int64 and sp._flops.dim() == 0 and sp._flops.is_cuda
    assert int(sp._flops) == int((pairs * per).sum()) + 24 * n_out


def test_use_mm_and_zaxis_modules():
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.models.mink.modules import sparse_conv as S

    st = _scene()
    m = st.coordinate_manager
    torch.manual_seed(6)
    inp = ME.SparseTensor(torch.randn(st.F.shape[0], 16, device="cuda"), st.coordinate_map_key, m)
    mm = S.WeightSparseConvolution(16, 5, kernel_size=1, bias=True, dimension=3).cuda().eval()
    mm.sparsify()
    with torch.no_grad():
        y = mm(inp)
    assert torch.equal(y.F, inp.F.mm(mm.kernel) + mm.bias) and int(mm._flops) == inp.F.shape[0] * 16 * 5 + 5 * inp.F.shape[0]
    z = S.WeightSparseConvolution(16, 24, kernel_size=3, dimension=3, sparse_mode=2).cuda().eval()
    z.sparsify()
    z.path = "sparse"
    nbr, _ = m.kernel_table(st.coordinate_map_key, st.coordinate_map_key, 3, 1)
    wz = torch.zeros_like(z.kernel)
    wz[[4, 13, 22]] = z.kernel.detach()[[4, 13, 22]]
    ref = R.restate(inp.F, wz, nbr, nbr.shape[0], None)
    with torch.no_grad():
        _check_bound(z(inp).F.cpu(), ref, "ZAXIS sparse")
        z.path = "dense"
        _check_bound(z(inp).F.cpu(), ref, "ZAXIS dense")


# ------------------------------------------------------------------------------------------------------------------ network
def _sparsify(model, path):
    for mod in model.modules():
        if hasattr(mod, "sparsify"):
            mod.sparsify("csr")
            mod.path = path


def test_pruned_network_logits():
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.src.utils import prune as P

    torch.manual_seed(0)
    dense = get_model("Res16UNet14", 3, 5).cuda()
    P.remove(P.global_magnitude_prune(dense, 0.9))
    coords, feats = batch_scenes([0, 1], grid=32, cin=3)
    batch = {"coordinates": coords.cuda(), "features": feats.cuda()}
    dense.train()
    with torch.no_grad():
        dense(dense.process_input(batch))  # running statistics of real activations
    sp = get_model("Res16UNet14", 3, 5, sparse=[1] * 9).cuda()
    sp.load_state_dict(dense.state_dict())
    dense.eval(), sp.eval()
    _sparsify(sp, "sparse")
    with torch.no_grad():
        yd = dense(dense.process_input(batch))
        ys = sp(sp.process_input(batch))
    assert ys.shape == yd.shape == (coords.shape[0], 5) and torch.isfinite(ys).all()
    err = float((ys - yd).abs().max())
    print(f"pruned Res16UNet14: max |sparse - dense| logit = {err:.3e}, max |logit| = {float(yd.abs().max()):.3e}")
    assert err < 1e-3
    layers = [mod for mod in sp.modules() if hasattr(mod, "sparsify") and not mod.use_mm]
    assert len(layers) >= 20
    for mod in layers:
        assert mod.nnz == int((mod.kernel != 0).sum()) and mod._flops is not None
    total = sum(mod.nnz for mod in layers) + sum(int((mod.kernel != 0).sum()) for mod in sp.modules() if getattr(mod, "use_mm", False))
    kept = sum(int((getattr(mo, n) != 0).sum()) for mo, n in P.get_parameters_to_prune(sp))
    assert total == kept and P.count_flops(sp) > 0


def test_evaluate_a_pruned_checkpoint(tmp_path, monkeypatch, capsys):
    """evaluate() on a checkpoint with model.*_orig / *_mask keys and `get_model.sparse` bound, every layer on the sparse kernel,
    against the dense evaluation of the same masked weights."""
    from nerf_downstream_amd.co3d_3d.eval import evaluate
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.src.utils import prune as P

    files = [f"{CFG}/co3d_cls.gin", f"{CFG}/synthetic_seg.gin", f"{CFG}/res16unet.gin"]
    binds = ["SparseVoxelSegDataset.grid=16", "SparseVoxelSegDataset.num_samples=8"]
    monkeypatch.setattr(wsconv, "MAX_DENSITY", 1.0)  # whatever the shipped crossover is, this run takes the sparse kernel
    try:
        gin.clear_config()
        gin.parse_config_files_and_bindings(files, binds + ["get_model.sparse=[1,1,1,1,1,1,1,1,1]", "evaluate.layout='csr'"])
        torch.manual_seed(1)
        model = get_model()
        params = P.global_magnitude_prune(model, 0.9)
        pruned = str(tmp_path / "pruned.ckpt")
        torch.save({"state_dict": {"model." + k: v for k, v in model.state_dict().items()}}, pruned)
        assert any(k.endswith("kernel_mask") for k in model.state_dict())
        num = P.count_parameters(model)
        P.remove(params)
        masked = str(tmp_path / "masked.ckpt")
        torch.save({"state_dict": {"model." + k: v for k, v in model.state_dict().items()}}, masked)
        out = str(tmp_path / "eval")
        res = evaluate(save_path=out, load_path=pruned, tag="sparse")
        assert "num_params, total=" in capsys.readouterr().out
        assert json.load(open(os.path.join(out, "sparse.json"))) == res
        assert sorted(res) == ["val/OA", "val/gflops", "val/loss", "val/mAcc", "val/mIoU", "val/pruned_params", "val/total_params"]
        assert res["val/total_params"] == num["total"] and res["val/pruned_params"] == num["pruned"] and res["val/gflops"] > 0
        gin.clear_config()
        gin.parse_config_files_and_bindings(files, binds)
        ref = evaluate(save_path=out, load_path=masked, tag="dense")
        assert sorted(ref) == ["val/OA", "val/loss", "val/mAcc", "val/mIoU"]  # an unpruned checkpoint: nothing new in the file
        print(f"mIoU sparse {res['val/mIoU']!r} dense {ref['val/mIoU']!r}")
        assert abs(res["val/mIoU"] - ref["val/mIoU"]) <= 1e-6
    finally:
        gin.clear_config()
