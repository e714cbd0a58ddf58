"""-m gpu: grouped convolution (csrc/gconv.hip) against the float64 restatement of tests/gconv_restate.py -- forward, data
gradient and weight gradient with error / bound <= 1 at every group width that has a kernel of its own (4 and 8: vector FMA;
16, 32, 64: fp32 matrix cores; unequal, tiny and depthwise: the generic kernel), on maps whose row counts are no multiple of any
tile (1,380 rows at stride 1, 1,512 -> 432 at stride 2), on the one-pixel image and on an empty table; every call twice, bit for
bit.  Then the layer: dense.Conv2d(groups=32) and autograd against F.conv2d(groups=32), the 2048-wide 1x1 layers of the
Bottleneck networks through the existing kernels, and where a NaN of x or dy may and may not show."""
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import gconv_restate as GR

pytestmark = pytest.mark.gpu

SHAPES = {"20x23 stride 1": (3, 20, 23, 1), "21x24 stride 2": (3, 21, 24, 2), "one pixel": (1, 1, 1, 1)}
WIDTHS = [(32, 4, 4), (32, 8, 8), (32, 16, 16), (32, 32, 32), (32, 64, 64), (3, 5, 7), (2, 4, 8), (5, 1, 1)]
OFFSET = {(32, 16, 16), (3, 5, 7)}  # x = normal + 3: products of one sign, a wrong column cannot cancel away


def _tables(shape, k):
    from nerf_downstream_amd.co3d_2d.src.model import dense

    B, H, W, stride = SHAPES[shape]
    og, nbr, nbr_t, _ = dense._conv_tables(dense.Grid(B, H, W), k, stride, k // 2, torch.device("cpu"))
    return B * H * W, og.rows, nbr, nbr_t, stride


@functools.lru_cache(maxsize=None)
def case(shape, k, G, ci, co):
    """(inputs, tables, float64 reference, bounds) of one case, computed once and shared; nobody writes into it."""
    n_in, n_out, nbr, nbr_t, stride = _tables(shape, k)
    x, w, dy = GR.inputs(n_in, n_out, k * k, G, ci, co, seed=G * 100 + ci, offset=3.0 if (G, ci, co) in OFFSET else 0.0)
    return (x, w, dy), (nbr, nbr_t, stride), GR.reference(x, w, dy, nbr), GR.bounds(x, w, dy, nbr)


def run_kernels(x, w, dy, nbr, nbr_t, stride):
    """The three passes as GroupedConvolutionFunction launches them, each twice: {"y", "dx", "dw"} on the CPU."""
    from nerf_downstream_amd.minkowski import functional as Fn

    K, G, ci, co = w.shape
    dev = torch.device("cuda", 0)
    x, w, dy, nbr, nbr_t = (t.to(dev).contiguous() for t in (x, w, dy, nbr, nbr_t))
    same_map = stride == 1
    out = {}
    for rep in range(2):
        got = {"y": Fn.gconv(x, w, nbr, G, ci, co),
               "dx": Fn.gconv(dy, w, nbr, G, co, ci, w_transposed=True, flip_k=True) if same_map else
                     Fn.gconv(dy, w, nbr_t, G, co, ci, w_transposed=True),
               "dw": Fn.gconv_wgrad(x, dy, nbr, G, ci, co)}
        torch.cuda.synchronize()
        for name, t in got.items():
            if rep:
                assert torch.equal(t.view(torch.int32), out[name].view(torch.int32)), f"{name}: two runs differ"
            out[name] = t
    return {name: t.cpu().reshape(t.shape[0], -1) if name != "dw" else t.cpu() for name, t in out.items()}


def check_case(shape, k, G, ci, co):
    (x, w, dy), (nbr, nbr_t, stride), ref, bd = case(shape, k, G, ci, co)
    got = run_kernels(x, w, dy, nbr, nbr_t, stride)
    ratios = {name: GR.worst(got[name], ref[name], bd[name]) for name in ("y", "dx", "dw")}
    print(f"{shape}, k = {k}, (G, ci, co) = {(G, ci, co)}: error / bound " + " ".join(f"{n}={r:.3f}" for n, r in ratios.items()))
    assert all(r <= 1 for r in ratios.values()), ratios


@pytest.mark.parametrize("G,ci,co", WIDTHS)
@pytest.mark.parametrize("shape", ["20x23 stride 1", "21x24 stride 2"])
def test_gconv_matches_the_restatement(shape, G, ci, co):
    check_case(shape, 3, G, ci, co)


@pytest.mark.parametrize("shape", ["20x23 stride 1", "21x24 stride 2"])
def test_gconv_pointwise_kernel(shape):
    check_case(shape, 1, 32, 8, 8)


@pytest.mark.parametrize("G,ci,co", [(32, 4, 4), (32, 16, 16), (32, 64, 64), (3, 5, 7)])
def test_gconv_one_pixel_image(G, ci, co):
    """B = 1, H = W = 1, pad 1: eight of the nine table columns are -1."""
    (_, _, _), (nbr, _, _), _, _ = case("one pixel", 3, G, ci, co)
    assert nbr.shape == (1, 9) and int((nbr < 0).sum()) == 8 and int(nbr[0, 4]) == 0
    check_case("one pixel", 3, G, ci, co)


@functools.lru_cache(maxsize=None)
def line_case(n, K, G, ci, co):
    """A line of n pixels with K offsets r - K // 2 .. r + K // 2 (-1 past the ends); its transposed table is the flipped one."""
    r = torch.arange(n).view(n, 1) + torch.arange(K).view(1, K) - K // 2
    nbr = torch.where((r >= 0) & (r < n), r, torch.full_like(r, -1)).int()
    x, w, dy = GR.inputs(n, n, K, G, ci, co, seed=K + ci)
    return (x, w, dy), nbr, GR.reference(x, w, dy, nbr), GR.bounds(x, w, dy, nbr)


@pytest.mark.parametrize("G,ci,co", [(32, 4, 4), (32, 8, 8), (32, 16, 16), (32, 64, 64), (3, 5, 7)])
def test_gconv_27_offsets(G, ci, co):
    """K = 27, the most a launch takes: the weight-gradient kernels built for up to 27 accumulators, the generic weight gradient
    behind widths 4 and 8 (their own needs K <= 9), and at width 64 the forward's 110,592 bytes of LDS, above the 64 KB a
    workgroup gets without asking."""
    (x, w, dy), nbr, ref, bd = line_case(150, 27, G, ci, co)
    got = run_kernels(x, w, dy, nbr, nbr.flip(1).contiguous(), 1)
    ratios = {name: GR.worst(got[name], ref[name], bd[name]) for name in ("y", "dx", "dw")}
    print(f"150 pixels in a line, K = 27, (G, ci, co) = {(G, ci, co)}: error / bound " + " ".join(f"{n}={r:.3f}" for n, r in ratios.items()))
    assert all(r <= 1 for r in ratios.values()), ratios


@pytest.mark.parametrize("G,ci,co", [(32, 8, 8), (32, 32, 32), (3, 5, 7)])
def test_gconv_empty_table(G, ci, co):
    from nerf_downstream_amd.minkowski import functional as Fn

    dev = torch.device("cuda", 0)
    x, w, _ = GR.inputs(7, 0, 9, G, ci, co, seed=1)
    nbr = torch.empty(0, 9, dtype=torch.int32, device=dev)
    y = Fn.gconv(x.to(dev), w.to(dev), nbr, G, ci, co)
    dw = Fn.gconv_wgrad(x.to(dev), torch.empty(0, G * co, device=dev), nbr, G, ci, co)
    torch.cuda.synchronize()
    assert y.shape == (0, G * co) and dw.shape == (9, G, ci, co) and not bool(dw.any())


def _rows_to_nchw(y, g):
    return y.view(g.B, g.H, g.W, -1).permute(0, 3, 1, 2)


@pytest.mark.parametrize("cin,cout,stride,hw", [(128, 128, 1, 20), (512, 512, 2, 21)])
def test_grouped_dense_conv_matches_torch(cin, cout, stride, hw):
    """dense.Conv2d(groups=32) keeps torch's weight layout: the repacking of the weights and of their gradient, through autograd,
    against F.conv2d(groups=32) on the CPU with the tolerances of test_gpu_dense2d.py::test_dense_conv_matches_torch."""
    from nerf_downstream_amd.co3d_2d.src.model import dense

    torch.manual_seed(0)
    x0 = torch.randn(3, cin, hw, hw + 3)
    conv = dense.Conv2d(cin, cout, 3, stride, 1, groups=32).cuda()
    w0 = conv.weight.detach().cpu().clone()
    assert tuple(w0.shape) == (cout, cin // 32, 3, 3)
    x = x0.clone().cuda().requires_grad_(True)
    rows, grid = x.permute(0, 2, 3, 1).reshape(-1, cin), dense.Grid(3, hw, hw + 3)
    y, og, partial = conv(rows, grid, bn_stats=True)
    assert partial is None  # a grouped layer leaves the statistics to the batch norm
    xr, wr = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=stride, padding=1, groups=32)
    assert (og.B, og.H, og.W) == (3, yr.shape[2], yr.shape[3])
    gy = torch.randn_like(yr)
    (yr * gy).sum().backward()
    (_rows_to_nchw(y, og) * gy.cuda()).sum().backward()
    scale = float(yr.detach().abs().max())
    assert torch.allclose(_rows_to_nchw(y, og).detach().cpu(), yr.detach(), atol=2e-5 * max(scale, 1.0))
    assert torch.allclose(conv.weight.grad.cpu(), wr.grad, atol=2e-4 * float(wr.grad.abs().max()))
    assert torch.allclose(x.grad.cpu(), xr.grad, atol=2e-5 * float(xr.grad.abs().max()) + 1e-6)


@pytest.mark.parametrize("cin,cout", [(2048, 512), (512, 2048)])
def test_wide_pointwise_layers_run_on_the_existing_kernels(cin, cout):
    """The 1x1 layers of layer4 of the Bottleneck networks: up to 2048 channels in and out on a 2 x 7 x 7 batch, forward and
    backward with bn_stats=True (where the statistics epilogue answers "no partials" the norm computes its own), followed by the
    batch norm.  The convolution alone at the tolerances of test_dense_conv_matches_torch, the norm behind it at
    test_dense_maxpool_and_batchnorm_match_torch's 1e-5 plus the convolution's tolerance divided by the smallest channel sd (the norm
    divides by it)."""
    from nerf_downstream_amd.co3d_2d.src.model import dense

    torch.manual_seed(2)
    x0 = torch.randn(2, cin, 7, 7)
    conv, bn, bnr = dense.Conv2d(cin, cout, 1, 1, 0).cuda(), dense.BatchNorm2d(cout).cuda(), nn.BatchNorm2d(cout)
    w0 = conv.weight.detach().cpu().clone()
    x = x0.clone().cuda().requires_grad_(True)
    grid = dense.Grid(2, 7, 7)
    y, og, partial = conv(x.permute(0, 2, 3, 1).reshape(-1, cin), grid, bn_stats=True)
    y.retain_grad()  # (`partial` may be None: the norm then computes its own statistics)
    out = bn(y, relu=True, partial=partial)
    xr, wr = x0.clone().requires_grad_(True), w0.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr)
    yr.retain_grad()
    outr = torch.relu(bnr(yr))
    g = torch.randn_like(outr)
    (outr * g).sum().backward()
    (_rows_to_nchw(out, og) * g.cuda()).sum().backward()
    scale = float(yr.detach().abs().max())
    conv_tol = 2e-5 * max(scale, 1.0)
    assert torch.allclose(_rows_to_nchw(y, og).detach().cpu(), yr.detach(), atol=conv_tol)
    sd = float(yr.detach().std((0, 2, 3), unbiased=False).min())
    assert torch.allclose(_rows_to_nchw(out, og).detach().cpu(), outr.detach(), atol=1e-5 + conv_tol / sd)
    assert torch.allclose(bn.running_var.cpu(), bnr.running_var, atol=1e-5 * max(1.0, float(bnr.running_var.max())))
    # the gradients of the convolution from the SAME gradient of its output (torch's), then the whole chain
    gyr = yr.grad
    assert torch.allclose(_rows_to_nchw(y.grad, og).cpu(), gyr, atol=1e-5 * max(1.0, float(gyr.abs().max())) + conv_tol / sd)
    conv.weight.grad, x.grad = None, None
    y2, og, _ = conv(x.permute(0, 2, 3, 1).reshape(-1, cin), grid, bn_stats=True)
    (_rows_to_nchw(y2, og) * gyr.cuda()).sum().backward()
    assert torch.allclose(conv.weight.grad.cpu(), wr.grad, atol=2e-4 * float(wr.grad.abs().max()))
    assert torch.allclose(x.grad.cpu(), xr.grad, atol=2e-5 * float(xr.grad.abs().max()) + 1e-6)


def _masked_worst(got, ref, bound):
    """Non-finite exactly where the restatement is, inside the bound everywhere else."""
    bad = ~torch.isfinite(ref)
    assert torch.equal(~torch.isfinite(got), bad), (int((~torch.isfinite(got)).sum()), int(bad.sum()))
    z = torch.zeros((), dtype=torch.float64)
    return GR.worst(torch.where(bad, z.float(), got), torch.where(bad, z, ref), torch.where(bad, z + 1, bound)), int(bad.sum())


@pytest.mark.parametrize("G,ci,co", [(32, 4, 4), (32, 16, 16), (3, 5, 7)])
@pytest.mark.parametrize("shape", ["20x23 stride 1", "21x24 stride 2"])
def test_gconv_non_finite_footprint(shape, G, ci, co):
    """One NaN in one input channel of one pixel reaches that group's output columns at the pixels whose window holds it and
    nothing else; one NaN in dy reaches, through the data gradient, that group's input columns at the pixels of its window and,
    through the weight gradient, column o of that group at the offsets its row has a neighbour for (a corner pixel: not all)."""
    (x, w, dy), (nbr, nbr_t, stride), _, _ = case(shape, 3, G, ci, co)
    B, H, W, _ = SHAPES[shape]
    x, dy = x.clone(), dy.clone()
    g, pix = G // 2, 1 * H * W + 0 * W + 1  # image 1, top row
    x[pix, g * ci + ci - 1] = float("nan")
    ref, bd = GR.reference(x, w, dy, nbr), GR.bounds(x, w, dy, nbr)
    got = run_kernels(x, w, dy, nbr, nbr_t, stride)
    r, n = _masked_worst(got["y"], ref["y"], bd["y"])
    cols = torch.zeros(G * co, dtype=torch.bool)
    cols[g * co:(g + 1) * co] = True
    bad = ~torch.isfinite(got["y"])
    assert r <= 1 and n > 0 and not bool(bad[:, ~cols].any()) and n == int((nbr == pix).any(1).sum()) * co
    # (dw of that group is NaN too, where the restatement's is)
    assert _masked_worst(got["dw"], ref["dw"], bd["dw"])[0] <= 1

    (x, w, dy), _, _, _ = case(shape, 3, G, ci, co)
    dy = dy.clone()
    orow, o = nbr.shape[0] - 1, co - 1  # the last output pixel: a corner
    dy[orow, g * co + o] = float("nan")
    ref, bd = GR.reference(x, w, dy, nbr), GR.bounds(x, w, dy, nbr)
    got = run_kernels(x, w, dy, nbr, nbr_t, stride)
    r, n = _masked_worst(got["dx"], ref["dx"], bd["dx"])
    assert r <= 1 and n == int((nbr[orow] >= 0).sum()) * ci
    r, n = _masked_worst(got["dw"], ref["dw"], bd["dw"])
    assert r <= 1 and n == int((nbr[orow] >= 0).sum()) * ci and n < 9 * ci
    assert GR.worst(got["y"], ref["y"], bd["y"]) <= 1
