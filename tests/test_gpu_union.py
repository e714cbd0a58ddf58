"""-m gpu: the union of sparse tensors (csrc/union.hip, minkowski/union.py) against tests/union_restate.py and the CPU oracle: the
map of the union, the sum and its gradient bit for bit, the module downstream of which convolutions and pooling run, non-finite
values, and CompletionUNet as a whole."""
import ctypes

import numpy as np
import pytest
import torch

import union_restate as U
from helpers import batch_scenes

pytestmark = pytest.mark.gpu

RELATIONS = ("disjoint", "identical", "contained", "partial", "twice", "lonely", "emptied")


def _ME():
    from nerf_downstream_amd import minkowski as ME

    return ME


def _derived(coords, feats, ts, B):
    """A HIP SparseTensor whose map is the int32 rows `coords` at tensor stride ts, on a manager of its own."""
    ME = _ME()
    m = ME.CoordinateManager.from_coordinates(torch.from_numpy(np.ascontiguousarray(coords, np.int32)).cuda(), ts, B)
    return ME.SparseTensor(feats, ME.CoordinateMapKey(ts), m)


def _tensors(lists, ts, B, C=1, seed=0):
    """One tensor per list, each on its own manager (list i and list j that are the same object share a tensor: one input
    given twice), and their features as float32 arrays."""
    gen, made, out = torch.Generator().manual_seed(seed), {}, []
    for c in lists:
        if id(c) not in made:
            made[id(c)] = _derived(c, torch.randn(c.shape[0], C, generator=gen).cuda(), ts, B)
        out.append(made[id(c)])
    return out


def _applies(relation, n, B):
    return not ((relation == "emptied" and B != 3) or (relation == "lonely" and B < 2) or (relation == "partial" and n < 2))


def _check_map(lists, ts, B, seed=0):
    ME = _ME()
    want_c, want_i2o, want_o2i, want_off = U.union_map(lists, B)
    coords, in2out, out2in, off = ME.union.union_map(_tensors(lists, ts, B, seed=seed))
    assert coords.dtype == torch.int32 and coords.shape[0] == want_c.shape[0] == out2in.shape[1]  # the count
    assert torch.equal(coords.cpu(), torch.from_numpy(want_c))
    assert len(in2out) == len(lists) and all(torch.equal(a.cpu(), torch.from_numpy(b)) for a, b in zip(in2out, want_i2o))
    assert torch.equal(out2in.cpu(), torch.from_numpy(want_o2i))
    assert off.cpu().tolist() == want_off.tolist()
    return want_c, want_off


# ------------------------------------------------------------------------------------------------------------------- the map
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("k", [2, 3, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_union_map(n, k, B):
    from nerf_downstream_amd._lib import CONSTANTS

    assert CONSTANTS["MINK_UNION_BLOCK"] == 256 and CONSTANTS["MINK_UNION_MAX_INPUTS"] == 8  # 255 / 256 / 257 / 513: beside its multiples
    ran = []
    for relation in RELATIONS:
        if not _applies(relation, n, B):
            continue
        lists = U.related_lists(np.random.default_rng(1000 * n + 10 * k + B), relation, n, k, B, 2)
        # on the CPU, before the GPU call: the case is what its name says
        rows = [set(map(tuple, c.tolist())) for c in lists]
        total, union = sum(len(r) for r in rows), len(set().union(*rows))
        if relation == "disjoint":
            assert union == total and all(c.shape[0] == n for c in lists)
        elif relation in ("identical", "contained"):
            assert union == len(rows[0]) == n and all(r <= rows[0] for r in rows)
            assert relation == "identical" or n == 1 or len(rows[1]) < n
        elif relation == "partial":
            assert max(len(r) for r in rows) < union < total
            assert all(0 < len(rows[i] & rows[i + 1]) < len(rows[i]) for i in range(k - 1))  # an overlap strictly between none and all
        elif relation == "twice":
            assert lists[1] is lists[0]
        elif relation == "lonely":
            assert (lists[0][:, 0] == B - 1).any() and all((c[:, 0] != B - 1).all() for c in lists[1:])
        elif relation == "emptied":
            assert all((c[:, 0] != 1).all() for c in lists) and any((c[:, 0] == 2).any() for c in lists)
        _, off = _check_map(lists, 2, B)
        if relation == "emptied":
            assert off[1] == off[2] < off[3]
        ran.append(relation)
    assert len(ran) >= (3 if n == 1 and B == 1 else 4)


@pytest.mark.parametrize("ts", [1, 2, 16])
@pytest.mark.parametrize("relation", ["partial", "emptied"])
def test_union_map_tensor_strides_and_the_ends_of_the_key_range(relation, ts):
    B = 3
    lists = U.related_lists(np.random.default_rng(ts), relation, 257, 3, B, ts, edges=True)
    top, bottom = (32767 // ts) * ts, -(32768 // ts) * ts
    assert top + ts > 32767 and bottom - ts < -32768 and lists[0][:, 1:].max() == top and lists[0][:, 1:].min() == bottom
    assert all((c[:, 1:] % ts == 0).all() for c in lists)
    _check_map(lists, ts, B, seed=ts)


# ---------------------------------------------------------------------------------------------------------- sum and backward
def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


@pytest.mark.parametrize("pad", [0, 4, 3])
@pytest.mark.parametrize("C", [1, 3, 4, 32, 36])
def test_union_sum_and_backward(C, pad):
    from nerf_downstream_amd._lib import check, lib

    ME = _ME()
    B, ts, k = 3, 2, 3
    lists = U.related_lists(np.random.default_rng(C), "partial", 257, k, B, ts)
    want_c, want_i2o, want_o2i, _ = U.union_map(lists, B)
    N = want_c.shape[0]
    assert ((want_o2i >= 0).sum(0) == 1).any() and ((want_o2i >= 0).sum(0) >= 2).any()  # rows of one input, and merged rows
    gen = torch.Generator().manual_seed(C)
    feats = [torch.randn(c.shape[0], C, generator=gen) for c in lists]
    feats[0][0, 0] = -0.0  # row 0 of input 0 is union row 0; where input 0 holds it alone, -0.0 must come out as -0.0
    g = torch.randn(N, C, generator=gen)
    want_y = torch.from_numpy(U.union_sum([f.numpy() for f in feats], want_o2i))
    want_g = [torch.from_numpy(a) for a in U.union_grad(g.numpy(), want_i2o)]

    def run():
        xs = [f.cuda().requires_grad_(i != 1) for i, f in enumerate(feats)]  # input 1 asks for no gradient
        y = ME.MinkowskiUnion()(*[_derived(c, x, ts, B) for c, x in zip(lists, xs)])
        y.F.backward(g.cuda())
        return y, xs

    y, xs = run()
    assert torch.equal(y.C.cpu(), torch.from_numpy(want_c)) and y.F.shape == (N, C) and y.F.dtype == torch.float32
    assert torch.equal(_bits(y.F), _bits(want_y))  # bit for bit, the sign of zero included
    assert xs[1].grad is None
    for i in (0, 2):
        assert torch.equal(_bits(xs[i].grad), _bits(want_g[i]))
    y2, xs2 = run()
    assert torch.equal(_bits(y2.F), _bits(y.F)) and all(torch.equal(_bits(xs2[i].grad), _bits(xs[i].grad)) for i in (0, 2))

    # the entry point itself with row pitches above C on every input and on y: the pad columns of y keep what they held
    ldx, ldy = [C + pad, C + 2 * pad, C + pad], C + pad
    bufs = [torch.full((f.shape[0], ld), 1e30).cuda() for f, ld in zip(feats, ldx)]
    for b, f in zip(bufs, feats):
        b[:, :C] = f.cuda()
    out = torch.full((N, ldy), 7.0).cuda()
    o2i = torch.from_numpy(want_o2i).cuda().contiguous()
    ptrs = (ctypes.c_void_p * k)(*[b.data_ptr() for b in bufs])
    check(lib().mink_union_sum(k, ptrs, (ctypes.c_int32 * k)(*ldx), (ctypes.c_int64 * k)(*[f.shape[0] for f in feats]), C, o2i.data_ptr(), N, N,
                               out.data_ptr(), ldy, torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert torch.equal(_bits(out[:, :C]), _bits(want_y)) and bool((out[:, C:] == 7.0).all())


def test_union_of_three_managers_equals_the_union_on_one():
    ME = _ME()
    B, ts, C = 2, 2, 8
    coords = U.related_lists(np.random.default_rng(5), "identical", 300, 3, B, ts)[0]
    gen = torch.Generator().manual_seed(5)
    feats = [torch.randn(coords.shape[0], C, generator=gen) for _ in range(3)]
    apart = ME.MinkowskiUnion()(*[_derived(coords, f.cuda(), ts, B) for f in feats])
    one = _derived(coords, feats[0].cuda(), ts, B)
    m, key = one.coordinate_manager, one.coordinate_map_key
    together = ME.MinkowskiUnion()(one, ME.SparseTensor(feats[1].cuda(), key, m), ME.SparseTensor(feats[2].cuda(), key, m))
    assert together.coordinate_manager is not m
    assert torch.equal(apart.C, together.C) and torch.equal(apart.C.cpu(), torch.from_numpy(coords))
    assert torch.equal(_bits(apart.F), _bits(together.F))
    want = (feats[0] + feats[1]) + feats[2]
    assert torch.equal(_bits(apart.F), _bits(want))
    # one input given twice: every row doubles
    twice = ME.MinkowskiUnion()(one, one)
    assert torch.equal(_bits(twice.F), _bits(feats[0] + feats[0])) and torch.equal(twice.C, one.C)


# ----------------------------------------------------------------------------------------------------------------- the module
def _downstream(oracle_maps, t, emptied=None):
    """3x3x3 convolutions at strides 1 and 2 and a global average pool on the HIP tensor `t` at tensor stride 2, against the
    oracle on a fresh tensor made from the coordinates divided by 2 (a convolution at stride s on multiples of s is the
    stride-1 convolution on the divided coordinates).  (The pattern of tests/test_gpu_generative.py.)"""
    ME = _ME()
    from oracle import me_cpu as OME

    C = t.F.shape[1]
    torch.manual_seed(C)
    coords = t.C.cpu()
    small = coords.clone()
    small[:, 1:] //= 2
    assert torch.equal(small[:, 1:] * 2, coords[:, 1:])
    rt = OME.TensorField(coordinates=small.float(), features=t.F.detach().cpu()).sparse()
    assert torch.equal(rt.C, small)
    for stride in (1, 2):
        rconv = OME.MinkowskiConvolution(C, 12, kernel_size=3, stride=stride, dimension=3)
        hconv = ME.MinkowskiConvolution(C, 12, kernel_size=3, stride=stride, dimension=3).cuda()
        hconv.load_state_dict(rconv.state_dict())
        hy, ry = hconv(t), rconv(rt)
        assert hy.tensor_stride == [2 * stride] * 3
        hc = hy.C.cpu()
        assert torch.equal(hc[:, 0], ry.C[:, 0]) and torch.equal(hc[:, 1:], ry.C[:, 1:] * 2)
        assert torch.allclose(hy.F.detach().cpu(), ry.F.detach(), atol=2e-5, rtol=1e-5)
    hp = ME.MinkowskiGlobalAvgPooling()(t).F.detach().cpu()
    B = t.coordinate_manager.batch_size()
    assert hp.shape == (B, C)
    f, b = t.F.detach().cpu().double(), coords[:, 0].long()
    for s in range(B):
        rows = f[b == s]
        if s == emptied:
            assert rows.shape[0] == 0 and bool((hp[s] == 0).all())  # the pooled row of the emptied sample is zero
        else:
            assert torch.allclose(hp[s].double(), rows.mean(0), atol=2e-5, rtol=1e-5)
    rp = OME.MinkowskiGlobalAvgPooling()(rt).F
    keep = [s for s in range(rp.shape[0]) if s != emptied]
    assert torch.allclose(hp[keep], rp[keep].float(), atol=2e-5, rtol=1e-5)


@pytest.mark.parametrize("relation,emptied", [("partial", None), ("emptied", 1)])
def test_module_and_what_runs_downstream_of_it(oracle_maps, relation, emptied):
    ME = _ME()
    B, ts = 3, 2
    lists = U.related_lists(np.random.default_rng(11), relation, 400, 2, B, ts)
    xs = _tensors(lists, ts, B, C=8, seed=11)
    y = ME.MinkowskiUnion()(*xs)
    m = y.coordinate_manager
    assert all(m is not x.coordinate_manager for x in xs)  # a manager of its own
    assert y.tensor_stride == [ts] * 3 and m.batch_size() == B and m.size(y.coordinate_map_key) == len(y)
    want_c, _, _, want_off = U.union_map(lists, B)
    assert torch.equal(y.C.cpu(), torch.from_numpy(want_c)) and m.batch_offsets(y.coordinate_map_key).cpu().tolist() == want_off.tolist()
    _downstream(oracle_maps, y, emptied=emptied)
    # `+` and ME.cat keep their refusals across managers
    with pytest.raises(ValueError, match="share the coordinate manager"):
        y + xs[0]
    with pytest.raises(ValueError, match="share the coordinate manager"):
        ME.cat(y, xs[0])


def test_module_refusals_on_the_device():
    ME = _ME()
    coords = U.related_lists(np.random.default_rng(0), "identical", 10, 2, 2, 2)[0]
    x = _derived(coords, torch.randn(coords.shape[0], 4, device="cuda"), 2, 2)
    union = ME.MinkowskiUnion()
    with pytest.raises(ValueError, match="at least 2 and at most 8"):
        union(x)
    coarse = coords.copy()
    coarse[:, 1:] *= 2
    with pytest.raises(ValueError, match="one tensor stride"):
        union(x, _derived(coarse, x.F, 4, 2))
    with pytest.raises(ValueError, match="one channel count"):
        union(x, _derived(coords, torch.randn(coords.shape[0], 5, device="cuda"), 2, 2))
    with pytest.raises(ValueError, match="one batch count"):
        union(x, _derived(coords, x.F, 2, 3))
    with pytest.raises(ValueError, match="origin map"):
        union(x, ME.MinkowskiGlobalAvgPooling()(x))


# ----------------------------------------------------------------------------------------------------------------- non-finite
@pytest.mark.parametrize("value", [float("nan"), float("inf"), float("-inf")])
def test_a_non_finite_value_reaches_its_union_row_alone(value):
    ME = _ME()
    B, ts, C, k = 2, 2, 5, 3
    lists = U.related_lists(np.random.default_rng(3), "partial", 257, k, B, ts)
    _, in2out, out2in, _ = U.union_map(lists, B)
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(c.shape[0], C, generator=gen) for c in lists]
    merged = np.nonzero((out2in[0] >= 0) & (out2in[1] >= 0))[0]
    leads = np.nonzero((out2in[1] >= 0) & (out2in[0] < 0))[0]
    assert merged.shape[0] > 0 and leads.shape[0] > 0
    for u in (int(merged[0]), int(leads[0])):  # a row input 1 adds to input 0's, and one where it is the first present (copied)
        poisoned = [f.clone() for f in feats]
        poisoned[1][out2in[1, u], 2] = value
        y = ME.MinkowskiUnion()(*[_derived(c, f.cuda(), ts, B) for c, f in zip(lists, poisoned)]).F.cpu()
        bad = ~torch.isfinite(y)
        assert bad.nonzero().tolist() == [[u, 2]]
        assert torch.equal(_bits(y), _bits(torch.from_numpy(U.union_sum([f.numpy() for f in poisoned], out2in))))  # (same NaN or same infinity)
        assert np.isnan(value) == bool(torch.isnan(y[u, 2])) and (np.isnan(value) or float(y[u, 2]) == value)
    # +inf in one input and -inf in another at one voxel: NaN there, as the float64 sum gives, and nowhere else
    u = int(merged[0])
    poisoned = [f.clone() for f in feats]
    poisoned[0][out2in[0, u], 1], poisoned[1][out2in[1, u], 1] = float("inf"), float("-inf")
    y = ME.MinkowskiUnion()(*[_derived(c, f.cuda(), ts, B) for c, f in zip(lists, poisoned)]).F.cpu()
    ref64 = np.zeros(y.shape, np.float64)
    with np.errstate(invalid="ignore"):
        for f, m in zip(poisoned, in2out):
            np.add.at(ref64, m, f.numpy().astype(np.float64))
    assert np.isnan(ref64[u, 1]) and (~torch.isfinite(y)).nonzero().tolist() == [[u, 1]] and bool(torch.isnan(y[u, 1]))


# ---------------------------------------------------------------------------------------------------------------- whole model
CIN = 4
CLS_BIAS = -8.0  # far below every logit: in training the prediction ORed into the keep mask is empty, the masks are the target's


def _blocks(net):
    return net.dec1, net.dec2, net.dec3


def _model_case():
    """Everything of the whole-model test that needs no GPU: weights, the partial input, the full target, the float64 pass."""
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from oracle import me_cpu as OME

    torch.manual_seed(0)
    model = get_model("CompletionUNet", CIN, 1)
    with torch.no_grad():
        for blk in _blocks(model):
            blk.cls.bias.fill_(CLS_BIAS)
    coords, feats = batch_scenes([41, 42], grid=16, cin=CIN)
    coords = coords.int()
    seen = torch.rand(coords.shape[0], generator=torch.Generator().manual_seed(2)) < 0.5  # the input: half of the target's voxels
    ref = U.RefCompletionUNet(OME, CIN).double()
    ref.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in model.state_dict().items()})
    for net in (model, ref):  # momentum 1: after the one training pass the running statistics ARE that batch's
        for mod in net.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.momentum = 1.0
    ref.train()
    rx = OME.TensorField(coordinates=coords[seen].double(), features=feats[seen].double()).sparse()
    levels, _ = ref(rx, coords.numpy())
    return model, ref, rx, coords, feats, seen, levels


def test_completion_unet(oracle_maps):
    """CompletionUNet against the float64 RefCompletionUNet by the criteria of test_gpu_generative.py::test_completion_net:
    coordinates and occupancy exact, logits and loss within 1e-3, parameter gradients with cosine above 0.999, median relative
    error under 2e-2, worst under 0.15."""
    import torch.nn.functional as F

    ME = _ME()
    model, ref, rx, coords, feats, seen, rlevels = _model_case()
    # on the CPU, before any GPU work: at each level the target keeps at least one and fewer than all voxels, no classifier
    # output comes near zero, and the union adds a row the decoder did not generate or merges one both hold
    assert len(rlevels) == 3
    for logits, occ, c, pred, (n_dec, n_skip, n_union) in rlevels:
        assert 1 <= int(occ.sum()) < occ.shape[0] == c.shape[0] == n_union
        assert not pred.any() and float(logits.detach().max()) < -1.0
        assert n_union > n_dec or n_dec + n_skip > n_union
        print(f"level of {n_union} rows: {n_dec} generated, {n_skip} of the skip, {n_dec + n_skip - n_union} merged, {int(occ.sum())} kept")
    rloss = sum(F.binary_cross_entropy_with_logits(lg[:, 0], torch.from_numpy(occ).double()) for lg, occ, _, _, _ in rlevels) / 3
    rloss.backward()
    # ... and the eval-mode pass without a target keeps some voxels at each level
    with torch.no_grad():
        for blk in _blocks(ref):
            blk.cls.bias.zero_()
        ref.eval()
        for _, _, c, pred, _ in ref(rx)[0]:
            assert 10 <= int(pred.sum())

    hip = model.cuda().train()
    x = ME.SparseTensor(feats[seen].cuda(), coordinates=coords[seen].cuda())
    target = ME.SparseTensor(torch.zeros(coords.shape[0], 1, device="cuda"), coordinates=coords.cuda())
    levels, out = hip(x, target)
    assert out.tensor_stride == [1, 1, 1] and len(levels) == 3
    for (hl, hocc), (rl, rocc, rc, _, _) in zip(levels, rlevels):
        assert torch.equal(hl.C.cpu(), torch.from_numpy(rc)) and hocc.cpu().numpy().tolist() == rocc.tolist()
        err = float((hl.F.detach().cpu().double() - rl.detach()).abs().max())
        print(f"logits of the level at tensor stride {hl.tensor_stride[0]}: max |diff| = {err:.3e}")
        assert err < 1e-3, err
    assert len(out) == int(rlevels[2][1].sum())
    loss = hip.loss(levels)
    print(f"loss {loss.item():.6f} against {rloss.item():.6f}")
    assert abs(loss.item() - rloss.item()) < 1e-3
    loss.backward()
    hp, rp = dict(hip.named_parameters()), dict(ref.named_parameters())
    assert hp.keys() == rp.keys()
    rel = {k: float((hp[k].grad.cpu().double() - rp[k].grad).norm() / rp[k].grad.norm().clamp_min(1e-12)) for k in hp}
    errs = sorted(rel.values())
    flat_g = torch.cat([hp[k].grad.cpu().double().flatten() for k in hp])
    flat_o = torch.cat([rp[k].grad.flatten() for k in hp])
    cosine = float(torch.dot(flat_g, flat_o) / (flat_g.norm() * flat_o.norm()))
    print(f"parameter gradients: cosine {cosine:.6f}, median relative error {errs[len(errs) // 2]:.3e}, worst {max(rel.items(), key=lambda kv: kv[1])}")
    assert max(rel.values()) < 0.15, max(rel.items(), key=lambda kv: kv[1])
    assert errs[len(errs) // 2] < 2e-2, errs[len(errs) // 2]
    assert cosine > 0.999

    # one eval-mode pass without a target: keep = logits > 0
    with torch.no_grad():
        for blk in _blocks(hip):
            blk.cls.bias.zero_()
        hip.eval()
        levels, out = hip(x)
    assert [occ for _, occ in levels] == [None, None, None] and out.tensor_stride == [1, 1, 1]
    generated = set(map(tuple, levels[2][0].C.cpu().tolist()))
    final = list(map(tuple, out.C.cpu().tolist()))
    assert 0 < len(final) <= len(generated) and set(final) <= generated
    assert len(final) == int((levels[2][0].F[:, 0] > 0).sum())
