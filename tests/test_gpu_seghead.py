"""-m gpu: the segmentation tail in HIP (csrc/seghead.hip) against the float64 restatement (tests/seghead_restate.py):
loss, gradient, prediction / confusion matrix / counts, run-to-run determinism, slice(), bad labels, and the trainer and
co3d_3d/eval.py end to end.  Inputs are seeded: logits ~ N(0, 3^2) clipped to +-16, 5 % of the labels ignored."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seghead_restate as R
from nerf_downstream_amd import gin_lite as gin

pytestmark = pytest.mark.gpu

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nerf_downstream_amd", "co3d_3d", "configs")
IGNORE = 255
# (N, C, ldz): the shapes of the issue, one with a row stride wider than C
SHAPES = [(1, 2, 2), (63, 8, 8), (4097, 13, 13), (200_000, 20, 20), (1_200_000, 21, 21), (50_001, 21, 24)]


def _record(kind, tag, ratio):
    """measured / bound: printed (pytest -s shows it) and, when SEGHEAD_PARITY_LOG names a file, appended to it
    (profiles/seghead_parity.txt is such a file)."""
    print(f"[seghead] {tag}: {kind} |err| / bound = {ratio:.4f}")
    path = os.environ.get("SEGHEAD_PARITY_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{ratio:8.4f}  {kind:8s} {tag}\n")


def _dev(z, ldz):
    """fp32 logits on the device with row stride ldz."""
    zt = torch.from_numpy(z).cuda()
    if ldz == z.shape[1]:
        return zt
    wide = torch.full((z.shape[0], ldz), float("nan"), device="cuda")
    wide[:, : z.shape[1]] = zt
    return wide[:, : z.shape[1]]


def _native(zt, labels_t, wt, ignore=IGNORE, g=1.0, backward=True):
    """The C entry points called directly -> dict(loss, lse, pred, hist, stats, dz); dz is NaN-filled before the call."""
    from nerf_downstream_amd._lib import check, lib
    from nerf_downstream_amd.minkowski._rt import _ptr, _stream
    from nerf_downstream_amd.minkowski.head import seg_stats

    L = lib()
    n, C = zt.shape
    dev = zt.device
    lse = torch.empty(n, device=dev)
    pred = torch.empty(n, dtype=torch.int32, device=dev)
    hist = torch.full((C, C), -7, dtype=torch.int64, device=dev)
    stats = torch.full((5,), -7, dtype=torch.int64, device=dev)
    loss = torch.empty((), device=dev)
    ws = torch.empty(max(L.mink_seg_ce_workspace_bytes(n, C), 8), dtype=torch.uint8, device=dev)
    is64 = int(labels_t.dtype == torch.int64)
    check(L.mink_seg_ce_forward(zt.data_ptr(), zt.stride(0), labels_t.data_ptr(), is64, _ptr(wt), ignore, n, C, lse.data_ptr(),
                                pred.data_ptr(), hist.data_ptr(), stats.data_ptr(), loss.data_ptr(), ws.data_ptr(), ws.numel(), _stream()))
    out = {"loss": loss, "lse": lse, "pred": pred, "hist": hist, "stats": stats}
    if backward:
        dz = torch.full((n, C), float("nan"), device=dev)
        gt = torch.tensor(g, device=dev)
        check(L.mink_seg_ce_backward(zt.data_ptr(), zt.stride(0), labels_t.data_ptr(), is64, _ptr(wt), ignore, lse.data_ptr(),
                                     stats.data_ptr(), gt.data_ptr(), n, C, dz.data_ptr(), _stream()))
        out["dz"] = dz
    torch.cuda.synchronize()
    out["st"] = seg_stats(stats)
    return out


def _check_against_restatement(z, labels, w, got, g=1.0, tag=""):
    n, C = z.shape
    ref = R.ce(z, labels, w, IGNORE)
    zmax = max(1.0, float(np.abs(z).max()))
    bound = (C + 8) * 2.0 ** -24 * zmax
    err = abs(got["loss"].item() - ref["loss"])
    _record("loss", tag, err / bound)
    assert err <= bound, (tag, err, bound)
    assert abs(got["st"]["den"] - ref["den"]) <= 1e-12 * max(ref["den"], 1.0) and abs(got["st"]["num"] - ref["num"]) <= bound * ref["den"]
    if "dz" in got:
        dz = got["dz"].cpu().numpy().astype(np.float64)
        assert not np.isnan(dz).any(), "an element of dz was left unwritten"
        gb = (C + 8) * 2.0 ** -23 * ref["wy"] / ref["den"] * abs(g)
        ratio = np.abs(dz - g * ref["grad"]) / np.maximum(gb, 1e-300)[:, None]
        valid, _, _ = R.classify(labels, C, IGNORE)
        worst = float(ratio[ref["wy"] > 0].max()) if (ref["wy"] > 0).any() else 0.0
        _record("gradient", tag, worst)
        assert worst <= 1.0, (tag, worst)
        assert (dz[~valid] == 0).all(), "ignored rows must get exact zeros"
    return ref


@pytest.mark.parametrize("weighted", [False, True], ids=["unweighted", "weighted"])
@pytest.mark.parametrize("n,C,ldz", SHAPES, ids=[f"{n}x{C}ld{l}" for n, C, l in SHAPES])
@pytest.mark.timeout(120)
def test_loss_and_gradient_against_float64(n, C, ldz, weighted):
    """Items 5 and 6.  Bound of the loss: |loss - ref| <= (C + 8) * 2^-24 * max(1, max|z|).  The row maximum is exact; exp
    and log are within 2 ulp; a C-term fp32 sum adds at most C * 2^-24 relative; adding the maximum back and subtracting z_y
    add one rounding each on values bounded by max|z| + log C; the sums over the rows are in double; a weighted mean of rows
    inherits the per-row bound.  The gradient adds one multiplication and the division:
    |dz - ref| <= (C + 8) * 2^-23 * w[y_i] / den per element, exact zeros on ignored rows, every element written (dz is
    filled with NaN before the call).  Worst-case bounds: the measured / bound ratios are printed."""
    z, labels, w = R.make_case(n, C, seed=100 + n % 97 + C, weighted=weighted)
    zt, yt = _dev(z, ldz), torch.from_numpy(labels).cuda()
    wt = None if w is None else torch.from_numpy(w).cuda()
    got = _native(zt, yt, wt, g=0.75)
    _check_against_restatement(z, labels, w, got, g=0.75, tag=f"{n}x{C} ld{ldz} {'w' if weighted else '-'}")
    # ... and the autograd front door is these kernels
    from nerf_downstream_amd import minkowski as ME

    leaf = zt.detach().clone().requires_grad_(True) if ldz == C else None
    if leaf is not None:
        loss, pred, hist, stats = ME.seg_cross_entropy(leaf, yt, weight=wt, ignore_index=IGNORE, want_pred=True, want_hist=True)
        (loss * 0.75).backward()
        assert torch.equal(loss.detach(), got["loss"]) and torch.equal(leaf.grad, got["dz"])
        assert torch.equal(pred, got["pred"]) and torch.equal(hist, got["hist"]) and torch.equal(stats, got["stats"])
        assert not pred.requires_grad and not hist.requires_grad


@pytest.mark.parametrize("dtype", [torch.int64, torch.int32], ids=["int64", "int32"])
@pytest.mark.parametrize("n,C,ldz", SHAPES, ids=[f"{n}x{C}ld{l}" for n, C, l in SHAPES])
@pytest.mark.timeout(120)
def test_prediction_histogram_and_counts_are_exact(n, C, ldz, dtype):
    """Item 7: pred / hist / counts equal numpy's argmax / bincount on the same fp32 logits, with constructed ties (two
    equal maxima in 1 % of the rows: the lowest index wins)."""
    z, labels, w = R.make_case(n, C, seed=7 + C, ties=True)
    got = _native(_dev(z, ldz), torch.from_numpy(labels).cuda().to(dtype), None, backward=False)
    pred = R.argmax_first(z)
    assert np.array_equal(got["pred"].cpu().numpy(), pred)
    assert np.array_equal(got["hist"].cpu().numpy(), R.fast_hist(pred, labels, C, IGNORE))
    valid, ignored, bad = R.classify(labels, C, IGNORE)
    assert (got["st"]["n_valid"], got["st"]["n_ignored"], got["st"]["n_bad"]) == (int(valid.sum()), int(ignored.sum()), 0)
    assert got["hist"].sum().item() == int(valid.sum())


def test_empty_and_all_ignored_batches():
    z0 = torch.empty(0, 20, device="cuda")
    got = _native(z0, torch.empty(0, dtype=torch.int64, device="cuda"), None)
    assert np.isnan(got["loss"].item()) and got["hist"].abs().sum().item() == 0 and got["stats"].abs().sum().item() == 0
    z, labels, _ = R.make_case(1000, 20, seed=1)
    got = _native(torch.from_numpy(z).cuda(), torch.full((1000,), IGNORE, dtype=torch.int64, device="cuda"), None)
    assert np.isnan(got["loss"].item()) and got["st"]["n_ignored"] == 1000 and got["st"]["den"] == 0.0
    assert (got["dz"] == 0).all()  # the documented deviation: zeros, where torch writes NaN; the NaN loss stops the trainer


@pytest.mark.timeout(120)
def test_results_are_bitwise_reproducible():
    """Item 8: forward and backward run twice on (1 200 000, 21), and once more on a side stream."""
    z, labels, w = R.make_case(1_200_000, 21, seed=11, weighted=True)
    zt, yt, wt = torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(w).cuda()
    a, b = _native(zt, yt, wt), _native(zt, yt, wt)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        c = _native(zt, yt, wt)
    torch.cuda.current_stream().wait_stream(side)
    for other in (b, c):
        for k in ("loss", "lse", "pred", "hist", "stats", "dz"):
            assert torch.equal(a[k], other[k]), k


def _duplicated_field(seed, n_vox=3000, max_members=9, C=21):
    rng = np.random.default_rng(seed)
    vox = np.unique(rng.integers(0, 24, (n_vox, 3)), axis=0)
    m = rng.integers(1, max_members + 1, len(vox))
    m[0] = max_members
    rows = np.repeat(np.arange(len(vox)), m)
    rng.shuffle(rows)
    xyz = vox[rows] + rng.random((len(rows), 3)) * 0.9  # distinct points of one voxel
    coords = np.concatenate([np.zeros((len(rows), 1)), xyz], 1).astype(np.float32)
    feats = rng.standard_normal((len(rows), C)).astype(np.float32)
    return torch.from_numpy(coords), torch.from_numpy(feats), int(m.max())


def test_slice_gather_and_segment_sum():
    """Item 9: SliceFunction forward == F[inverse] exactly; backward within m * 2^-24 * sum |dy_member| of a float64 segment
    sum (a fixed-order fp32 sum of m terms), bitwise equal between two runs; up to 9 points per voxel; no duplicates: no copy."""
    from nerf_downstream_amd import minkowski as ME

    coords, feats, mmax = _duplicated_field(5)
    assert mmax == 9
    field = ME.TensorField(coordinates=coords.cuda(), features=feats.cuda())
    x = field.sparse()
    mgr = x.coordinate_manager
    inv = mgr.field_inverse.long()
    assert x.F.shape[0] < feats.shape[0] and mgr.field_members is not None
    leaf = torch.randn(x.F.shape[0], 21, device="cuda", generator=torch.Generator("cuda").manual_seed(1)).requires_grad_(True)
    y = ME.SparseTensor(leaf, x.coordinate_map_key, mgr).slice(field).F
    assert torch.equal(y.detach(), leaf.detach()[inv])
    dy = torch.randn(y.shape, device="cuda", generator=torch.Generator("cuda").manual_seed(2))
    g1, = torch.autograd.grad(y, leaf, dy, retain_graph=True)
    g2, = torch.autograd.grad(y, leaf, dy)
    assert torch.equal(g1, g2)
    ref = R.segment_sum(dy.cpu().numpy(), inv.cpu().numpy(), leaf.shape[0])
    mag = R.segment_sum(np.abs(dy.cpu().numpy()), inv.cpu().numpy(), leaf.shape[0])
    members = np.bincount(inv.cpu().numpy(), minlength=leaf.shape[0])[:, None]
    assert (np.abs(g1.cpu().numpy() - ref) <= members * 2.0 ** -24 * mag).all()
    for C in (1, 3, 20):  # any width, not only multiples of 4
        src = torch.randn(leaf.shape[0], C, device="cuda")
        assert torch.equal(ME.slice_rows(src, mgr.field_inverse, *mgr.field_members), src[inv])
    # no duplicates: the identity, the same storage
    from helpers import batch_scenes

    c2, f2 = batch_scenes([3], grid=16, cin=4)
    field2 = ME.TensorField(coordinates=c2.cuda(), features=f2.cuda())
    x2 = field2.sparse()
    assert x2.slice(field2).F.data_ptr() == x2.F.data_ptr()


def test_bad_labels_are_counted_and_raise_in_python():
    """Item 10: 3 labels of value C + 5: the native path counts them (no device-side assert), loss and gradient are those of
    the restatement with the rows left out, and the trainer's metrics raise ValueError.  Bad labels never reach torch's
    NLL kernel here."""
    from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import SegmentationTraining

    n, C = 5000, 20
    z, labels, w = R.make_case(n, C, seed=21, bad=3)
    zt, yt = torch.from_numpy(z).cuda(), torch.from_numpy(labels).cuda()
    got = _native(zt, yt, None)
    assert got["st"]["n_bad"] == 3
    _check_against_restatement(z, labels, None, got, tag="bad labels")
    m = SegmentationTraining(model=None, ignore_label=IGNORE)
    leaf = zt.clone().requires_grad_(True)
    loss = m.loss(leaf, yt)
    assert torch.equal(loss.detach(), got["loss"])
    with pytest.raises(ValueError, match=r"3 labels.*\[0, 20\)"):
        m.train_metrics(leaf.detach(), {"labels": yt})
    with pytest.raises(ValueError, match="3 labels"):
        m.val_metrics(m.val_vector(zt, yt))
    clean = torch.where(yt == C + 5, torch.full_like(yt, IGNORE), yt)
    assert m.val_metrics(m.val_vector(zt, clean))["val/loss"] == pytest.approx(R.ce(z, labels, None, IGNORE)["loss"], abs=1e-5)


def _seg_setup(extra=()):
    gin.clear_config()
    gin.parse_config_files_and_bindings(
        [f"{CFG}/co3d_cls.gin", f"{CFG}/synthetic_seg.gin"],
        ["train.gpus=1", "train.batch_size=4", "train.val_batch_size=4", "SparseVoxelSegDataset.grid=32",
         "SparseVoxelSegDataset.num_samples=16", "train.lr=0.05", "train.scheduler_name='PolyLR'", *extra])


@pytest.mark.long
@pytest.mark.timeout(120)
def test_trainer_metrics_and_gradients_match_the_torch_expressions():
    """Item 11: SegmentationTraining + Res16UNet14A on the synthetic segmentation set (grid 32).  The first step's loss,
    train/* metrics and the val/* dict equal what the torch expressions this module used before give on the same logits
    (loss within the bound of item 5, count-derived metrics exactly); the parameter gradients of a step through the new loss
    match those through F.cross_entropy within 2e-5 of their largest magnitude (tests/test_gpu_parity_full.py's bound)."""
    from nerf_downstream_amd.co3d_3d.src.data.data_module import DataModule
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import SegmentationTraining, confusion, iou_metrics
    from nerf_downstream_amd.co3d_3d.train import _to_device

    _seg_setup()
    try:
        dev = torch.device("cuda", 0)
        torch.manual_seed(0)
        model = get_model().to(dev)
        model.train()
        module = SegmentationTraining(model)
        data = DataModule(batch_size=4, val_batch_size=4, train_num_workers=0, val_num_workers=0)
        batch = _to_device(next(iter(data.train_dataloader())), dev)
        C = 8

        loss, out = module.training_step(batch)
        got = module.train_metrics(out.detach(), batch)
        logits, labels = out.detach(), batch["labels"].long()
        want_loss = F.cross_entropy(logits, labels, ignore_index=IGNORE)
        bound = (C + 8) * 2.0 ** -24 * max(1.0, float(logits.abs().max()))
        print(f"[seghead] trainer loss {loss.item():.8f} torch {want_loss.item():.8f} |err| / bound = {abs(loss.item() - want_loss.item()) / bound:.4f}")
        assert abs(loss.item() - want_loss.item()) <= bound
        miou, macc, oa = iou_metrics(confusion(logits.argmax(1), labels, C))
        want = {"train/mIoU": miou, "train/mAcc": macc, "train/OA": oa,
                "train/ignore_ratio": 100.0 * float((labels == IGNORE).float().mean())}
        assert got == want, (got, want)
        assert 0 < got["train/ignore_ratio"] < 20

        def grads(loss_fn):
            model.zero_grad(set_to_none=True)
            o = module.forward(model.process_input(batch))
            loss_fn(o).backward()
            torch.cuda.synchronize()
            return model.final.kernel.grad.clone(), model.conv0p1s1[0].kernel.grad.clone()

        new = grads(lambda o: module.loss(o, labels))
        old = grads(lambda o: F.cross_entropy(o, labels, ignore_index=IGNORE))
        for a, b, name in zip(new, old, ("final.kernel", "conv0p1s1[0].kernel")):
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            print(f"[seghead] {name}.grad max|diff| / max|grad| = {err / scale:.3e}")
            assert scale > 0 and err <= 2e-5 * scale, (name, err, scale)

        vbatch = _to_device(next(iter(data.val_dataloader())), dev)
        model.eval()
        module.keep_val_logits = True
        with torch.no_grad():
            got_val = module.val_metrics(module.val_accumulate(vbatch))
        vlogits, vlabels = module.last_val[0], module.last_val[1].long()
        want_vloss = F.cross_entropy(vlogits, vlabels, ignore_index=IGNORE).item()
        miou, macc, oa = iou_metrics(confusion(vlogits.argmax(1), vlabels, C))
        assert (got_val["val/mIoU"], got_val["val/mAcc"], got_val["val/OA"]) == (miou, macc, oa)
        assert abs(got_val["val/loss"] - want_vloss) <= (C + 8) * 2.0 ** -24 * max(1.0, float(vlogits.abs().max()))
        assert sorted(got_val) == ["val/OA", "val/loss", "val/mAcc", "val/mIoU"]
    finally:
        gin.clear_config()


@pytest.mark.long
@pytest.mark.timeout(150)
def test_eval_end_to_end(tmp_path):
    """Item 12: 10 training steps on the synthetic set, evaluate() the last.ckpt: <tag>.json's val/mIoU equals validate()'s on
    the same weights exactly, eval_results.json has C + 1 entries per list and its per-class IoU equals the restatement on
    the accumulated histogram; a second call without `replace` leaves both files untouched."""
    from nerf_downstream_amd.co3d_3d.eval import evaluate
    from nerf_downstream_amd.co3d_3d.src.data.data_module import DataModule
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.train import TRAINING_MODULES, load_checkpoint, train, validate, validation_pass

    _seg_setup(["train.max_steps=10", "train.val_every_n_steps=10", "train.log_every_n_steps=5"])
    try:
        train(save_path=str(tmp_path / "run"), resume_training=False, run_name="s", run_name_postfix=None)
        ckpt, out = str(tmp_path / "run" / "s" / "last.ckpt"), str(tmp_path / "eval")
        res = evaluate(save_path=out, load_path=ckpt, tag="t", visualize=True)
        assert json.load(open(os.path.join(out, "t.json"))) == res and 0.0 < res["val/mIoU"] <= 100.0

        dev = torch.device("cuda", 0)
        model = get_model().to(dev)
        load_checkpoint(ckpt, model, weights_only=True)
        module = TRAINING_MODULES["SegmentationTraining"](model)
        loader = DataModule(val_batch_size=1, val_num_workers=0).val_dataloader()
        assert validate(module, loader, dev, 1)["val/mIoU"] == res["val/mIoU"]
        tot = validation_pass(module, loader, dev, 1)
        hist = tot[2:66].reshape(8, 8).cpu().numpy()
        table = json.load(open(os.path.join(out, "eval_results.json")))
        assert [len(table[k]) for k in ("labels", "iou", "acc")] == [9, 9, 9]
        miou, ious, macc, accs = R.iou_meter(hist)
        assert np.allclose(table["iou"], list(ious) + [miou], rtol=0, atol=1e-9)
        assert np.allclose(table["acc"], list(accs) + [macc], rtol=0, atol=1e-9)
        assert len(os.listdir(os.path.join(out, "figure", "t"))) == (len(loader) + 1) // 2

        stamp = {f: os.stat(os.path.join(out, f)).st_mtime_ns for f in ("t.json", "eval_results.json")}
        assert evaluate(save_path=out, load_path=ckpt, tag="t") is None
        assert stamp == {f: os.stat(os.path.join(out, f)).st_mtime_ns for f in stamp}
    finally:
        gin.clear_config()
