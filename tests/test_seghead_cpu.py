"""CPU: the segmentation tail's host side -- argument validation of the new C entry points (no GPU: every check comes
before the first launch), the torch fallback of seg_cross_entropy against F.cross_entropy, per_class_metrics against the
float64 restatement, and co3d_3d/eval.py run on the host with the oracle namespace injected."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import seghead_restate as R
from nerf_downstream_amd import gin_lite as gin

CFG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "nerf_downstream_amd", "co3d_3d", "configs")
P = 0x10000  # aligned, never dereferenced


@pytest.fixture(autouse=True)
def _clean_gin():
    gin.clear_config()
    yield
    gin.clear_config()


def test_argument_validation_without_gpu():
    from nerf_downstream_amd import _lib

    L = _lib.lib()
    n, C = 1000, 20
    need = L.mink_seg_ce_workspace_bytes(n, C)
    assert need > 0 and L.mink_seg_ce_workspace_bytes(1_200_000, 21) >= need
    assert L.mink_seg_ce_workspace_bytes(n, 1) == -1 and L.mink_seg_ce_workspace_bytes(0, C) > 0
    fwd = lambda z=P, ldz=C, lab=P, w=None, n=n, C=C, lse=P, stats=P, loss=P, ws=P, wsb=need: L.mink_seg_ce_forward(  # noqa: E731
        z, ldz, lab, 1, w, 255, n, C, lse, None, None, stats, loss, ws, wsb, None)
    assert fwd(z=None) == -1 and b"NULL" in L.mink_last_error()
    assert fwd(stats=None) == -1 and b"NULL" in L.mink_last_error()
    assert fwd(C=1, ldz=1) == -1 and b"C=1" in L.mink_last_error()
    assert fwd(C=4096, ldz=4096) == -1
    assert fwd(ldz=C - 1) == -1 and b"bad shape" in L.mink_last_error()
    assert fwd(z=P + 2) == -1 and b"misaligned" in L.mink_last_error()
    assert fwd(lab=P + 4) == -1 and b"misaligned" in L.mink_last_error()  # int64 labels want 8 bytes
    assert fwd(wsb=need - 1) == -1
    assert b"workspace" in L.mink_last_error() and str(need).encode() in L.mink_last_error()
    bwd = lambda z=P, C=C, dz=P: L.mink_seg_ce_backward(z, C, P, 0, None, 255, P, P, P, n, C, dz, None)  # noqa: E731
    assert bwd(dz=None) == -1 and b"NULL" in L.mink_last_error()
    assert bwd(C=1) == -1 and bwd(z=P + 1) == -1
    assert L.mink_rows_gather(None, 20, 10, 20, P, 10, P, None) == -1 and b"NULL" in L.mink_last_error()
    assert L.mink_rows_gather(P, 19, 10, 20, P, 10, P, None) == -1 and b"bad shape" in L.mink_last_error()
    assert L.mink_segment_sum(P, 21, 21, None, P, 10, P, None) == -1 and b"NULL" in L.mink_last_error()
    assert L.mink_segment_sum(P, 21, 0, P, P, 10, P, None) == -1
    assert L.mink_rows_gather(P, 20, 10, 20, P, 0, P, None) == 0  # nothing to do: no launch


@pytest.mark.parametrize("weighted", [False, True])
def test_cpu_front_door_equals_torch(weighted):
    from nerf_downstream_amd import minkowski as ME
    from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import confusion
    from nerf_downstream_amd.minkowski.functional import seg_stats

    z, labels, w = R.make_case(4097, 13, seed=3, weighted=weighted)
    zt = torch.from_numpy(z).requires_grad_(True)
    yt, wt = torch.from_numpy(labels), None if w is None else torch.from_numpy(w)
    loss, pred, hist, stats = ME.seg_cross_entropy(zt, yt, weight=wt, ignore_index=255, want_pred=True, want_hist=True)
    want = F.cross_entropy(zt, yt, weight=wt, ignore_index=255)
    assert loss.item() == want.item()
    g, = torch.autograd.grad(loss, zt)
    g0, = torch.autograd.grad(want, zt)
    assert torch.equal(g, g0)
    assert torch.equal(pred.long(), zt.argmax(1)) and torch.equal(hist, confusion(zt.argmax(1), yt, 13))
    assert np.array_equal(hist.numpy(), R.fast_hist(R.argmax_first(z), labels, 13, 255))
    st, ref = seg_stats(stats), R.ce(z, labels, w, 255)
    valid, ignored, bad = R.classify(labels, 13, 255)
    assert (st["n_valid"], st["n_ignored"], st["n_bad"]) == (valid.sum(), ignored.sum(), 0)
    assert abs(st["den"] - ref["den"]) < 1e-9 * ref["den"] and abs(loss.item() - ref["loss"]) < 1e-5
    assert ME.MinkowskiFunctional.seg_cross_entropy is ME.seg_cross_entropy
    # bad labels never reach torch's kernel on this path either: counted, left out
    z, labels, w = R.make_case(500, 8, seed=4, bad=3)
    loss, _, hist, stats = ME.seg_cross_entropy(torch.from_numpy(z), torch.from_numpy(labels).int(), ignore_index=255, want_hist=True)
    assert seg_stats(stats)["n_bad"] == 3 and abs(loss.item() - R.ce(z, labels, None, 255)["loss"]) < 1e-5
    assert np.array_equal(hist.numpy(), R.fast_hist(R.argmax_first(z), labels, 8, 255))


def test_per_class_metrics_match_the_restatement():
    from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import SegmentationTraining, iou_metrics, per_class_metrics

    #            pred: 0  1  2  3
    hist = np.array([[5, 1, 0, 0],   # class 0
                     [2, 3, 0, 1],   # class 1
                     [0, 0, 0, 0],   # class 2: never seen in the ground truth, predicted once below
                     [0, 0, 1, 4]])  # class 3 (the void class in the second case)
    for void_last in (False, True):
        got = per_class_metrics(torch.from_numpy(hist), void_last=void_last)
        miou, ious, macc, accs = R.iou_meter(hist, void_last=void_last)
        assert np.allclose(got["iou"], ious, rtol=0, atol=1e-12) and np.allclose(got["acc"], accs, rtol=0, atol=1e-12)
        assert abs(got["miou"] - miou) < 1e-12 and abs(got["macc"] - macc) < 1e-12
    got = per_class_metrics(hist)
    assert got["iou"][2] == 0.0 and got["acc"][2] == 0.0  # the never-seen class scores 0 ...
    assert got["iou"][0] == pytest.approx(100 * 5 / 8) and got["miou"] == pytest.approx(100 * (5 / 8 + 3 / 7 + 0 + 4 / 6) / 4)  # ... and counts
    assert per_class_metrics(hist, void_last=True)["miou"] == pytest.approx(100 * (5 / 8 + 3 / 7 + 0) / 3)
    assert iou_metrics(torch.from_numpy(hist))[0] == pytest.approx(100 * (5 / 8 + 3 / 7 + 0 + 4 / 6) / 4)  # (class 2 was predicted: it counts there too)
    hist[3, 2] = 0
    assert iou_metrics(torch.from_numpy(hist))[0] == pytest.approx(100 * (5 / 8 + 3 / 7 + 4 / 5) / 3)  # now absent: dropped there ...
    assert per_class_metrics(hist)["miou"] == pytest.approx(100 * (5 / 8 + 3 / 7 + 0 + 4 / 5) / 4)  # ... kept here

    # val_metrics accepts the present vector layout and the one that carries the bad-label count; a non-zero count raises
    m = SegmentationTraining(model=None, ignore_label=255)
    base = torch.cat([torch.tensor([3.0, 6.0], dtype=torch.float64), torch.from_numpy(hist).double().flatten()])
    a, b = m.val_metrics(base), m.val_metrics(torch.cat([base, torch.zeros(1, dtype=torch.float64)]))
    assert a == b and a["val/loss"] == 0.5
    with pytest.raises(ValueError, match=r"2 labels.*\[0, 4\)"):
        m.val_metrics(torch.cat([base, torch.tensor([2.0], dtype=torch.float64)]))
    z, labels, _ = R.make_case(300, 8, seed=5, bad=3)
    with pytest.raises(ValueError, match="3 labels"):
        m.train_metrics(torch.from_numpy(z), {"labels": torch.from_numpy(labels)})


def test_eval_cli_arguments():
    from nerf_downstream_amd.co3d_3d import eval as E

    p = E.build_parser()
    a = p.parse_args(["--ginc", "a.gin", "--ginc", "b.gin", "--ginb", "x.y=1", "--load_path", "r/run/last.ckpt", "--tag", "t",
                      "--replace", "--visualize", "--seed", "3", "--training_module", "SegmentationTraining", "--save_path", "out"])
    assert a.ginc == ["a.gin", "b.gin"] and a.ginb == ["x.y=1"] and a.replace and a.visualize and a.seed == 3 and a.tag == "t"
    assert E.refused_options(a) == []
    for flags, name in ((["--sparsify"], "sparsify"), (["--convert_powernorm"], "convert_powernorm"), (["--profile"], "profile"),
                        (["--device", "cpu"], "device cpu"), (["--layout", "csr"], "layout"), (["--sparse_mode", "1,1"], "sparse_mode")):
        assert E.refused_options(p.parse_args(flags + ["--load_path", "x"])) == [name]
        assert E.main(flags + ["--load_path", "x"]) == 2


def test_eval_on_the_host_with_the_oracle(tmp_path, capsys):
    """train 3 steps with the CPU oracle backend, evaluate last.ckpt: <tag>.json carries validate()'s metrics on the same
    weights, eval_results.json the reference's table layout; a second call without --replace touches nothing."""
    from nerf_downstream_amd.co3d_3d.eval import evaluate
    from nerf_downstream_amd.co3d_3d.src.data.data_module import DataModule
    from nerf_downstream_amd.co3d_3d.src.models import get_model
    from nerf_downstream_amd.co3d_3d.train import TRAINING_MODULES, load_checkpoint, train, validate, validation_pass
    from oracle import me_cpu as OME

    gin.parse_config_files_and_bindings(
        [f"{CFG}/co3d_cls.gin", f"{CFG}/synthetic_seg.gin", f"{CFG}/res16unet.gin"],
        ["train.gpus=0", "train.max_steps=3", "train.val_every_n_steps=3", "train.log_every_n_steps=1", "train.batch_size=2",
         "train.val_batch_size=2", "SparseVoxelSegDataset.grid=16", "SparseVoxelSegDataset.num_samples=8", "train.lr=0.01"],
    )
    train(save_path=str(tmp_path), resume_training=False, run_name="s", run_name_postfix=None, ME=OME)
    ckpt, out = str(tmp_path / "s" / "last.ckpt"), str(tmp_path / "eval")
    res = evaluate(save_path=out, load_path=ckpt, tag="t", visualize=True, ME=OME)
    assert sorted(res) == ["val/OA", "val/loss", "val/mAcc", "val/mIoU"]
    assert json.load(open(os.path.join(out, "t.json"))) == res

    model = get_model(ME=OME)
    load_checkpoint(ckpt, model, weights_only=True)
    module = TRAINING_MODULES["SegmentationTraining"](model)
    loader = DataModule(val_batch_size=1, val_num_workers=0).val_dataloader()
    assert validate(module, loader, torch.device("cpu"), 1) == res
    tot = validation_pass(module, loader, torch.device("cpu"), 1)
    hist = tot[2:66].reshape(8, 8).numpy()
    table = json.load(open(os.path.join(out, "eval_results.json")))
    assert sorted(table) == ["acc", "iou", "labels"] and table["labels"] == [str(i) for i in range(8)] + ["mean"]
    miou, ious, macc, accs = R.iou_meter(hist)
    assert len(table["iou"]) == len(table["acc"]) == 9
    assert np.allclose(table["iou"], list(ious) + [miou], rtol=0, atol=1e-9) and np.allclose(table["acc"], list(accs) + [macc], rtol=0, atol=1e-9)
    saved = sorted(os.listdir(os.path.join(out, "figure", "t")))
    assert len(saved) == (len(loader) + 1) // 2
    blob = torch.load(os.path.join(out, "figure", "t", saved[0]), weights_only=True)
    assert sorted(blob) == ["coordinates", "labels", "logits"] and blob["logits"].shape == (blob["labels"].shape[0], 8)

    stamp = {f: os.stat(os.path.join(out, f)).st_mtime_ns for f in ("t.json", "eval_results.json")}
    capsys.readouterr()
    assert evaluate(save_path=out, load_path=ckpt, tag="t", ME=OME) is None
    assert "skip" in capsys.readouterr().out
    assert stamp == {f: os.stat(os.path.join(out, f)).st_mtime_ns for f in stamp}
    assert evaluate(save_path=out, load_path=ckpt, tag="t", replace=True, ME=OME) == res
