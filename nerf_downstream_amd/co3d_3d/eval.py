#!/usr/bin/env python3
"""Evaluation of a trained segmentation checkpoint: the counterpart of the reference's co3d_3d/eval.py (argparse
:105-135, `evaluate()` :21-101) built from this trainer's pieces, without PyTorch-Lightning:

    python -m nerf_downstream_amd.co3d_3d.eval --ginc nerf_downstream_amd/co3d_3d/configs/scannet_plenoxel.gin \
        --ginc nerf_downstream_amd/co3d_3d/configs/res16unet.gin --load_path experiments/run/last.ckpt --tag run

One validation pass with batches of one scene, the confusion matrix accumulated on the device, then
  <save_path>/<tag>.json          the `val/*` metrics of train.validate,
  <save_path>/eval_results.json   {"labels": [class names..., "mean"], "iou": [per class..., mean], "acc": [...]} in percent,
                                  the table every ScanNet paper reports (reference IoUMeter.compute convention; classes in
                                  index order),
and, with --visualize, <save_path>/figure/<tag>/<scene>.pth (coordinates, logits, labels) for every second batch.
An existing <tag>.json is kept unless --replace is given.

Pruned checkpoints (reference eval.py:49-83): when a state-dict key contains `_mask` the prunable parameters are identity-pruned
so the `*_orig` / `*_mask` pairs load, the `num_params, total=..., net=..., ratio=...` line is printed, the masks are made
permanent and every module that has `sparsify` is sparsified with `evaluate.layout` ("csr", "coo" or "strided"); <tag>.json then
also carries `val/total_params`, `val/pruned_params` and `val/gflops`.  The weight-sparse layers come from the binding the
reference's `--sparsify --sparse_mode 1,1,1,1,1,1,1,1,1` boils down to:

        --ginb "get_model.sparse=[1,1,1,1,1,1,1,1,1]" --ginb "evaluate.layout='csr'"

PowerNorm (the reference declares --convert_powernorm and never uses it): the binding

        --ginb "evaluate.convert_powernorm=True"

turns every batch norm of the model into a MinkowskiPowerNorm, before the checkpoint is loaded when it was trained with PN
layers, after it for a batch-norm checkpoint.

The command-line flags --sparsify / --sparse_mode / --layout / --convert_powernorm themselves, and the reference's
--device cpu / --profile options, are refused here."""
import argparse
import json
import logging
import os
import sys
import time

import numpy as np
import torch

from nerf_downstream_amd import gin_lite as gin
from nerf_downstream_amd.co3d_3d import train as T
from nerf_downstream_amd.co3d_3d.src.data.data_module import DataModule
from nerf_downstream_amd.co3d_3d.src.models import get_model
from nerf_downstream_amd.co3d_3d.src.modules.segmentation_training import per_class_metrics, refuse_instance_head
from nerf_downstream_amd.co3d_3d.src.utils import prune as P

logger = logging.getLogger(__name__)

OUT_OF_SCOPE = ("convert_powernorm", "sparsify", "sparse_mode", "layout", "profile", "device")
SPARSE_HINT = ("a pruned checkpoint is evaluated through gin bindings, not through --sparsify / --sparse_mode / --layout: "
               "--ginb \"get_model.sparse=[1,1,1,1,1,1,1,1,1]\" --ginb \"evaluate.layout='csr'\"")
POWERNORM_HINT = ("PowerNorm is reached through a gin binding, not through --convert_powernorm: "
                  "--ginb \"evaluate.convert_powernorm=True\" (training: --ginb \"train.convert_powernorm=True\")")


def _gin_or(name, default):
    try:
        return gin.query_parameter(name)
    except gin.GinError:
        return default


def _scene_name(batch, index):
    meta = batch.get("metadata")
    if meta and isinstance(meta[0], dict) and meta[0].get("file"):
        return os.path.splitext(os.path.basename(str(meta[0]["file"])))[0]
    return f"{index:06d}"


@gin.configurable
def evaluate(save_path, load_path, training_module: str = "SegmentationTraining", tag="default", visualize=False, replace=False,
             val_phase="val", val_num_workers=None, ME=None, device=None, seed: int = 777, layout="csr", convert_powernorm=False):
    """-> the `val/*` dict written to <save_path>/<tag>.json, or None when that file exists and `replace` is not set.
    `ME` / `device` are test hooks, as in train(): the CPU tests inject the oracle namespace.  `layout`: what `sparsify()` is
    called with when the checkpoint is a pruned one ("csr" / "coo": the sparse kernel, "strided": the dense one on the masked
    weights).  `convert_powernorm` (`--ginb "evaluate.convert_powernorm=True"`): every batch norm becomes a MinkowskiPowerNorm
    -- before the checkpoint is loaded when its keys contain `.pn.running_phi` (a checkpoint trained with PN layers), after it
    otherwise (a batch-norm checkpoint evaluated as PN: `running_var` becomes `running_phi`)."""
    os.makedirs(save_path, exist_ok=True)
    json_path = os.path.join(save_path, f"{tag}.json")
    if not replace and os.path.isfile(json_path):
        print(f"====== skip existing experiment ({json_path}; --replace to run it again) =====")
        return None
    if device is None:
        if ME is None and not torch.cuda.is_available():
            raise RuntimeError("co3d_3d.eval needs a GPU: the HIP backend has no CPU fallback")
        device = torch.device("cuda", 0) if ME is None else torch.device("cpu")
    if device.type == "cuda":
        torch.cuda.set_device(device)
    if training_module != "SegmentationTraining":
        raise ValueError(f"evaluate.training_module = {training_module!r}: only SegmentationTraining has an evaluation table")
    torch.manual_seed(seed)
    model = (get_model(ME=ME) if ME is not None else get_model()).to(device)
    refuse_instance_head(model, "co3d_3d.eval")
    keys = list(T.load_checkpoint_file(load_path)["state_dict"])
    is_pruned = any("_mask" in k for k in keys)
    pn_checkpoint = any(".pn.running_phi" in k for k in keys)
    if convert_powernorm and pn_checkpoint:
        model = T.to_powernorm(model, ME)
    if is_pruned:  # identity pruning gives every prunable parameter the `_orig` / `_mask` pair the checkpoint holds
        logger.info("received checkpoint of pruned network")
        to_prune = P.get_parameters_to_prune(model)
        P.register_prune_buffers(to_prune)
    T.load_checkpoint(load_path, model, weights_only=True)  # tensors and plain containers only: nothing from the file is executed
    if convert_powernorm and not pn_checkpoint:
        model = T.to_powernorm(model, ME)
    sparsified = False
    if is_pruned:
        num = P.count_parameters(model)
        net = num["total"] - num["pruned"]
        print(f"num_params, total={num['total']}, net={net}, ratio={net / num['total'] * 100:.2f}")
        P.remove(to_prune)  # the pruned state becomes permanent: the zeros are in the parameters
        for _, m in model.named_modules():
            if hasattr(m, "sparsify"):
                m.sparsify(layout)
                sparsified = True
    model.eval()
    workers = val_num_workers if val_num_workers is not None else _gin_or("train.val_num_workers", 0)
    data = DataModule(val_batch_size=1, val_phase=val_phase, val_num_workers=workers)
    module = T.TRAINING_MODULES[training_module](model)
    loader = data.val_dataloader()

    on_batch = None
    if visualize:
        fig_dir = os.path.join(save_path, "figure", str(tag))
        os.makedirs(fig_dir, exist_ok=True)
        module.keep_val_logits = True

        def on_batch(i, batch):
            if i % 2 == 0:
                logits, labels = module.last_val
                path = os.path.join(fig_dir, _scene_name(batch, i) + ".pth")
                torch.save({"coordinates": batch["coordinates"].cpu(), "logits": logits.cpu(), "labels": labels.cpu()}, path)
                logger.info(f"saved {path}")

    t0 = time.time()
    tot = T.validation_pass(module, loader, device, 1, on_batch=on_batch)
    module.keep_val_logits, module.last_val = False, None
    results = module.val_metrics(tot)
    if sparsified:
        results["val/total_params"], results["val/pruned_params"] = num["total"], num["pruned"]
        results["val/gflops"] = P.count_flops(model)  # of the last scene's forward pass
    elapsed = time.time() - t0
    logger.info(f"elapsed time: {elapsed:.2f} s, iter time: {elapsed / max(len(loader), 1):.4f} s")

    c = int(np.sqrt(tot.numel() - 2))
    hist = tot[2:2 + c * c].reshape(c, c).cpu()
    ds = data.val_dataset
    names = list(getattr(ds, "CLASS_LABELS", None) or [])
    names = [str(x) for x in names] if len(names) == c else [str(i) for i in range(c)]
    void_label = getattr(ds, "void_label", None)
    void_last = void_label is not None and void_label != getattr(ds, "ignore_label", void_label)
    pc = per_class_metrics(hist, void_last=void_last)
    print(" & ".join(names))
    print(" & ".join(f"{v:.1f}" for v in pc["iou"]))
    print(f"miou: {pc['miou']}\nmacc: {pc['macc']}")
    with open(os.path.join(save_path, "eval_results.json"), "w") as f:
        json.dump({"labels": names + ["mean"], "iou": pc["iou"] + [pc["miou"]], "acc": pc["acc"] + [pc["macc"]]}, f)
    with open(json_path, "w") as f:
        json.dump(results, f, indent=4)
    return results


def build_parser():
    p = argparse.ArgumentParser()
    p.add_argument("--ginc", action="append", help="gin config file")
    p.add_argument("--ginb", action="append", help="gin bindings")
    p.add_argument("--training_module", type=str, default="SegmentationTraining")
    p.add_argument("--save_path", type=str, default=None, help="path to save results (default: the checkpoint's directory)")
    p.add_argument("--load_path", type=str, default=None, help="path to learned weights")
    p.add_argument("--device", type=str, choices=["cpu", "cuda"], default="cuda")
    p.add_argument("--seed", type=int, default=777)
    p.add_argument("--convert_powernorm", action="store_true")
    p.add_argument("--sparsify", action="store_true")
    p.add_argument("--sparse_mode", type=str, default=None)
    p.add_argument("--debug", action="store_true")
    p.add_argument("--visualize", action="store_true")
    p.add_argument("--replace", action="store_true")
    p.add_argument("--profile", action="store_true")
    p.add_argument("--layout", type=str, choices=["csr", "coo", "strided"], default=None)
    p.add_argument("--tag", type=str)
    return p


def refused_options(args):
    """Names of the reference's options that were given and are out of scope here."""
    given = [k for k in OUT_OF_SCOPE if k != "device" and getattr(args, k) not in (None, False)]
    return given + (["device cpu"] if args.device == "cpu" else [])


def main(argv=None):
    args = build_parser().parse_args(argv)
    bad = refused_options(args)
    if bad:
        print("out of scope here (the reference's pruning / sparse-layout / profiling study): --" + ", --".join(bad), file=sys.stderr)
        if any(b in ("sparsify", "sparse_mode", "layout") for b in bad):
            print(SPARSE_HINT, file=sys.stderr)
        if "convert_powernorm" in bad:
            print(POWERNORM_HINT, file=sys.stderr)
        return 2
    if not args.load_path:
        print("--load_path is required", file=sys.stderr)
        return 2
    T.setup_logger(f"eval_{args.seed}", args.debug)
    logging.info(f"Gin configuration files: {args.ginc}")
    logging.info(f"Gin bindings: {args.ginb or []}")
    np.random.seed(args.seed)
    gin.parse_config_files_and_bindings(args.ginc, args.ginb or [])
    tag = args.tag if args.tag is not None else f"{os.path.basename(os.path.dirname(os.path.abspath(args.load_path)))}-cuda-False"
    save_path = args.save_path if args.save_path is not None else os.path.dirname(os.path.abspath(args.load_path))
    evaluate(save_path=save_path, load_path=args.load_path, training_module=args.training_module, tag=tag,
             visualize=args.visualize, replace=args.replace, seed=args.seed)
    return 0


if __name__ == "__main__":
    sys.exit(main())
