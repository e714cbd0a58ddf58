"""Segmentation step logic (counterpart of the reference's co3d_3d/src/modules/segmentation_training.py:27-238
without PyTorch-Lightning): per-point logits `model(field)` (Res16UNet: `out.slice(x).F`), cross entropy
with an ignore label and an optional weight on the last ("void") class (SegLoss :27-44), and the
confusion-matrix metrics of src/utils `fast_hist` / `per_class_iu` (:115-126) accumulated on the device.

Loss, prediction, confusion matrix and the label counts of a step come out of ONE pass over the logits
(minkowski/head.py: seg_cross_entropy); the metrics below only do arithmetic on that pass's C x C histogram."""
import math

import numpy as np
import torch

from nerf_downstream_amd import gin_lite as gin
from nerf_downstream_amd.minkowski.head import seg_cross_entropy, seg_stats

EPS = 1e-10


@torch.no_grad()
def confusion(pred, label, n):
    """hist[label, pred] over the points with 0 <= label < n (reference fast_hist)."""
    k = (label >= 0) & (label < n)
    return torch.bincount(n * label[k] + pred[k], minlength=n * n).reshape(n, n)


def iou_metrics(hist):
    """-> (mIoU, mAcc, OA) in percent; classes that never occur (no label, no prediction) do not count."""
    hist = hist.double()
    tp, rows, cols = hist.diag(), hist.sum(1), hist.sum(0)
    seen = (rows + cols) > 0
    iou = tp / (rows + cols - tp + EPS)
    acc = tp / (rows + EPS)
    has = rows > 0
    miou = float(iou[seen].mean()) if bool(seen.any()) else 0.0
    macc = float(acc[has].mean()) if bool(has.any()) else 0.0
    return 100.0 * miou, 100.0 * macc, 100.0 * float(tp.sum() / (hist.sum() + EPS))


def per_class_metrics(hist, void_last=False):
    """-> {"iou": [C], "acc": [C], "miou", "macc"} in percent, with the convention of the reference's IoUMeter.compute
    (src/metrics.py:41-58), the one its eval_results.json table is made with: a class without a single ground-truth
    point scores 0 for both and STILL counts in the means; with a void class (`void_last`) the last entry is left out
    of the means.  `iou_metrics` above is the training-log convention (reference utils per_class_iu / the per-batch
    mIoU): it drops the classes that never occur, which suits a batch that holds a few of the classes; an evaluation
    over the whole validation split reports every class of the benchmark, hence both exist."""
    hist = torch.as_tensor(hist).double()
    tp, seen, positive = hist.diag(), hist.sum(1), hist.sum(0)
    has = seen > 0
    one = torch.ones_like(tp)
    iou = torch.where(has, tp / torch.where(has, seen + positive - tp, one), 0 * tp)
    acc = torch.where(has, tp / torch.where(has, seen, one), 0 * tp)
    k = iou.numel() - 1 if void_last else iou.numel()
    return {"iou": (100.0 * iou).tolist(), "acc": (100.0 * acc).tolist(),
            "miou": 100.0 * float(iou[:k].mean()), "macc": 100.0 * float(acc[:k].mean())}


def refuse_instance_head(model, who):
    """The *Ins networks return (offsets, logits); the reference holds no loss for the offsets, so nothing here trains or
    scores them.  Refused where the model is handed over, not later on the tuple."""
    if getattr(getattr(model, "module", model), "INSSEG", False):
        raise ValueError(f"{who}: {type(getattr(model, 'module', model)).__name__} is an instance-segmentation variant (INSSEG): its "
                         "forward returns (offsets, logits) and there is no loss for the offsets; use the network without `Ins`")


@gin.configurable
class SegmentationTraining:
    monitor = "val/mIoU"

    def __init__(self, model, ignore_label=255, void_weight=None):
        refuse_instance_head(model, "SegmentationTraining")
        self.model,self.ignore_label, self.void_weight = model, ignore_label, void_weight
        self._weight = None
        self._last = None  # (logits, hist, stats) of the last loss(): what train_metrics reads at a log step
        self.keep_val_logits, self.last_val = False, None  # (co3d_3d/eval.py --visualize: the last validation batch's logits, labels)

    def forward(self, batch_or_field):
        x = batch_or_field if hasattr(batch_or_field, "sparse") else self.model.process_input(batch_or_field)
        return self.model(x)

    def _class_weight(self, logits):
        if self.void_weight is None or not self.void_weight > 0:
            return None
        # reference SegLoss: weight[-1] = void_weight
        if self._weight is None or self._weight.device != logits.device or self._weight.numel() != logits.shape[1]:
            self._weight = torch.ones(logits.shape[1], device=logits.device)
            self._weight[-1] = self.void_weight
        return self._weight

    def loss(self, logits, labels):
        """Cross entropy with the ignore label and the void-class weight; the confusion matrix and the label counts of the
        same pass stay on the module (on the device, no synchronisation) for train_metrics."""
        loss, _, hist, stats = seg_cross_entropy(logits, labels, weight=self._class_weight(logits), ignore_index=self.ignore_label,
                                                 want_hist=True)
        self._last = (logits.detach(), hist, stats)
        return loss

    def training_step(self, batch, field=None):
        self._last = None
        x = field if field is not None else self.model.process_input(batch)
        if hasattr(x, "materialise"):  # (a deferred augmented batch not yet through finish_input)
            x = x.materialise()
        rows = getattr(x, "source_rows", None)
        if rows is not None:  # augmented on the device: the field holds the surviving rows, in this order
            batch["source_rows"] = rows
        row_labels = getattr(x, "row_labels", None)
        if row_labels is not None:  # point cloud prepared on the device: the voted class of every row of the field
            batch["row_labels"] = row_labels
        out = self.forward(x)
        return self.loss(out, self.labels(batch)), out

    @staticmethod
    def labels(batch):
        """The labels of the rows the model saw: those the field carried (`row_labels`: point clouds, voted per voxel),
        gathered by `source_rows` when the batch was augmented on the device (crop and dropout remove rows), the batch's
        own labels otherwise."""
        if "row_labels" in batch:
            return batch["row_labels"].long()
        labels = batch["labels"].long()
        rows = batch.get("source_rows")
        return labels if rows is None else labels[rows.long()]

    @staticmethod
    def check_finite(loss_float):
        if not np.isfinite(loss_float):
            raise ValueError(f"Invalid loss: {loss_float}")

    @staticmethod
    def _refuse_bad_labels(n_bad, classes, ignore_label):
        if n_bad:
            raise ValueError(f"{int(n_bad)} labels are neither the ignore label ({ignore_label}) nor in [0, {classes}): "
                             "they were left out of the loss; fix the dataset's label map")

    @torch.no_grad()
    def train_metrics(self, out, batch):
        """Metrics of a training step at a log step.  `out` being the logits the last loss() saw (the usual case: the
        trainer hands back training_step's output), its confusion matrix and counts are reused; anything else is run
        through the same kernel once."""
        last = self._last
        if last is not None and last[0].data_ptr() == out.data_ptr() and last[0].shape == out.shape:
            hist, stats = last[1], last[2]
        else:
            _, _, hist, stats = seg_cross_entropy(out, self.labels(batch), ignore_index=self.ignore_label, want_hist=True)
        st = seg_stats(stats)
        self._refuse_bad_labels(st["n_bad"], out.shape[1], self.ignore_label)
        miou, macc, oa = iou_metrics(hist)
        # the share of ignored rows as the fp32 mean of a 0 / 1 mask gives it: count * (1 / N), both roundings in fp32
        ratio = float(np.float32(st["n_ignored"]) * (np.float32(1.0) / np.float32(max(out.shape[0], 1))))
        return {"train/mIoU": miou, "train/mAcc": macc, "train/OA": oa, "train/ignore_ratio": 100.0 * ratio}

    @torch.no_grad()
    def val_accumulate(self, batch):
        """-> float64 vector [loss * points, points, confusion matrix..., bad labels] that validate() sums over batches and
        ranks; nothing is read back to the host here."""
        x = self.model.process_input(batch)
        if hasattr(x, "materialise"):
            x = x.materialise()
        row_labels = getattr(x, "row_labels", None)  # (point clouds: the metrics are taken over the representatives)
        logits = self.forward(x)
        labels = batch["labels"] if row_labels is None else row_labels
        if self.keep_val_logits:
            self.last_val = (logits, labels)
        return self.val_vector(logits, labels)

    def val_vector(self, logits, labels):
        loss, _, hist, stats = seg_cross_entropy(logits, labels, weight=self._class_weight(logits), ignore_index=self.ignore_label,
                                                 want_hist=True)
        n = stats[2:3].double()  # valid rows
        loss_n = torch.where(n > 0, loss.detach().double().reshape(1) * n, torch.zeros_like(n))  # (nothing valid: loss is NaN)
        return torch.cat([loss_n, n, hist.double().flatten(), stats[4:5].double()])

    def val_metrics(self, tot):
        """`tot`: the summed val_accumulate vectors: [loss * points, points, C * C confusion matrix] and, optionally, the
        count of bad labels as one more element."""
        n = max(float(tot[1]), 1.0)
        c = math.isqrt(tot.numel() - 2)
        if tot.numel() - 2 - c * c == 1:
            self._refuse_bad_labels(float(tot[-1]), c, self.ignore_label)
        miou, macc, oa = iou_metrics(tot[2:2 + c * c].reshape(c, c))
        return {"val/loss": float(tot[0]) / n, "val/mIoU": miou, "val/mAcc": macc, "val/OA": oa}
