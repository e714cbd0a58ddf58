"""float64 numpy restatement of the segmentation tail (csrc/seghead.hip, modules/segmentation_training.py): weighted /
ignore-label mean cross entropy and its gradient, first-index argmax, the reference's `fast_hist`, `IoUMeter.compute`,
and the seeded inputs the CPU and GPU tests share."""
import numpy as np


def classify(labels, C, ignore):
    """-> (valid, ignored, bad) boolean masks."""
    y = np.asarray(labels).astype(np.int64)
    ignored = y == ignore
    valid = (y >= 0) & (y < C) & ~ignored
    return valid, ignored, ~valid & ~ignored


def ce(z, labels, weight=None, ignore=-100):
    """-> dict(loss, num, den, lse[N], grad[N, C]) in float64; bad labels are left out like ignored ones; den == 0 gives
    loss NaN and a zero gradient (the documented deviation from torch, which writes NaN)."""
    z = np.asarray(z, dtype=np.float64)
    n, C = z.shape
    valid, _, _ = classify(labels, C, ignore)
    w = np.ones(C) if weight is None else np.asarray(weight, dtype=np.float64)
    mx = z.max(1)
    lse = mx + np.log(np.exp(z - mx[:, None]).sum(1))
    y = np.where(valid, np.asarray(labels).astype(np.int64), 0)
    wy = np.where(valid, w[y], 0.0)
    with np.errstate(invalid="ignore"):
        num = float(np.where(valid, wy * (lse - z[np.arange(n), y]), 0.0).sum())  # (a row left out contributes 0, whatever it holds)
    den = float(wy.sum())
    with np.errstate(invalid="ignore", divide="ignore"):
        loss = np.float64(num) / np.float64(den)
    onehot = np.zeros_like(z)
    onehot[np.arange(n), y] = 1.0
    with np.errstate(invalid="ignore"):
        grad = np.where(valid[:, None], (wy / den)[:, None] * (np.exp(z - lse[:, None]) - onehot), 0.0) if den != 0 else np.zeros_like(z)
    return {"loss": float(loss), "num": num, "den": den, "lse": lse, "grad": grad, "wy": wy}


def argmax_first(z):
    return np.argmax(np.asarray(z), axis=1)  # numpy returns the first of equal maxima


def fast_hist(pred, labels, C, ignore=-100):
    """hist[label, pred] over the valid rows."""
    valid, _, _ = classify(labels, C, ignore)
    y = np.asarray(labels).astype(np.int64)[valid]
    return np.bincount(C * y + np.asarray(pred).astype(np.int64)[valid], minlength=C * C).reshape(C, C)


def iou_meter(hist, void_last=False):
    """The reference's IoUMeter.compute on a confusion matrix, in percent -> (miou, ious, macc, accs)."""
    hist = np.asarray(hist, dtype=np.float64)
    C = hist.shape[0]
    seen, correct, positive = hist.sum(1), np.diag(hist), hist.sum(0)
    ious, accs = np.zeros(C), np.zeros(C)
    for i in range(C):
        if seen[i] != 0:
            ious[i] = correct[i] / (seen[i] + positive[i] - correct[i])
            accs[i] = correct[i] / seen[i]
    k = C - 1 if void_last else C
    return 100 * ious[:k].mean(), 100 * ious, 100 * accs[:k].mean(), 100 * accs


def segment_sum(dy, inverse, n_rows):
    out = np.zeros((n_rows, dy.shape[1]), dtype=np.float64)
    np.add.at(out, np.asarray(inverse).astype(np.int64), np.asarray(dy, dtype=np.float64))
    return out


def make_case(n, C, seed, ignore=255, weighted=False, ties=False, bad=0):
    """Logits ~ N(0, 3^2) clipped to +-16 (fp32), 5 % of the labels set to the ignore label, weights None or ones with the
    last class at 0.3; `ties`: two equal maxima in 1 % of the rows; `bad`: that many labels set to C + 5."""
    rng = np.random.default_rng(seed)
    z = np.clip(rng.normal(0.0, 3.0, (n, C)), -16.0, 16.0).astype(np.float32)
    labels = rng.integers(0, C, n).astype(np.int64)
    labels[rng.random(n) < 0.05] = ignore
    if ties and n >= 100:
        rows = rng.choice(n, n // 100, replace=False)
        a = rng.integers(0, C, rows.size)
        b = (a + 1 + rng.integers(0, C - 1, rows.size)) % C
        top = z[rows].max(1) + np.float32(1.0)
        z[rows, a], z[rows, b] = top, top
    if bad:
        labels[rng.choice(n, bad, replace=False)] = C + 5
    w = None
    if weighted:
        w = np.ones(C, dtype=np.float32)
        w[-1] = np.float32(0.3)
    return z, labels, w
