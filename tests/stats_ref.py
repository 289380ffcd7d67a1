"""numpy restatement of the phase-statistics tally (csrc/stats.hip, bmnas.metrics.PhaseStats) and of its read-out.

The accumulator is a vector of 4 + 3 O int64 words:
    0  the loss sum (bits of a float64)   1  tallies   2  samples   3  correct predictions
    4 + 3c, 5 + 3c, 6 + 3c                 tp, fp, fn of class c
Everything here is written from the definition, sample by sample, not by calling the functions it is compared with."""
import math

import numpy as np

HEAD = 4


def words(O):
    return HEAD + 3 * O


def empty(O):
    return np.zeros(words(O), dtype=np.int64)


def logit_threshold(th):
    """log(th / (1 - th)) in float64, rounded once to fp32 (returned as a Python float holding that fp32 value)."""
    return float(np.float32(math.log(th / (1.0 - th))))


def argmax_first(row):
    """torch's rule: a NaN is a maximum and the first NaN wins; otherwise the first of the largest values."""
    best = 0
    for i in range(1, len(row)):
        v, b = row[i], row[best]
        if np.isnan(b):
            break
        if np.isnan(v) or v > b:
            best = i
    return best


def _head(acc, loss, n):
    if loss is not None:
        term = np.float64(np.float32(loss)) * np.float64(n)          # one product ...
        total = acc[0:1].view(np.float64)[0] + term                  # ... one sum, each rounded on its own
        acc[0:1].view(np.float64)[0] = total
    acc[1] += 1
    acc[2] += n


def tally_acc(acc, logits, labels, loss):
    """logits (n, O) fp32, labels (n,) int64, loss a float (fp32 value) or None -> acc, updated in place."""
    logits = np.asarray(logits, dtype=np.float32)
    n = logits.shape[0]
    _head(acc, loss, n)
    for r in range(n):
        acc[3] += int(argmax_first(logits[r]) == int(labels[r]))
    return acc


def tally_f1(acc, logits, targets, loss, logit_thr):
    logits, targets = np.asarray(logits, dtype=np.float32), np.asarray(targets, dtype=np.float32)
    n, O = logits.shape
    _head(acc, loss, n)
    thr = np.float32(logit_thr)
    for r in range(n):
        for c in range(O):
            pred, truth = bool(logits[r, c] > thr), bool(targets[r, c] > np.float32(0.5))
            if pred and truth:
                acc[HEAD + 3 * c] += 1
            elif pred:
                acc[HEAD + 3 * c + 1] += 1
            elif truth:
                acc[HEAD + 3 * c + 2] += 1
    return acc


def loss_sum(acc):
    return float(acc[0:1].view(np.float64)[0])


def accuracy(acc, n):
    return float(acc[3]) / n


def f1(acc, f1_type):
    """f1_score(average=f1_type, zero_division=1) from the counts: per class 2 tp / (2 tp + fp + fn), 1.0 on an empty
    denominator; macro the mean, weighted by tp + fn (the plain mean when all weights are 0), micro on the summed counts."""
    counts = acc[HEAD:].astype(np.float64).reshape(-1, 3)
    tp, fp, fn = counts[:, 0], counts[:, 1], counts[:, 2]
    if f1_type == 'micro':
        tp, fp, fn = tp.sum(keepdims=True), fp.sum(keepdims=True), fn.sum(keepdims=True)
    den = 2 * tp + fp + fn
    f = np.where(den == 0, 1.0, 2 * tp / np.where(den == 0, 1, den))
    if f1_type == 'micro':
        return float(f[0])
    if f1_type == 'macro':
        return float(f.mean())
    w = tp + fn
    if w.sum() == 0:
        return float(f.mean())
    return float((f * w).sum() / w.sum())


def off_band(x, thr, band=1e-4):
    """Move the logits out of |x - thr| < band (away from the threshold, keeping their side); -> fp32 array."""
    x = np.array(x, dtype=np.float32)
    near = np.abs(x.astype(np.float64) - thr) < band
    x[near] = np.where(x[near] > thr, np.float32(thr + 4 * band), np.float32(thr - 4 * band))
    return x


def band_empty(x, thr, band=1e-4):
    x = np.asarray(x, dtype=np.float64)
    x = x[np.isfinite(x)]
    return not bool((np.abs(x - thr) < band).any())
