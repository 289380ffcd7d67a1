"""Phase statistics of the trainer loop on the device: loss sum, accuracy and F1 counts, one launch per batch.

`PhaseStats` keeps what the loop's `loss_sum += loss.double() * n` and its AccuracyMeter / F1Meter keep, in ONE persistent
device accumulator of 64-bit words that a single launch (csrc/stats.hip: bmnas_phase_stats_acc / _f1) tallies a batch
into — eagerly behind a step, or as the last node of a captured forward (bmnas.graph.GraphedForward(stats=...)), where a
replay then tallies its own batch with no host call at all.  Nothing grows with the length of the phase: F1 comes from
per-class counts, not from the kept predictions.

Accumulator (int64, 4 + 3 O words; all-zero is the empty tally):
    word 0   the loss sum, the bits of a float64        word 2   samples tallied
    word 1   tallies (launches)                          word 3   correct predictions            ('acc')
    words 4 + 3c, 5 + 3c, 6 + 3c   tp, fp, fn of class c                                         ('f1')

The one stated difference from F1Meter: the threshold.  F1Meter predicts `sigmoid(x) > th` in fp32; here the
threshold is moved to the logit once, logit_threshold = log(th / (1 - th)) computed in float64 on the host and rounded to
fp32, and an element is predicted positive when `x > logit_threshold` (strict).  The two agree except for a logit within
about 1e-6 of the threshold, where fp32 sigmoid's rounding decides the first and the logit itself the second.

F1 from counts is sklearn's `f1_score(..., zero_division=1)`: per class f = 2 tp / (2 tp + fp + fn), 1.0 where the
denominator is 0; 'macro' the mean, 'weighted' the mean with weights tp + fn (the plain mean when all are 0), 'micro' the
same formula on the summed counts.  'samples' is no function of the counts and is refused.  A one-column target is read
differently by sklearn (as a binary problem): kind 'f1' needs O >= 2.
"""
import math

import numpy as np
import torch

from .lib import BmnasError

HEAD_WORDS = 4
MAX_CLASSES = 128                            # lib.STATS_MAX_CLASSES: the fused head's class limit
F1_TYPES = ('micro', 'macro', 'weighted')


def stats_words(O):
    """Accumulator length for O classes (what bmnas_phase_stats_words returns)."""
    return HEAD_WORDS + 3 * int(O)


def logit_threshold(th):
    """The logit at which sigmoid crosses th: float64 on the host, rounded once to the fp32 the kernel compares with."""
    th = float(th)
    if not 0.0 < th < 1.0:
        raise BmnasError(f'PhaseStats: the F1 threshold must lie in (0, 1), got {th!r}')
    return float(np.float32(math.log(th / (1.0 - th))))


def f1_from_counts(tp, fp, fn, f1_type):
    """sklearn.metrics.f1_score(average=f1_type, zero_division=1) of a multilabel problem from its per-class counts."""
    tp, fp, fn = (np.asarray(a, dtype=np.float64) for a in (tp, fp, fn))
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


def _all_sum(t):
    """The loop's sum over the data-parallel ranks (float64, as AccuracyMeter's); the identity in one process."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
        from models.search.train_searchable import _loop
        return _loop._all_sum(t)
    return t


class PhaseStats:
    """kind 'acc': labels (n,) int64, compute(n) = correct / n.  kind 'f1': labels (n, O) fp32, compute(n) = F1 of
    `output > logit(threshold)` against `labels > 0.5`, f1_type in 'micro' | 'macro' | 'weighted'.

        stats = PhaseStats('f1', 'weighted', 0.3)
        stats.reset(device)                       # per phase: one memset
        stats.update(loss, output, labels)        # per batch: one launch
        stats.loss_sum(), stats.samples(), stats.compute(n)       # per phase: one device-to-host read

    update() is one native launch for contiguous fp32 device logits with labels of the kind's dtype and shape and at most
    128 classes (`launches`); any other call — other dtypes, CPU tensors, non-contiguous tensors, O > 128 — is the same
    tally written with torch ops into the same words (`_update_torch`, counted in `fallbacks`; it also works on the CPU)."""

    def __init__(self, kind, f1_type=None, threshold=None):
        if kind not in ('acc', 'f1'):
            raise BmnasError(f"PhaseStats: kind must be 'acc' or 'f1', got {kind!r}")
        self.kind = kind
        if kind == 'f1':
            f1_type = 'weighted' if f1_type is None else f1_type
            threshold = 0.3 if threshold is None else threshold
            if f1_type == 'samples':
                raise BmnasError("PhaseStats: F1 average='samples' is no function of the per-class counts "
                                 "(it needs every sample's predictions): use _loop.F1Meter")
            if f1_type not in F1_TYPES:
                raise BmnasError(f'PhaseStats: f1_type must be one of {F1_TYPES}, got {f1_type!r}')
            self.f1_type, self.threshold = f1_type, float(threshold)
            self.logit_threshold = logit_threshold(threshold)
            self.name = f'{f1_type} F1'
        else:
            if f1_type is not None or threshold is not None:
                raise BmnasError("PhaseStats: f1_type / threshold belong to kind 'f1'")
            self.f1_type = self.threshold = self.logit_threshold = None
            self.name = 'Acc'
        self.acc = None                      # the accumulator: allocated by the first update(), then only zeroed
        self.O = None
        self.device = None
        self.launches = 0
        self.fallbacks = 0
        self._host = None

    @staticmethod
    def from_meter(meter):
        """_loop.AccuracyMeter -> PhaseStats('acc'); _loop.F1Meter(f1_type, th) -> PhaseStats('f1', f1_type, th); any
        other object (a foreign meter, a subclass with an update of its own) -> None: the loop keeps the meter."""
        from models.search.train_searchable import _loop
        if type(meter) is _loop.AccuracyMeter:
            return PhaseStats('acc')
        if type(meter) is _loop.F1Meter:
            return PhaseStats('f1', meter.f1_type, meter.th)
        return None

    # ---- per phase ------------------------------------------------------------------------------------------------
    def reset(self, device):
        """An empty tally on `device`.  The accumulator keeps its address (captured launches hold it): one memset."""
        device = torch.device(device)
        if self.acc is not None:
            same = self.acc.device.type == device.type and device.index in (None, self.acc.device.index)
            if same:
                self.acc.zero_()
            else:
                self.acc = self.O = None
        self.device = device
        self._host = None

    def touch(self):
        """A captured launch has tallied behind this object's back (a GraphedForward replay): forget the host copy."""
        self._host = None

    # ---- per batch ------------------------------------------------------------------------------------------------
    def native_ok(self, loss, output, labels):
        """Whether update() of these tensors is the one native launch."""
        if not (torch.is_tensor(output) and output.dim() == 2 and output.is_cuda and output.dtype == torch.float32
                and output.is_contiguous() and output.shape[0] >= 1 and 1 <= output.shape[1] <= MAX_CLASSES):
            return False
        if not (torch.is_tensor(labels) and labels.device == output.device and labels.is_contiguous()):
            return False
        if self.kind == 'acc':
            if labels.dtype != torch.int64 or tuple(labels.shape) != (output.shape[0],):
                return False
        elif labels.dtype != torch.float32 or labels.shape != output.shape:
            return False
        return loss is None or (torch.is_tensor(loss) and loss.device == output.device
                                and loss.dtype == torch.float32 and loss.numel() == 1)

    def update(self, loss, output, labels):
        """Tally one batch: loss a 0-dim tensor (the batch mean; None: no loss term), output (n, O) logits."""
        if not (torch.is_tensor(output) and output.dim() == 2):
            raise BmnasError('PhaseStats.update: output must be an (n, O) tensor of logits')
        n, O = output.shape
        if self.kind == 'f1' and O < 2:
            raise BmnasError("PhaseStats: kind 'f1' needs O >= 2 (sklearn reads a one-column target as a binary "
                             'problem, not as one label of a multilabel one)')
        if self.acc is None:
            self.acc = torch.zeros(stats_words(O), dtype=torch.int64, device=output.device)
            self.O = O
        elif O != self.O or output.device != self.acc.device:
            raise BmnasError(f'PhaseStats.update: ({n}, {O}) logits on {output.device} into an accumulator of {self.O} '
                             f'classes on {self.acc.device}')
        self._host = None
        if self.native_ok(loss, output, labels):
            from . import lib
            if self.kind == 'acc':
                lib.phase_stats_acc(output, labels, loss, self.acc)
            else:
                lib.phase_stats_f1(output, labels, loss, self.logit_threshold, self.acc)
            self.launches += 1
        else:
            self._update_torch(loss, output, labels)
            self.fallbacks += 1

    @torch.no_grad()
    def _update_torch(self, loss, output, labels):
        """The kernels' tally with torch ops, word for word (several launches; any dtype, layout or device)."""
        acc, n = self.acc, output.shape[0]
        output, labels = output.detach(), labels.detach().to(acc.device)
        if loss is not None:
            # (fp32 -> float64, one product, one sum: the loop's `loss_sum += loss.double() * n`)
            acc[0:1].view(torch.float64).add_(loss.detach().to(acc.device).float().double().reshape(1) * n)
        acc[1] += 1
        acc[2] += n
        if self.kind == 'acc':
            acc[3] += (output.argmax(1) == labels).sum()
            return
        pred, truth = output.float() > self.logit_threshold, labels > 0.5
        counts = torch.stack([(pred & truth).sum(0), (pred & ~truth).sum(0), (~pred & truth).sum(0)], dim=1)
        acc[HEAD_WORDS:] += counts.reshape(-1)

    # ---- per phase: ONE device-to-host read ---------------------------------------------------------------------------
    def _words(self):
        """-> float64 numpy vector: [loss sum, launches, samples, correct, tp0, fp0, fn0, ...], summed over the ranks the
        way AccuracyMeter sums (float64 through _loop._all_sum: counts are exact below 2^53)."""
        if self._host is None:
            if self.acc is None:
                return np.zeros(HEAD_WORDS, dtype=np.float64)
            vec = torch.cat([self.acc[0:1].view(torch.float64), self.acc[1:].to(torch.float64)])
            self._host = _all_sum(vec).cpu().numpy()
        return self._host

    def loss_sum(self):
        return float(self._words()[0])

    def tallies(self):
        return int(self._words()[1])

    def samples(self):
        return int(self._words()[2])

    def compute(self, n):
        w = self._words()
        if self.kind == 'acc':
            return float(w[3]) / n
        counts = w[HEAD_WORDS:].reshape(-1, 3)
        return f1_from_counts(counts[:, 0], counts[:, 1], counts[:, 2], self.f1_type)
