"""The weight-averaging recurrence of torch.optim.swa_utils.AveragedModel as the one-launch update computes it
(include/bmnas_hip.h: bmnas_avg_multi; bmnas.optim.AveragedModel), in numpy, written from the definition:

    w   = 1                        the first update (torch copies)
    w   = 1 - decay                EMA
    w   = fp32(1) / fp32(n + 1)    SWA, after n completed updates
    d   = p - a
    a   = a + w * d                |w| < 0.5
    a   = p - d * (1 - w)          otherwise                               (at::lerp's two branches)

`dtype=np.float32` evaluates it with every operation rounded to fp32 on its own — what the kernel does (no fused
multiply-add), with w and omw = 1 - w formed in double and each rounded once, as the host stages them: these are the bits
the GPU tests compare with.  `dtype=np.float64` is the statement in double, with SWA's weight the exact 1 / (n + 1):
what tests/test_avg_ref.py compares both the fp32 sequence and torch's own class with.
A RAW row copies bits.  Note the one value the first update does not copy: p = -0.0 over a positive a gives +0.0
(p - (-0.0)); every other finite p comes out bit for bit."""
import numpy as np


def weight(n, decay=None, exact=False):
    """The weight of the live tensor in the update that follows n completed ones, as a double.  SWA's is the fp32 quotient
    torch forms (get_swa_multi_avg_fn: 1 / (num_averaged + 1) on a tensor); exact: 1 / (n + 1) in double."""
    if n == 0:
        return 1.0
    if decay is None:
        return 1.0 / (n + 1) if exact else float(np.float32(1.0) / np.float32(n + 1))
    return 1.0 - float(decay)


def lerp(a, p, w, dtype=np.float32):
    """One update of one tensor with weight w (a double) -> the new average."""
    a, p = np.asarray(a, dtype=dtype), np.asarray(p, dtype=dtype)
    wq, omw = dtype(w), dtype(1.0 - w)
    d = p - a
    if abs(float(np.float32(w))) < 0.5:
        return a + wq * d
    return p - d * omw


def update(avg, live, n, decay=None, dtype=np.float32):
    """One update_parameters() over lists of arrays after n completed updates -> the new averages.  Integer arrays are
    copied (RAW rows), whatever the recipe."""
    w = weight(n, decay, exact=dtype is np.float64)
    out = []
    for a, p in zip(avg, live):
        p = np.asarray(p)
        if p.dtype.kind in 'iub':
            out.append(p.copy())
        else:
            out.append(lerp(a, p, w, dtype))
    return out


def run(snapshots, decay=None, dtype=np.float32):
    """The average after one update per snapshot (a list of lists of arrays), from n = 0."""
    avg = [np.zeros_like(np.asarray(x)) for x in snapshots[0]]
    for n, live in enumerate(snapshots):
        avg = update(avg, live, n, decay, dtype)
    return avg


def bound(n_updates, M):
    """|fp32 recurrence - float64 recurrence| after n updates of data no larger than M: an update has three roundings of
    values no larger than 2 M, plus the rounding of w, and the earlier error enters with a factor (1 - w) <= 1."""
    return 5 * n_updates * 2.0 ** -24 * M
