"""float64 statement of the Adam variants of the one-launch step (include/bmnas_hip.h: bmnas_adam_multi_ex;
bmnas.optim.Adam(amsgrad=..., decoupled_weight_decay=...), bmnas.optim.AdamW), in numpy, written from the definitions —
torch 2.10's _single_tensor_adam — and pinned to torch itself by tests/test_adam_ref.py.  Clipping comes from
tests/clip_ref.py: the coefficient multiplies the gradient first; a decoupled decay never touches the gradient."""
import numpy as np

import clip_ref
from clip_ref import _f64


def maximum(a, b):
    """torch.maximum: a NaN in either operand gives NaN (np.fmax / C's fmax would drop it)."""
    return np.maximum(_f64(a), _f64(b))


def adam_step(p, g, m, v, vmax, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0, amsgrad=False, decoupled=False):
    """One update of one tensor at step count t (1-based) -> (p, m, v, vmax); vmax is passed through (None allowed)
    without amsgrad."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    b1, b2 = betas
    if wd != 0:
        if decoupled:
            p = p * (1 - lr * wd)
        else:
            g = g + wd * p
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    if amsgrad:
        vmax = maximum(vmax, v)
        denom = np.sqrt(vmax) / np.sqrt(1 - b2 ** t) + eps
    else:
        denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * (m / denom), m, v, vmax


class Ref:
    """The optimizer over a list of tensors: per-tensor step counts (a tensor without a gradient does not advance),
    per-tensor learning rate / weight decay, optional global clipping in front of every step."""

    def __init__(self, params, betas=(0.9, 0.999), eps=1e-8, amsgrad=False, decoupled=False, max_norm=None):
        self.P = [_f64(p).copy() for p in params]
        self.M = [np.zeros_like(p) for p in self.P]
        self.V = [np.zeros_like(p) for p in self.P]
        self.X = [np.zeros_like(p) for p in self.P]          # max_exp_avg_sq
        self.T = [0] * len(self.P)
        self.betas, self.eps, self.amsgrad, self.decoupled, self.max_norm = betas, eps, amsgrad, decoupled, max_norm
        self.norm = None

    def step(self, grads, lrs, wds=0.0):
        n = len(self.P)
        per = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * n
        lrs, wds = per(lrs), per(wds)
        grads = [None if g is None else _f64(g) for g in grads]
        if self.max_norm is not None:
            grads, self.norm = clip_ref.clip(grads, self.max_norm)
        for i, g in enumerate(grads):
            if g is None:
                continue
            self.T[i] += 1
            self.P[i], self.M[i], self.V[i], self.X[i] = adam_step(
                self.P[i], g, self.M[i], self.V[i], self.X[i], self.T[i], lrs[i], self.betas, self.eps, wds[i],
                self.amsgrad, self.decoupled)
