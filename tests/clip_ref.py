"""float64 statement of global gradient-norm clipping inside the Adam step (include/bmnas_hip.h:
bmnas_grad_sqnorm_multi, bmnas_adam_multi_clip, bmnas_grad_scale_multi; bmnas.optim.Adam(max_grad_norm=...)), in numpy,
written from the definitions — torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam (amsgrad off, L2 weight decay
folded into the gradient) — and pinned to torch itself by tests/test_clip_ref.py."""
import numpy as np


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=np.float64)


def grad_norm(grads):
    """L2 norm over all gradients together; None entries (parameters without a gradient) are left out."""
    return float(np.sqrt(sum(float((_f64(g) ** 2).sum()) for g in grads if g is not None)))


def clip_coef(norm, max_norm):
    """max_norm / (norm + 1e-6) clamped to <= 1 by compare and select: a NaN norm gives a NaN coefficient (what
    torch.clamp(max=1) does; min(1, c) would give 1)."""
    with np.errstate(invalid='ignore', divide='ignore'):
        c = np.float64(max_norm) / (np.float64(norm) + 1e-6)
    return float(1.0 if c > 1.0 else c)


def clip(grads, max_norm):
    """-> (clipped gradients, pre-clip norm)"""
    n = grad_norm(grads)
    c = clip_coef(n, max_norm)
    return [None if g is None else _f64(g) * c for g in grads], n


def adam_step(p, g, m, v, t, lr, betas=(0.9, 0.999), eps=1e-8, wd=0.0):
    """One torch.optim.Adam update of one tensor at step count t (1-based) -> (p, m, v)."""
    p, g, m, v = _f64(p), _f64(g), _f64(m), _f64(v)
    b1, b2 = betas
    if wd != 0:
        g = g + wd * p
    m = m + (1 - b1) * (g - m)
    v = v * b2 + (1 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1 - b2 ** t) + eps
    return p - (lr / (1 - b1 ** t)) * (m / denom), m, v


def clipped_adam_step(params, grads, ms, vs, ts, lrs, max_norm, betas=(0.9, 0.999), eps=1e-8, wds=0.0):
    """Clip over ALL tensors together, then Adam tensor by tensor: the gradient is scaled BEFORE the weight-decay term
    (torch clips `.grad`, Adam then adds wd * p).  ts / lrs / wds: per tensor (or one value for all).  Tensors whose
    gradient is None are returned unchanged and their step count does not advance.
    -> (params, ms, vs, ts, pre-clip norm)"""
    n = len(params)
    per = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * n
    ts, lrs, wds = per(ts), per(lrs), per(wds)
    cg, norm = clip(grads, max_norm)
    out_p, out_m, out_v, out_t = [], [], [], []
    for i in range(n):
        if cg[i] is None:
            out_p.append(_f64(params[i])); out_m.append(_f64(ms[i])); out_v.append(_f64(vs[i])); out_t.append(ts[i])
            continue
        p, m, v = adam_step(params[i], cg[i], ms[i], vs[i], ts[i] + 1, lrs[i], betas, eps, wds[i])
        out_p.append(p); out_m.append(m); out_v.append(v); out_t.append(ts[i] + 1)
    return out_p, out_m, out_v, out_t, norm
