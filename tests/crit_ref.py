"""float64 restatement of the two criteria with their options (weight, pos_weight, label smoothing,
ignore_index, reduction mean | sum): loss and dloss/dlogits written out as formulas, on the CPU.
tests/test_crit_ref.py pins it against torch.nn.functional with autograd; the GPU tests of the
weighted criterion kernels (csrc/linear.hip, csrc/head.hip) compare against it.

    BCE   c = 1 + (p - 1) y
          l  = w [(1 - y) z + c (log1p(exp(-|z|)) + max(-z, 0))]
          dz = w [(1 - y) - c (1 - sigmoid(z))]                 mean: / numel
    CE    keep_i = y_i != ignore_index, p = softmax(z_i), W = sum_c w_c
          loss  = ((1 - e) sum_i keep_i w[y_i] (-log p[y_i]) + (e / O) sum_i keep_i sum_c w_c (-log p_c)) / den
          dz_ic = keep_i [(1 - e) w[y_i] (p_c - [c == y_i]) + (e / O) (W p_c - w_c)] / den
          den   = sum_i keep_i w[y_i] (mean) | 1 (sum);  no row counts under mean: loss NaN, dz 0
"""
import torch

F64 = torch.float64


def _vec(v, n):
    return torch.ones(n, dtype=F64) if v is None else v.detach().cpu().to(F64)


def bce(z, y, weight=None, pos_weight=None, reduction='mean'):
    """-> (loss 0-dim, dz like z), float64."""
    z, y = z.detach().cpu().to(F64), y.detach().cpu().to(F64)
    O = z.shape[-1]
    w, p = _vec(weight, O), _vec(pos_weight, O)
    c = 1 + (p - 1) * y
    soft = torch.log1p(torch.exp(-z.abs())) + torch.clamp(-z, min=0)
    loss = (w * ((1 - y) * z + c * soft)).sum()
    dz = w * ((1 - y) - c * (1 - torch.sigmoid(z)))
    if reduction == 'mean':
        return loss / z.numel(), dz / z.numel()
    assert reduction == 'sum'
    return loss, dz


def ce(z, y, weight=None, label_smoothing=0.0, ignore_index=-100, reduction='mean'):
    """-> (loss 0-dim, dz (b, O)), float64.  y: int64 class ids (b)."""
    z, y = z.detach().cpu().to(F64), y.detach().cpu()
    b, O = z.shape
    w = _vec(weight, O)
    keep = y != ignore_index
    yc = torch.where(keep, y, torch.zeros_like(y))               # (never an index where the row is ignored)
    zs = z - z.max(1, keepdim=True).values
    logp = zs - torch.log(torch.exp(zs).sum(1, keepdim=True))
    p = torch.exp(logp)
    k = keep.to(F64)
    wy = w[yc] * k
    onehot = torch.zeros_like(z)
    onehot[torch.arange(b), yc] = 1.0
    nll = -(wy * logp[torch.arange(b), yc]).sum()
    smooth = -(k[:, None] * w[None, :] * logp).sum()
    e = label_smoothing
    den = wy.sum() if reduction == 'mean' else torch.ones((), dtype=F64)
    assert reduction in ('mean', 'sum')
    loss = ((1 - e) * nll + (e / O) * smooth) / den              # (0 / 0 = NaN when no row counts, as torch)
    num = k[:, None] * ((1 - e) * wy[:, None] * (p - onehot) + (e / O) * (w.sum() * p - w[None, :]))
    dz = torch.where(keep[:, None], num / den, torch.zeros_like(num))
    return loss, dz
