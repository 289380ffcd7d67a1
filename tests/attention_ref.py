"""Plain torch statement of the scaled-dot-attention block and of the 1x1 conv beside it, for
tests/test_attention_channels_gpu.py (the HIP kernels against it) and tests/test_attention_ref.py (its own
fp32-vs-fp64 conditioning).  Nothing of the product is imported here: tensors in, tensors out, gradients by
autograd; the dropout multipliers are data (`mask`).

    s   = x^T y / sqrt(C)                       (b, L, L)
    a   = softmax(s, -1)
    o   = (a y^T)^T * mask                      (b, C, L)
    out = LayerNorm_[C, L](o; ln_w, ln_b), eps 1e-5, biased variance
    loss = sum(out * g * gscale)
"""
import numpy as np
import torch

EPS = 1e-5
DROP_P, DROP_SEED, DROP_OFFSET = 0.25, 12345678901234567, 977
GSCALE = 0.37

# Table A: (C, b, L, mode, gscale given, dropout on).  mode: 'same' = y is x and dy is not passed (the y-gradient
# is added into dx), 'same+' = the same with the accumulate bit of dx set, 'acc0'..'acc3' = distinct y with that
# accumulate mask (bit 0: dx, bit 1: dy).  C covers KCH 1 full (64), 2 ragged (80), 4 ragged (208), 4 full (256),
# 5 run as 6 (272), 6 full (384), 7 run as 8 (400), 8 full (512); (b, L) = (5, 4) and (3, 8) leave the last 16-row
# tile group partly empty.  Every mode, gscale None / given and dropout off / on occurs with a ragged C (80 / 208)
# and with a C > 256.
TABLE_A = [
    (64, 5, 4, 'same', True, True), (64, 3, 8, 'acc0', False, False), (64, 2, 16, 'acc3', True, True),
    (80, 5, 4, 'acc1', True, True), (80, 3, 8, 'same', False, False), (80, 2, 16, 'acc2', False, True),
    (80, 5, 4, 'acc0', True, False), (80, 3, 8, 'acc3', True, True),
    (208, 5, 4, 'acc2', True, False), (208, 3, 8, 'acc3', False, True), (208, 2, 16, 'same', True, True),
    (208, 2, 16, 'same+', False, True),
    (256, 5, 4, 'acc0', False, True), (256, 3, 8, 'acc1', True, False), (256, 2, 16, 'same', False, True),
    (272, 5, 4, 'same', True, True), (272, 3, 8, 'acc0', True, True), (272, 2, 16, 'acc1', False, False),
    (384, 5, 4, 'acc2', False, True), (384, 3, 8, 'acc3', True, False), (384, 2, 16, 'acc0', True, True),
    (400, 5, 4, 'acc3', True, True), (400, 3, 8, 'same', False, False), (400, 2, 16, 'acc2', True, True),
    (400, 3, 8, 'same+', True, True),
    (512, 5, 4, 'acc1', True, True), (512, 3, 8, 'acc2', False, True), (512, 2, 16, 'same', True, False),
]


def gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def rand(g, *shape):
    return torch.from_numpy(g.standard_normal(shape).astype(np.float32))


def make_inputs(C, b, L, same, seed=0):
    """fp32 inputs of one case.  y carries a DC offset of 0.5: the attention output then has a non-zero
    per-sample mean, so a channel chunk missing from a LayerNorm sum shows in `mean`, not only in `rstd`."""
    g = gen(7000 + 13 * C + 5 * b + L + seed)
    y = rand(g, b, C, L) + 0.5
    x = y if same else rand(g, b, C, L)
    return {'x': x, 'y': y, 'ln_w': 1 + 0.1 * rand(g, C, L), 'ln_b': 0.1 * rand(g, C, L), 'g': rand(g, b, C, L),
            'prev_dx': rand(g, b, C, L), 'prev_dy': rand(g, b, C, L)}


def attention_ref(x, y, ln_w, ln_b, g, mask=None, gscale=None, same=False, dtype=torch.float64):
    """-> dict(out, xhat, stats (b, 2) = (mean, rstd), dx, dy, dln_w, dln_b) in `dtype`.  same: y is x, dx is
    then the one summed gradient and dy is None."""
    b, C, L = x.shape
    xr = x.detach().to(dtype).clone().requires_grad_(True)
    yr = xr if same else y.detach().to(dtype).clone().requires_grad_(True)
    w = ln_w.detach().to(dtype).clone().requires_grad_(True)
    bb = ln_b.detach().to(dtype).clone().requires_grad_(True)
    s = torch.einsum('bci,bcj->bij', xr, yr) / float(C) ** 0.5
    a = torch.softmax(s, -1)
    o = torch.einsum('bij,bcj->bci', a, yr)
    if mask is not None:
        o = o * mask.detach().to(dtype).reshape(b, C, L)
    mean = o.mean(dim=(1, 2), keepdim=True)
    var = ((o - mean) ** 2).mean(dim=(1, 2), keepdim=True)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xhat = (o - mean) * rstd
    out = xhat * w + bb
    gs = 1.0 if gscale is None else float(gscale)
    (out * g.detach().to(dtype) * gs).sum().backward()
    return {'out': out.detach(), 'xhat': xhat.detach(),
            'stats': torch.cat([mean.detach().reshape(b, 1), rstd.detach().reshape(b, 1)], 1),
            'dx': xr.grad, 'dy': None if same else yr.grad, 'dln_w': w.grad, 'dln_b': bb.grad}


def effective_weight(W, fold_cols):
    """float64 weight the conv applies: W[:, :K] + W[:, K:] when the columns are folded (conv of cat[z, z])."""
    W = W.double()
    return W if fold_cols == 0 else W[:, :fold_cols] + W[:, fold_cols:2 * fold_cols]


def conv_fwd_ref(srcs, W, bias, fold_cols):
    """float64: U = Weff cat(srcs) + bias, and the per-channel sums of d = U - bias and of d^2."""
    cat = torch.cat([s.double() for s in srcs], 1)
    d = torch.einsum('mk,bkl->bml', effective_weight(W, fold_cols), cat)
    U = d if bias is None else d + bias.double()[None, :, None]
    return {'U': U, 'd_sum': d.sum(dim=(0, 2)), 'd_sq': (d * d).sum(dim=(0, 2))}


def bn_input_grad(dV, U, bn_w):
    """float64 train-mode BatchNorm input gradient -> (dU, chan = mean | rstd | scale | 0, bn_grad = sum(dV xhat) |
    sum(dV)), the two vectors in the layout the kernels read."""
    dV, U = dV.double(), U.double()
    M, N = U.shape[1], U.shape[0] * U.shape[2]
    mean = U.mean(dim=(0, 2))
    rstd = 1.0 / torch.sqrt(U.var(dim=(0, 2), unbiased=False) + EPS)
    xhat = (U - mean[None, :, None]) * rstd[None, :, None]
    scale = rstd * bn_w.double()
    s_dx, s_d = (dV * xhat).sum(dim=(0, 2)), dV.sum(dim=(0, 2))
    dU = scale[None, :, None] * (dV - s_d[None, :, None] / N - xhat * s_dx[None, :, None] / N)
    chan = torch.cat([mean, rstd, scale, torch.zeros(M, dtype=torch.float64)])
    return dU, chan, torch.cat([s_dx, s_d])


def conv_bwd_ref(dU, W, fold_cols, srcs):
    """float64: dsrc = Weff^T dU (b, K, L), dW = dU cat(srcs)^T (M, K), dbias (M)."""
    dU = dU.double()
    cat = torch.cat([s.double() for s in srcs], 1)
    return {'dsrc': torch.einsum('mk,bml->bkl', effective_weight(W, fold_cols), dU),
            'dW': torch.einsum('bml,bkl->mk', dU, cat), 'dbias': dU.sum(dim=(0, 2))}
