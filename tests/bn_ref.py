"""float64 statement of the BatchNorm family of csrc/bnmix.hip and csrc/bn_fin.hpp, for tests/test_bn_kernels_gpu.py
(the HIP kernels against it) and tests/test_bn_ref.py (this file against torch in float64 on the CPU).  Nothing of the
product is imported: tensors in, tensors out.  The train-mode input gradient, the eval-mode `chan`, the per-n-group
partials and the sharded sums are the ones tests/attention_ref.py and tests/conv_ref.py already state.

    chan = mean | rstd | scale | shift           (4 M)      scale = bn_w rstd, shift = bn_b - mean scale
    bn_grad = sum dV u_hat | sum dV              (2 M)      u_hat = (U - mean) rstd, sums over (sample, l)

An activation is (b, M, L); N = b L columns per channel; the GLU's M = 2 C channels are [a | gate].
"""
import torch

from attention_ref import EPS, bn_input_grad  # noqa: F401
from conv_ref import bn_eval_chan, chan_combine, group_partials, shard_sums  # noqa: F401

MOMENTUM = 0.1


def _chan(mean, var, bn_w, bn_b):
    rstd = 1.0 / torch.sqrt(var + EPS)
    scale = bn_w.double() * rstd
    return torch.cat([mean, rstd, scale, bn_b.double() - mean * scale])


def _finish(mean, var, N, bn_w, bn_b, rm, rv, nbt, training):
    """dict(chan, rm, rv, nbt) after one step.  rm / rv / nbt None: absent, None comes back.  Eval: chan from the
    running statistics, nothing else changes."""
    if not training:
        return {'chan': bn_eval_chan(bn_w, bn_b, rm, rv), 'rm': rm.double(), 'rv': rv.double(),
                'nbt': None if nbt is None else nbt.clone()}
    out = {'chan': _chan(mean, var, bn_w, bn_b), 'rm': None, 'rv': None, 'nbt': None if nbt is None else nbt + 1}
    if rm is not None:
        out['rm'] = (1.0 - MOMENTUM) * rm.double() + MOMENTUM * mean
        out['rv'] = (1.0 - MOMENTUM) * rv.double() + MOMENTUM * var * N / (N - 1)
    return out


def sums_of(U, conv_bias, shards):
    """stat (shards, M, 2): the sums of d = U - bias and of d^2 (conv_ref.shard_sums, one n-group per block)."""
    d = U.double() if conv_bias is None else U.double() - conv_bias.double()[None, :, None]
    return shard_sums(d, shards)


def fin_from_sums(stat, conv_bias, bn_w, bn_b, rm, rv, nbt, N, training=True):
    """bn_fin_fill: stat (shards, M, 2) holds the sums of d = u - bias and of d^2 over the N columns.
    var = max(E[d^2] - E[d]^2, 0), mean = E[d] + bias."""
    if not training:
        return _finish(None, None, N, bn_w, bn_b, rm, rv, nbt, False)
    s = stat.double().sum(0)
    dm = s[:, 0] / N
    var = torch.clamp(s[:, 1] / N - dm * dm, min=0.0)
    mean = dm if conv_bias is None else dm + conv_bias.double()
    return _finish(mean, var, N, bn_w, bn_b, rm, rv, nbt, True)


def partial_counts(N, n_part):
    return [min(16, N - 16 * p) for p in range(n_part)]


def fin_from_partials(part, bn_w, bn_b, rm, rv, nbt, N, training=True):
    """bmnas_bn_finalize: Chan's rule over part (M, n_part, 2) = (sum, second moment about the partial's own mean) of
    the partials of min(16, N - 16 p) columns."""
    if not training:
        return _finish(None, None, N, bn_w, bn_b, rm, rv, nbt, False)
    mean, var = chan_combine(part.double(), partial_counts(N, part.shape[1]))
    return _finish(mean, var, N, bn_w, bn_b, rm, rv, nbt, True)


def affine(U, scale, shift):
    return U.double() * scale.double()[None, :, None] + shift.double()[None, :, None]


def softplus(v):
    return torch.clamp(v, min=0.0) + torch.log1p(torch.exp(-v.abs()))


def mish(v):
    return v * torch.tanh(softplus(v))


def dmish(v):
    t = torch.tanh(softplus(v))
    return t + v * torch.sigmoid(v) * (1.0 - t * t)


def tail_fwd(kind, U, scale, shift, mask=None):
    """kind 'relu' | 'mish': act(v) m, (b, M, L); 'glu': va sigmoid(vg) m over the two halves of M = 2 C, (b, C, L).
    mask: the dropout multipliers of the output's elements (flat or shaped), None = 1."""
    v = affine(U, scale, shift)
    if kind == 'glu':
        C = U.shape[1] // 2
        o = v[:, :C] * torch.sigmoid(v[:, C:])
    else:
        o = torch.relu(v) if kind == 'relu' else mish(v)
    return o if mask is None else o * mask.double().reshape(o.shape)


def tail_bwd(kind, g, U, chan, mask=None, prev_bn_grad=None):
    """-> (dV (b, M, L): the gradient at the BatchNorm output, bn_grad (2 M) added to prev_bn_grad).  g: the gradient of
    the tail's output.  The ReLU gradient at v == 0 is 0."""
    M = U.shape[1]
    c = chan.double()
    mean, rstd, scale, shift = c[:M], c[M:2 * M], c[2 * M:3 * M], c[3 * M:]
    v = affine(U, scale, shift)
    gm = g.double() if mask is None else g.double() * mask.double().reshape(g.shape)
    if kind == 'glu':
        C = M // 2
        va, sg = v[:, :C], torch.sigmoid(v[:, C:])
        dV = torch.cat([gm * sg, gm * va * sg * (1.0 - sg)], 1)
    elif kind == 'relu':
        dV = torch.where(v > 0, gm, torch.zeros_like(gm))
    else:
        dV = gm * dmish(v)
    uhat = (U.double() - mean[None, :, None]) * rstd[None, :, None]
    bn_grad = torch.cat([(dV * uhat).sum(dim=(0, 2)), dV.sum(dim=(0, 2))])
    return dV, bn_grad if prev_bn_grad is None else bn_grad + prev_bn_grad.double()


def phase_b(dV, U, chan, bn_grad, training):
    """bmnas_bn_bwd_apply: dU = scale (dV - db / N - u_hat dw / N) in training, scale dV in eval (U and bn_grad are
    then not read)."""
    M = dV.shape[1]
    c = chan.double()
    scale = c[2 * M:3 * M][None, :, None]
    if not training:
        return dV.double() * scale
    N = dV.shape[0] * dV.shape[2]
    uhat = (U.double() - c[:M][None, :, None]) * c[M:2 * M][None, :, None]
    bg = bn_grad.double()
    return scale * (dV.double() - bg[M:][None, :, None] / N - uhat * bg[:M][None, :, None] / N)
