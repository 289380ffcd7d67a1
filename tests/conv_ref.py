"""float64 statement of what the four stand-alone 1x1-conv entry points compute (include/bmnas_hip.h:
bmnas_conv1x1_fwd, _bwd_data, _bwd_weight, _bwd_all), for tests/test_conv_kernels_gpu.py (the HIP kernels against it)
and tests/test_conv_ref.py (this file against torch autograd on the CPU).  Nothing of the product is imported:
tensors in, tensors out.  The contraction itself, the weight fold and the train-mode BatchNorm input gradient are the
ones tests/attention_ref.py already states; here is what the stand-alone entry points add to them.

Columns: an activation (b, C, L) is C rows of b * L columns n = s * L + l; an n-group is 16 consecutive columns
(16 / L samples), the last one holds the b * L - 16 g columns that are left.
"""
import torch

from attention_ref import EPS, bn_input_grad, conv_bwd_ref, conv_fwd_ref, effective_weight  # noqa: F401


def n_groups(b, L):
    return (b * L + 15) // 16


def weight_used(W, K, fold_cols):
    """(M, K) float64 weight a call applies: the first K columns of the (M, ldw) rows, plus the K columns that start
    at fold_cols when the columns are folded (the tests fold with fold_cols = K: the conv of cat[z, z])."""
    if fold_cols == 0:
        return effective_weight(W[:, :K], 0)
    assert fold_cols == K, (fold_cols, K)
    return effective_weight(W[:, :2 * K], K)


def columns(U):
    """(b, M, L) -> (M, b * L): channel rows over the (sample, l) columns."""
    return U.double().permute(1, 0, 2).reshape(U.shape[1], -1)


def group_partials(U):
    """part (M, ng, 2) = (sum, second moment about the group's OWN mean) of every channel over the valid columns of
    every n-group (bn_tile_stats: cnt = min(16, b L - 16 g); bmnas_bn_finalize combines them with Chan's rule)."""
    c = columns(U)
    M, N = c.shape
    ng = (N + 15) // 16
    part = torch.zeros(M, ng, 2, dtype=torch.float64)
    for g in range(ng):
        blk = c[:, 16 * g:min(16 * g + 16, N)]
        s = blk.sum(1)
        mean = s / blk.shape[1]
        part[:, g, 0] = s
        part[:, g, 1] = ((blk - mean[:, None]) ** 2).sum(1)
    return part


def chan_combine(part, counts):
    """Chan's parallel rule over the partials -> (mean, biased variance) per channel: what they must add up to."""
    n = torch.zeros((), dtype=torch.float64)
    mean = torch.zeros(part.shape[0], dtype=torch.float64)
    m2 = torch.zeros(part.shape[0], dtype=torch.float64)
    for g, cnt in enumerate(counts):
        mg = part[:, g, 0] / cnt
        delta = mg - mean
        tot = n + cnt
        mean = mean + delta * cnt / tot
        m2 = m2 + part[:, g, 1] + delta * delta * n * cnt / tot
        n = tot
    return mean, m2 / n


def shard_sums(d, stat_shards, groups_per_block=1):
    """stat (stat_shards, M, 2): the sums of d = U - bias and of d^2 over the valid columns, column block
    g // groups_per_block going to shard (g // groups_per_block) % stat_shards.  A column block is one n-group for the
    split-K and whole-K LDS kernels and the 2 or 4 n-groups of a tile for the pipelined ones."""
    c = columns(d)
    M, N = c.shape
    stat = torch.zeros(stat_shards, M, 2, dtype=torch.float64)
    for g in range((N + 15) // 16):
        blk = c[:, 16 * g:min(16 * g + 16, N)]
        sh = (g // groups_per_block) % stat_shards
        stat[sh, :, 0] += blk.sum(1)
        stat[sh, :, 1] += (blk * blk).sum(1)
    return stat


def conv_fwd(srcs, W, bias, fold_cols=0, stat_shards=0, groups_per_block=1):
    """-> dict(U, part (M, ng, 2), stat (stat_shards, M, 2) or None)."""
    K = sum(s.shape[1] for s in srcs)
    r = conv_fwd_ref(srcs, weight_used(W, K, fold_cols), bias, 0)
    d = r['U'] if bias is None else r['U'] - bias.double()[None, :, None]
    return {'U': r['U'], 'part': group_partials(r['U']),
            'stat': shard_sums(d, stat_shards, groups_per_block) if stat_shards > 0 else None}


def bn_eval_input_grad(dV, scale):
    """eval-mode BatchNorm input gradient: dU = scale * dV, scale = bn_w / sqrt(running_var + eps) (chan[2M:3M])."""
    return dV.double() * scale.double()[None, :, None]


def bn_eval_chan(bn_w, bn_b, running_mean, running_var):
    """chan = mean | rstd | scale | shift of an eval-mode BatchNorm, in the layout the kernels read."""
    rstd = 1.0 / torch.sqrt(running_var.double() + EPS)
    scale = rstd * bn_w.double()
    return torch.cat([running_mean.double(), rstd, scale, bn_b.double() - running_mean.double() * scale])


def conv_bwd_data(dU, W, fold_cols, C_src, prevs, accumulate_mask):
    """dsrcs: prevs[q] is None for a NULL destination (skipped: None comes back), otherwise the tensor the
    destination held before the call; bit q of accumulate_mask adds to it, a clear bit overwrites it."""
    K = C_src * len(prevs)
    d = torch.einsum('mk,bml->bkl', weight_used(W, K, fold_cols), dU.double())
    out = []
    for q, prev in enumerate(prevs):
        if prev is None:
            out.append(None)
            continue
        v = d[:, q * C_src:(q + 1) * C_src]
        out.append(v + prev.double() if (accumulate_mask >> q) & 1 else v)
    return out


def conv_bwd_weight(dU, srcs, prev_dW, prev_dbias, dup_cols=0):
    """dW (M, ldw) and dbias (M) after the call: both ACCUMULATE into what was there; with dup_cols > 0 the same
    value is also added at column k + dup_cols; columns the call does not name keep their value; dbias None = NULL."""
    r = conv_bwd_ref(dU, torch.zeros(dU.shape[1], 0), 0, srcs)
    K = r['dW'].shape[1]
    dW = prev_dW.double().clone()
    dW[:, :K] += r['dW']
    if dup_cols > 0:
        dW[:, dup_cols:dup_cols + K] += r['dW']
    return dW, None if prev_dbias is None else prev_dbias.double() + r['dbias']
