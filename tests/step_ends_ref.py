"""Plain float64 statement of the jobs packed into the launches that open and close a search step — the cell prologue
(csrc/bnmix.hip: cell_prologue_body, cell_prologue_pair_k) and the backward epilogue (csrc/layernorm.hip:
backward_epilogue_k, ln_affine_body; csrc/arch_body.hpp) — and of the stand-alone entry points made of the same pieces,
for tests/test_step_ends_kernels_gpu.py (the HIP kernels against it) and tests/test_step_ends_ref.py (this file against
torch autograd).  Nothing of the product is imported here: tensors in, tensors out, every formula written out by hand.
All inputs are the fp32 values the kernel sees, cast to double.

    row softmax   w = exp(l - max l) / sum_p exp(l_p - max l)                       per row of an architecture tensor
    its backward  D = sum over gradient shards,  dl = w (D - sum_p w_p D_p)
    fold          Weff = W[:, :C] + W[:, C:]                                        W (M, 2 C)
    pair sum      h = sum_j softmax(alpha_j)[1] x_j,  z = (softmax(beta_0)[1] + softmax(beta_1)[1]) h
    LN affine     gy = g gscale [xhat w + b > 0],  dln_w = sum_s gy xhat,  dln_b = sum_s gy
    chunk sum     out[e] = sum_c part[c, e]
"""
import torch

from lazy_ln_ref import RELU_MARGIN, clear_relu_bias  # noqa: F401  (the K7-like inputs of the GPU tests use them)


def _d(t):
    return t.detach().double().cpu()


def row_softmax(logits):
    """(rows, cols) logits -> (rows, cols) weights"""
    a = _d(logits)
    e = torch.exp(a - a.max(dim=1, keepdim=True).values)
    return e / e.sum(dim=1, keepdim=True)


def row_softmax_bwd(w, dw_shards):
    """w (rows, cols): the softmaxed weights; dw_shards (n_shards, rows, cols): their gradient, in shards that the
    backward sums.  -> dlogits (rows, cols)"""
    w = _d(w)
    D = _d(dw_shards).sum(dim=0)
    return w * (D - (w * D).sum(dim=1, keepdim=True))


def fold(W):
    """W (M, 2 C) -> (M, C)"""
    W = _d(W)
    C = W.shape[1] // 2
    assert W.shape[1] == 2 * C
    return W[:, :C] + W[:, C:]


def pair_sum(xs, alpha_logits, beta_logits):
    """xs: n_in tensors of one shape; alpha_logits (n_in, 2): the logits row of each input's edge; beta_logits (2, 2).
    -> h, z"""
    wa, wb = row_softmax(alpha_logits)[:, 1], row_softmax(beta_logits)[:, 1]
    assert wa.numel() == len(xs) and wb.numel() == 2
    h = sum(wa[j] * _d(x) for j, x in enumerate(xs))
    return h, (wb[0] + wb[1]) * h


def ln_affine(g, gscale, srcs, resid, ln_w, ln_b, stats, relu, prenorm):
    """g (b, ...): gradient at the LayerNorm's output (after the ReLU when relu); gscale: None or a scalar tensor;
    srcs: the tensors (b, C, L) whose concatenation along C (+ resid) the LayerNorm normalised — with prenorm srcs[0] IS
    xhat; stats (b, 2) = the fp32 mean | rstd the kernel is handed (None with prenorm); ln_w / ln_b: read only for
    the ReLU's argument.  -> dln_w, dln_b, flat (sum_q C_q L)."""
    b = g.shape[0]
    gy = _d(g).reshape(b, -1)
    if gscale is not None:
        gy = gy * float(_d(gscale).reshape(-1)[0])
    if prenorm:
        xhat = _d(srcs[0]).reshape(b, -1)
    else:
        x = torch.cat([_d(s).reshape(b, -1) for s in srcs], dim=1)
        if resid is not None:
            x = x + _d(resid).reshape(b, -1)
        st = _d(stats)
        xhat = (x - st[:, 0:1]) * st[:, 1:2]
    if relu:
        gy = gy * (xhat * _d(ln_w).reshape(-1) + _d(ln_b).reshape(-1) > 0).double()
    return (gy * xhat).sum(dim=0), gy.sum(dim=0)


def chunk_sum(part, n_chunk):
    """part: n_chunk consecutive copies of n floats -> (n)"""
    p = _d(part).reshape(n_chunk, -1)
    return p.sum(dim=0)
