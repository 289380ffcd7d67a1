"""Plain float64 statement of the step node's streaming LayerNorm (csrc/lazy_ln.hpp, csrc/lazyln.hip) and of the
head that consumes it (csrc/head.hip), for tests/test_lazy_ln_kernels_gpu.py (the HIP kernels against it) and
tests/test_lazy_ln_ref.py (this file against torch autograd).  Nothing of the product is imported here: tensors in,
tensors out, every formula written out by hand.

    node     n = (pre - mean) rstd w + b            LayerNorm_[C, L], eps 1e-5, biased variance
             backward through S1 = S(gy w), S2 = S(gy w xhat):   g = rstd (gy w - S1 / N - xhat S2 / N)
    records  per part of 1024 elements of a sample, moments centred on the part's own mean (lazy_ln.hpp)
    head     logits = relu(LayerNorm_[M C, L](cat(n_q))).view(b, -1) @ W^T + bias,  BCE-with-logits / cross-entropy
"""
import torch

EPS = 1e-5
PART = 1024             # elements per part (256 float4)
GROUP = 64              # elements per k-group of the head's backward partials
RELU_MARGIN = 1e-3      # no K7 ReLU argument of a test input may lie closer to zero than this


def _flat(t):
    return t.double().reshape(t.shape[0], -1)


def n_parts(n):
    return (n + PART - 1) // PART


def records(pre, ln_w, ln_b, centre=None):
    """rec (b, P, 8) = {m_k, S(c^2), S(c w), S(c^2 w^2), S(c w b), S(c w^2), 0, 0} with c = pre - m_k, and
    prm (P, 8) = {S(w^2), S(w), S(w b), S(b), S(b^2), n_k, 0, 0}.  centre (b, P): use these part centres instead of the
    part means (what a consumer sees when the stored m_k carries a rounding error)."""
    x, w, b = _flat(pre), ln_w.double().reshape(-1), ln_b.double().reshape(-1)
    bs, n = x.shape
    P = n_parts(n)
    rec = torch.zeros(bs, P, 8, dtype=torch.float64)
    prm = torch.zeros(P, 8, dtype=torch.float64)
    for k in range(P):
        sl = slice(k * PART, min((k + 1) * PART, n))
        xk, wk, bk = x[:, sl], w[sl], b[sl]
        m = xk.mean(dim=1) if centre is None else centre[:, k].double()
        c = xk - m[:, None]
        cw = c * wk
        rec[:, k, 0] = m
        rec[:, k, 1] = (c * c).sum(1)
        rec[:, k, 2] = cw.sum(1)
        rec[:, k, 3] = (cw * cw).sum(1)
        rec[:, k, 4] = (cw * bk).sum(1)
        rec[:, k, 5] = (cw * wk).sum(1)
        prm[k, 0] = (wk * wk).sum()
        prm[k, 1] = wk.sum()
        prm[k, 2] = (wk * bk).sum()
        prm[k, 3] = bk.sum()
        prm[k, 4] = (bk * bk).sum()
        prm[k, 5] = xk.shape[1]
    return rec, prm


def combine(rec, prm):
    """-> mean, rstd, S(o), S(o^2) per sample, o = (pre - mean) rstd w + b: the Chan combination of lazy_ln.hpp."""
    rec, prm = rec.double(), prm.double()
    nk = prm[:, 5]
    D = nk.sum()
    mu = (rec[:, :, 0] * nk).sum(1) / D
    d = rec[:, :, 0] - mu[:, None]
    M2 = (rec[:, :, 1] + nk * d * d).sum(1)
    S1 = (rec[:, :, 2] + d * prm[:, 1]).sum(1)
    S2 = (rec[:, :, 3] + 2.0 * d * rec[:, :, 5] + d * d * prm[:, 0]).sum(1)
    S3 = (rec[:, :, 4] + d * prm[:, 2]).sum(1)
    rstd = 1.0 / torch.sqrt(M2 / D + EPS)
    return mu, rstd, rstd * S1 + prm[:, 3].sum(), rstd * rstd * S2 + 2.0 * rstd * S3 + prm[:, 4].sum()


def moments(pre):
    """mean, rstd per sample, directly."""
    x = _flat(pre)
    mean = x.mean(1)
    return mean, 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + EPS)


def node_ln(pre, ln_w, ln_b):
    """-> n (shape of pre), mean (b), rstd (b), xhat (shape of pre)."""
    x = _flat(pre)
    mean, rstd = moments(pre)
    xhat = (x - mean[:, None]) * rstd[:, None]
    n = xhat * ln_w.double().reshape(-1) + ln_b.double().reshape(-1)
    return n.reshape(pre.shape), mean, rstd, xhat.reshape(pre.shape)


def out_sums(n):
    """(b, 2): per-sample sum and sum of squares of a node output."""
    f = _flat(n)
    return torch.stack([f.sum(1), (f * f).sum(1)], dim=1)


def ln_partials(gy, ln_w, xhat, group):
    """(b, ceil(N / group), 2): S(gy w), S(gy w xhat) over consecutive groups of `group` elements of a sample
    (group = PART: the K1 backward's per-part partials; GROUP: the head backward's per-64-k partials)."""
    gw = _flat(gy) * ln_w.double().reshape(-1)
    gx = gw * _flat(xhat)
    bs, n = gw.shape
    ng = (n + group - 1) // group
    out = torch.zeros(bs, ng, 2, dtype=torch.float64)
    for k in range(ng):
        sl = slice(k * group, min((k + 1) * group, n))
        out[:, k, 0] = gw[:, sl].sum(1)
        out[:, k, 1] = gx[:, sl].sum(1)
    return out


def node_ln_bwd(gy, ln_w, xhat, rstd, sums):
    """LayerNorm input gradient from the two sums, sums (b, 2) = S(gy w), S(gy w xhat) over the whole sample."""
    gw = _flat(gy) * ln_w.double().reshape(-1)
    xh = _flat(xhat)
    n = gw.shape[1]
    g = rstd.double()[:, None] * (gw - sums[:, 0:1].double() / n - xh * sums[:, 1:2].double() / n)
    return g.reshape(gy.shape)


# ------------------------------------------------------------------------------------------------------------ the head
def head_fwd(ns, ln_w, ln_b, W, bias):
    """ns: the node outputs n_q (b, C, L).  -> dict(logits, mean, rstd, xhat, arg, A, B): arg = the ReLU's argument,
    A / B (b, O) = sum_k mask w W, sum_k mask w xhat W (the two extra products of the forward GEMM)."""
    x = torch.cat([_flat(n) for n in ns], dim=1)
    w, b = ln_w.double().reshape(-1), ln_b.double().reshape(-1)
    Wd = W.double()
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + EPS)
    xhat = (x - mean[:, None]) * rstd[:, None]
    arg = xhat * w + b
    mask = (arg > 0).double()
    logits = (arg * mask) @ Wd.t() + bias.double()
    return dict(logits=logits, mean=mean, rstd=rstd, xhat=xhat, arg=arg, mask=mask, A=(mask * w) @ Wd.t(),
                B=(mask * w * xhat) @ Wd.t(), shapes=[n.shape for n in ns])


def relu_margin(fw):
    return float(fw['arg'].abs().min())


def assert_relu_clear(fw):
    m = relu_margin(fw)
    assert m >= RELU_MARGIN, f'a K7 ReLU argument lies {m:.2e} from zero (< {RELU_MARGIN})'


def bce_logits(z, y):
    """BCEWithLogits, reduction = mean -> loss, dloss/dz."""
    z, y = z.double(), y.double()
    loss = (z.clamp(min=0) - z * y + torch.log1p(torch.exp(-z.abs()))).mean()
    return loss, (torch.sigmoid(z) - y) / z.numel()


def cross_entropy(z, label):
    """CrossEntropy, reduction = mean -> loss, dloss/dz."""
    z = z.double()
    mx = z.max(dim=1, keepdim=True).values
    e = torch.exp(z - mx)
    den = e.sum(1, keepdim=True)
    onehot = torch.zeros_like(z)
    onehot[torch.arange(z.shape[0]), label] = 1.0
    loss = ((mx + torch.log(den)) - (z * onehot).sum(1, keepdim=True)).mean()
    return loss, (e / den - onehot) / z.shape[0]


def head_bwd(fw, ln_w, W, dlogits):
    """-> dict(dn = [gradient of n_q], dW, dbias, dln_w, dln_b)."""
    w, Wd, dl = ln_w.double().reshape(-1), W.double(), dlogits.double()
    gy = (dl @ Wd) * fw['mask']                                 # gradient at the LayerNorm output
    gw = gy * w
    D = gw.shape[1]
    m1, m2 = gw.sum(1, keepdim=True) / D, (gw * fw['xhat']).sum(1, keepdim=True) / D
    dx = fw['rstd'][:, None] * (gw - m1 - fw['xhat'] * m2)
    dn, at = [], 0
    for shp in fw['shapes']:
        n = shp[1] * shp[2]
        dn.append(dx[:, at:at + n].reshape(shp))
        at += n
    return dict(dn=dn, dW=dl.t() @ (fw['arg'] * fw['mask']), dbias=dl.sum(0), dln_w=(gy * fw['xhat']).sum(0),
                dln_b=gy.sum(0))


# ------------------------------------------------------------------------------------------------------------ inputs
def offset_resid(gen, b, C, L):
    """The offset case: centred at +30 with std 0.5, part 0 shifted by +20 and part 1 by -20 — part means far from
    the sample mean, which is what the Chan combination exists for."""
    r = torch.randn(b, C * L, generator=gen) * 0.5 + 30.0
    r[:, :PART] += 20.0
    if C * L > PART:
        r[:, PART:2 * PART] -= 20.0
    return r.reshape(b, C, L)


def clear_relu_bias(gen, ns, ln_w, ln_b, tries=64):
    """Redraw the K7 bias entries whose ReLU argument lies within RELU_MARGIN of zero for some sample until none
    remains.  -> the bias to use (same shape and dtype as ln_b)."""
    x = torch.cat([_flat(n) for n in ns], dim=1)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + EPS)
    xw = (x - mean[:, None]) * rstd[:, None] * ln_w.double().reshape(-1)
    out = ln_b.clone().reshape(-1)
    for _ in range(tries):
        bad = ((xw + out.double()).abs() < 2.0 * RELU_MARGIN).any(dim=0)
        if not bool(bad.any()):
            return out.reshape(ln_b.shape)
        out[bad] = (torch.randn(int(bad.sum()), generator=gen) * 0.2).to(out.dtype)
    raise AssertionError('could not clear the K7 ReLU arguments')
