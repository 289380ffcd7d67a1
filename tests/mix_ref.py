"""float64 statement of the NodeMixedOp mix (csrc/mix_terms.hpp) as its kernel families compute it — csrc/bnmix.hip,
csrc/nodemix_sel.hip, csrc/mixconv.hip and the mix epilogue of csrc/conv1x1.hip — for tests/test_mix_kernels_gpu.py (the
HIP kernels against it) and tests/test_mix_ref.py (this file against torch autograd in float64 on the CPU).  Nothing of
the product is imported: tensors in, tensors out.

    s = g0 (x + y) + g1 p1 + g2 drop(va sigmoid(vg)) + g3 drop(act(vf)),      va | vg | vf = BatchNorm(U rows)

mask: bit 0 Sum, 1 ScaleDotAttn, 2 LinearGLU, 3 ConcatFC (act 'relu') / CatConvMish (act 'mish').  U (b, M, L) holds only
the present conv rows, M = 2 C [LinearGLU: a | gate] + C [FC], LinearGLU's first.  cols[k] is the gamma column of kind
k (any value where the kind is absent); gamma has one entry per present kind.  m_glu / m_fc: the dropout multipliers
(0 or 1 / (1 - p)) of the two sites, flat or shaped (b, C, L), None = 1.  chan = mean | rstd | scale | shift (4 M).
"""
import torch

from bn_ref import affine, dmish, mish
from conv_ref import conv_fwd_ref, shard_sums
from lazy_ln_ref import node_ln, node_ln_bwd, out_sums

SUM, ATTN, GLU, FC = 1, 2, 4, 8
ALL = 15
IDENT = (0, 1, 2, 3)
RELU_MARGIN = 1e-3      # no ReLU argument of a GPU case may lie closer to zero than this


def conv_rows(mask, C):
    """-> (M, first FC row): the rows of U under a mask"""
    fo = 2 * C if mask & GLU else 0
    return fo + (C if mask & FC else 0), fo


def _m(mask_t, like):
    return torch.ones_like(like) if mask_t is None else mask_t.double().reshape(like.shape)


def _bn_out(mask, U, scale, shift, C):
    """va, vg, vf (b, C, L) of the present rows, None where absent"""
    M, fo = conv_rows(mask, C)
    if M == 0:
        return None, None, None
    assert U.shape[1] == M and scale.numel() == M and shift.numel() == M
    v = affine(U, scale, shift)
    va, vg = (v[:, :C], v[:, C:2 * C]) if mask & GLU else (None, None)
    return va, vg, (v[:, fo:fo + C] if mask & FC else None)


def _act(act, v):
    assert act in ('relu', 'mish')
    return torch.relu(v) if act == 'relu' else mish(v)


def mix_terms(mask, act, x, y, p1, U, scale, shift, m_glu, m_fc):
    """-> the four terms [x + y, p1, drop(glu), drop(act(fc))], None where absent"""
    ref = next(t for t in (x, p1, U) if t is not None)
    b, L = ref.shape[0], ref.shape[2]
    C = (x if mask & SUM else p1).shape[1] if mask & (SUM | ATTN) else U.shape[1] // conv_rows(mask, 1)[0]
    va, vg, vf = _bn_out(mask, U, scale, shift, C)
    t = [None] * 4
    if mask & SUM:
        t[0] = x.double() + y.double()
    if mask & ATTN:
        t[1] = p1.double()
    if mask & GLU:
        t[2] = va * torch.sigmoid(vg)
        t[2] = t[2] * _m(m_glu, t[2])
    if mask & FC:
        t[3] = _act(act, vf)
        t[3] = t[3] * _m(m_fc, t[3])
    assert all(q is None or q.shape == (b, C, L) for q in t)
    return t


def mix_fwd(mask, act, cols, gamma, x, y, p1, U, scale, shift, m_glu=None, m_fc=None):
    """s (b, C, L)"""
    assert 1 <= mask <= 15
    g = gamma.double()
    t = mix_terms(mask, act, x, y, p1, U, scale, shift, m_glu, m_fc)
    return sum(g[cols[k]] * t[k] for k in range(4) if mask >> k & 1)


def mix_bwd(mask, act, cols, gamma, g, x, y, p1, U, chan, m_glu=None, m_fc=None, *, dx_old=None, dy_old=None,
            acc_mask=0, prev_bn_grad=None):
    """g: the gradient of s.  -> dict
      dgamma   (len(gamma)): <g, term_k> at column cols[k], 0 elsewhere (to be ADDED to what a shard held)
      dgamma_abs  the same sums over |g term_k|: the scale a cancelling scalar reduction is judged by
      dV       (b, M, L) the gradient at the BatchNorm output (None at M = 0); the ReLU gradient at vf == 0 is 0
      bn_grad  (2 M) = sum dV u_hat | sum dV, added to prev_bn_grad
      dx, dy   what the destinations hold afterwards, given what they held before (dx_old / dy_old: None = a NULL
               destination, None comes back).  With Sum: g0 g (+ old under the accumulate bit: 1 dx, 2 dy); dy NULL sends
               both halves, 2 g0 g, to dx.  Without Sum (node_mix_sel_bwd_k): a destination whose bit is clear is
               zero-filled, one whose bit is set is untouched — `dx_rule` / `dy_rule` say 'write' | 'zero' | 'keep'."""
    assert 1 <= mask <= 15
    gm, gd = gamma.double(), g.double()
    C = gd.shape[1]
    M, fo = conv_rows(mask, C)
    scale = shift = None
    if M:
        c = chan.double()
        mean, rstd, scale, shift = c[:M], c[M:2 * M], c[2 * M:3 * M], c[3 * M:]
    t = mix_terms(mask, act, x, y, p1, U, scale, shift, m_glu, m_fc)
    dgamma, dgabs = torch.zeros_like(gm), torch.zeros_like(gm)
    for k in range(4):
        if mask >> k & 1:
            dgamma[cols[k]] = (gd * t[k]).sum()
            dgabs[cols[k]] = (gd * t[k]).abs().sum()
    out = dict(dgamma=dgamma, dgamma_abs=dgabs, dV=None, bn_grad=None)
    if M:
        va, vg, vf = _bn_out(mask, U, scale, shift, C)
        parts = []
        if mask & GLU:
            sg = torch.sigmoid(vg)
            gm2 = gm[cols[2]] * gd * _m(m_glu, gd)
            parts += [gm2 * sg, gm2 * va * sg * (1.0 - sg)]
        if mask & FC:
            gm3 = gm[cols[3]] * gd * _m(m_fc, gd)
            parts.append(torch.where(vf > 0, gm3, torch.zeros_like(gm3)) if act == 'relu' else gm3 * dmish(vf))
        dV = torch.cat(parts, 1)
        uhat = (U.double() - mean[None, :, None]) * rstd[None, :, None]
        bg = torch.cat([(dV * uhat).sum(dim=(0, 2)), dV.sum(dim=(0, 2))])
        out.update(dV=dV, bn_grad=bg if prev_bn_grad is None else bg + prev_bn_grad.double())
    for name, old, bit in (('dx', dx_old, 1), ('dy', dy_old, 2)):
        if old is None:
            out[name], out[name + '_rule'] = None, None
        elif mask & SUM:
            d = gm[cols[0]] * gd * (2.0 if name == 'dx' and dy_old is None else 1.0)
            out[name], out[name + '_rule'] = (d + old.double() if acc_mask & bit else d), 'write'
        elif acc_mask & bit:
            out[name], out[name + '_rule'] = old.double(), 'keep'
        else:
            out[name], out[name + '_rule'] = torch.zeros_like(gd), 'zero'
    return out


# ------------------------------------------------------------------------------------------------ the next-step rider
def next_fwd(prevs, w, s):
    """z_next = sum_j w_j prev_j + w_n s;  w: the n + 1 weights (already picked at their stride)"""
    w = w.double()
    assert w.numel() == len(prevs) + 1
    return sum((w[j] * p.double() for j, p in enumerate(prevs)), w[len(prevs)] * s.double())


def next_bwd(prevs, w, s, gz, gz2, g_in, dprev_old, dest, acc_mask):
    """The backward of z_next inside the mix backward.  G = gz + gz2 (gz2 None: absent); g_out = g_in + w_n G (g_in
    None: absent); dw[j] = <G, prev_j> (j < n), dw[n] = <G, s> (to be ADDED to a shard), dw_abs the sums of |.|.
    dprev: dest[j] names destination j's buffer (None: NULL; equal names alias), dprev_old[name] is what the buffer
    held; in order j = 0 .. n - 1: buffer (=|+= by bit j of acc_mask) w_j G, as read-modify-write.
    -> dict(G, g_out, dw, dw_abs, dprev {name: final contents})"""
    w = w.double()
    n = len(prevs)
    assert w.numel() == n + 1 and len(dest) == n
    G = gz.double() if gz2 is None else gz.double() + gz2.double()
    g_out = w[n] * G if g_in is None else g_in.double() + w[n] * G
    terms = [G * p.double() for p in prevs] + [G * s.double()]
    buf = {k: v.double().clone() for k, v in dprev_old.items()}
    for j in range(n):
        if dest[j] is None:
            continue
        buf[dest[j]] = w[j] * G + (buf[dest[j]] if acc_mask >> j & 1 else 0.0)
    return dict(G=G, g_out=g_out, dw=torch.stack([t.sum() for t in terms]),
                dw_abs=torch.stack([t.abs().sum() for t in terms]), dprev=buf)


# ------------------------------------------------------------------------------------- the LayerNorm tail around the mix
def mix_ln_fwd(s, resid, ln_w, ln_b):
    """pre = s + resid, out = LayerNorm_[C, L](pre), stats (b, 2) = mean | rstd, out_sums (b, 2) = S(out) | S(out^2)"""
    pre = s.double() + resid.double()
    out, mean, rstd, _ = node_ln(pre, ln_w, ln_b)
    return dict(pre=pre, out=out, stats=torch.stack([mean, rstd], 1), out_sums=out_sums(out))


def mix_ln_bwd(gy, pre, ln_w, stats, dresid_old=None, accumulate_resid=False):
    """gy: the gradient of out; pre and stats (b, 2) as the forward SAVED them (the kernel recomputes neither).
    -> g_in (the LayerNorm input gradient = the mix's g), dresid (None for a NULL destination; = | += g_in)"""
    st = stats.double()
    xhat = (pre.double() - st[:, 0][:, None, None]) * st[:, 1][:, None, None]
    gw = gy.double().reshape(gy.shape[0], -1) * ln_w.double().reshape(-1)
    sums = torch.stack([gw.sum(1), (gw * xhat.reshape(gw.shape)).sum(1)], 1)
    g_in = node_ln_bwd(gy, ln_w, xhat, st[:, 1], sums)
    dres = None
    if dresid_old is not None:
        dres = g_in + dresid_old.double() if accumulate_resid else g_in.clone()
    return g_in, dres


# ----------------------------------------------------------------------------------- the mix as out_conv's last operand
def mix_conv(srcs, s, W, bias, stat_shards):
    """V = W cat(srcs, s) + bias over the first (n_src + 1) C columns of W (C, ldw); stat (stat_shards, C, 2): the sums
    of V - bias and its square, 16-column group g going to shard g % stat_shards (None at 0 shards)."""
    C = s.shape[1]
    K = (len(srcs) + 1) * C
    r = conv_fwd_ref(list(srcs) + [s], W.double()[:, :K], bias, 0)
    V = r['U']
    d = V - bias.double()[None, :, None]
    return V, (shard_sums(d, stat_shards) if stat_shards else None)


# -------------------------------------------------------------------------------------------------------------- inputs
def fc_margin(U_fc, scale, shift):
    """the smallest |vf| of the float64 evaluation of the (rounded) inputs"""
    return float(affine(U_fc, scale, shift).abs().min())


def clear_fc_relu(gen, U_fc, mean, rstd, bn_w, bn_b, margin=RELU_MARGIN, tries=8):
    """Choose bn_b of the FC rows so that no vf = scale (u - mean) + bn_b lies within `margin` of zero.  U_fc (b, C, L)
    float32, mean / rstd / bn_w (C) as the case will use them (any dtype), bn_b (C) float32: a channel that is too close
    is redrawn (`tries` times, N(0, 0.2^2) like the first draw), and if that does not clear it, -bn_b is placed in the
    middle of the widest gap of the channel's sorted t = scale (u - mean) values within the range of the draws.
    -> (bn_b float32, the margin reached on the float64 evaluation of the ROUNDED float32 result)."""
    scale = (bn_w.double() * rstd.double())
    t = (U_fc.double() - mean.double()[None, :, None]) * scale[None, :, None]          # vf = t + bn_b
    t = t.permute(1, 0, 2).reshape(t.shape[1], -1)
    out = bn_b.clone().float()

    def dist(bb):
        return (t + bb.double()[:, None]).abs().min(dim=1).values

    for _ in range(tries):
        bad = dist(out) < 2.0 * margin
        if not bool(bad.any()):
            break
        out[bad] = (torch.randn(int(bad.sum()), generator=gen) * 0.2).float()
    bad = (dist(out) < 2.0 * margin).nonzero().reshape(-1)
    for c in bad.tolist():
        v = torch.sort(-t[c]).values                              # bn_b must avoid every -t
        v = v[(v > -1.0) & (v < 1.0)]
        edges = torch.cat([torch.tensor([-1.0], dtype=torch.float64), v, torch.tensor([1.0], dtype=torch.float64)])
        gaps = edges[1:] - edges[:-1]
        i = int(torch.argmax(gaps))
        out[c] = float(0.5 * (edges[i] + edges[i + 1]))
    return out, float(dist(out).min())
