"""The multi-head attention of the Attention / MultiHeadAttn primitive (reference models/search/darts/operations.py:67-86:
nn.MultiheadAttention over (b, C, L) tensors, tokens = the L positions, features = the C channels) stated in plain
float64, forward and backward, plus the deterministic inputs of the tests that use it.  tests/test_mha_ref.py pins it
to torch.nn.MultiheadAttention and to the reference's own class (tests/golden/mha.npz).

With W (3C, C), bi (3C), Wo (C, C), bo (C), h heads, d = C / h:
    Q = W[0:C] q + bi[0:C]    K = W[C:2C] k + bi[C:2C]    V = W[2C:3C] v + bi[2C:3C]          (1x1 convs)
    per sample s, head a:  S[i, j] = sum_c Q[s, a d + c, i] K[s, a d + c, j] / sqrt(d),  P = softmax_j(S),
                           P' = mask o P,  O[s, a d + c, i] = sum_j P'[i, j] V[s, a d + c, j]
    out = Wo O + bo
`mask` holds the dropout MULTIPLIERS (0 or 1 / (1 - p)) of the b h L L probabilities, or is None."""
import math

import numpy as np
import torch

# (C, heads, L, b): the shapes of the kernel tests (tests/test_mha_kernels_gpu.py) — d = 4 with the smallest L and a
# ragged last tile, d = 24 (not a multiple of the 16-channel chunk), the two flagship shapes, the largest d
KERNEL_TABLE = [(16, 4, 4, 7), (16, 2, 8, 5), (16, 1, 16, 1), (48, 2, 16, 5), (32, 8, 8, 6), (128, 2, 8, 7),
                (192, 2, 16, 5), (512, 4, 4, 3), (512, 1, 16, 2)]
DROP_P, DROP_SEED, DROP_OFFSET = 0.25, 0x5EED0123456789, 3 << 33


def gen(seed):
    return np.random.Generator(np.random.PCG64(seed))


def rand(g, *shape):
    """uniform in [-1, 1), fp32"""
    return torch.from_numpy((g.random(shape) * 2.0 - 1.0).astype(np.float32))


def case_seed(C, heads, L, b):
    return 1700 + 7 * C + 131 * heads + 17 * L + b


def make_core_inputs(C, heads, L, b):
    """Projected operands of the core kernels and the gradient of O.  |Q|, |K| < 1.5: the scores are sums of d
    products of variance 9/16 each, divided by sqrt(d) — standard deviation 0.75 whatever d, far from saturation."""
    g = gen(case_seed(C, heads, L, b))
    return {'Q': rand(g, b, C, L) * 1.5, 'K': rand(g, b, C, L) * 1.5, 'V': rand(g, b, C, L), 'dO': rand(g, b, C, L)}


def make_params(C, seed):
    """in_proj / out_proj parameters with torch's keys.  Weights uniform in +-3 / sqrt(C): with inputs uniform in
    [-1, 1) the projections have variance 1 and the scores standard deviation ~1; biases in +-0.1."""
    g = gen(seed)
    a = 3.0 / math.sqrt(C)
    return {'in_proj_weight': rand(g, 3 * C, C) * a, 'in_proj_bias': rand(g, 3 * C) * 0.1,
            'out_proj.weight': rand(g, C, C) * a, 'out_proj.bias': rand(g, C) * 0.1}


def make_inputs(C, L, b, seed):
    """q, k, v and the output gradient g, uniform in [-1, 1)."""
    g = gen(seed + 1)
    return {'q': rand(g, b, C, L), 'k': rand(g, b, C, L), 'v': rand(g, b, C, L), 'g': rand(g, b, C, L)}


def _heads(t, heads):
    b, C, L = t.shape
    return t.reshape(b, heads, C // heads, L)


def core_ref(Q, K, V, heads, dO=None, mask=None):
    """The per-head core in float64 -> dict(O, P[, dQ, dK, dV]).  mask: (b, heads, L, L) multipliers or None."""
    Q, K, V = Q.double(), K.double(), V.double()
    b, C, L = Q.shape
    d = C // heads
    Qh, Kh, Vh = _heads(Q, heads), _heads(K, heads), _heads(V, heads)
    S = torch.einsum('bhci,bhcj->bhij', Qh, Kh) / math.sqrt(d)
    P = torch.softmax(S, -1)
    m = torch.ones_like(P) if mask is None else mask.double().reshape(b, heads, L, L)
    Pd = P * m
    out = {'P': P, 'O': torch.einsum('bhij,bhcj->bhci', Pd, Vh).reshape(b, C, L)}
    if dO is not None:
        dOh = _heads(dO.double(), heads)
        dP = torch.einsum('bhci,bhcj->bhij', dOh, Vh) * m
        dS = P * (dP - (dP * P).sum(-1, keepdim=True))
        out['dV'] = torch.einsum('bhij,bhci->bhcj', Pd, dOh).reshape(b, C, L)
        out['dQ'] = (torch.einsum('bhij,bhcj->bhci', dS, Kh) / math.sqrt(d)).reshape(b, C, L)
        out['dK'] = (torch.einsum('bhij,bhci->bhcj', dS, Qh) / math.sqrt(d)).reshape(b, C, L)
    return out


def mha_ref(q, k, v, params, heads, g=None, mask=None):
    """The whole operation in float64 -> dict(out, P[, dq, dk, dv, and the four parameter gradients under torch's
    keys]).  dq / dk / dv are the gradients of the three ROLES: a tensor that plays several roles gets their sum."""
    W, bi = params['in_proj_weight'].double(), params['in_proj_bias'].double()
    Wo, bo = params['out_proj.weight'].double(), params['out_proj.bias'].double()
    C = Wo.shape[0]
    xs = [q.double(), k.double(), v.double()]
    proj = [torch.einsum('mc,bcl->bml', W[r * C:(r + 1) * C], xs[r]) + bi[r * C:(r + 1) * C, None] for r in range(3)]
    dO = None if g is None else torch.einsum('mc,bml->bcl', Wo, g.double())
    core = core_ref(proj[0], proj[1], proj[2], heads, dO, mask)
    res = {'out': torch.einsum('mc,bcl->bml', Wo, core['O']) + bo[None, :, None], 'P': core['P']}
    if g is None:
        return res
    gd = g.double()
    res['out_proj.weight'] = torch.einsum('bml,bcl->mc', gd, core['O'])
    res['out_proj.bias'] = gd.sum((0, 2))
    dproj = [core['dQ'], core['dK'], core['dV']]
    res['in_proj_weight'] = torch.cat([torch.einsum('bml,bcl->mc', dproj[r], xs[r]) for r in range(3)], 0)
    res['in_proj_bias'] = torch.cat([dproj[r].sum((0, 2)) for r in range(3)], 0)
    for r, name in enumerate(('dq', 'dk', 'dv')):
        res[name] = torch.einsum('mc,bml->bcl', W[r * C:(r + 1) * C], dproj[r])
    return res


PARAM_KEYS = ('in_proj_weight', 'in_proj_bias', 'out_proj.weight', 'out_proj.bias')


def rel_err(got, want):
    """max |got - want| / (|want| + max|want|): the quantity gpu_util.assert_close_scaled bounds."""
    g = np.asarray(got.detach().cpu().double().numpy() if torch.is_tensor(got) else got, dtype=np.float64)
    w = np.asarray(want.detach().cpu().double().numpy() if torch.is_tensor(want) else want, dtype=np.float64)
    assert g.shape == w.shape, (g.shape, w.shape)
    scale = np.abs(w) + np.abs(w).max()
    r = np.abs(g - w) / np.where(scale > 0, scale, 1.0)
    return float(np.max(np.where(np.isfinite(r), r, np.inf)))
