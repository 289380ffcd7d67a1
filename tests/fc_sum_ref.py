"""float64 restatement of a mixed-edge sum whose primitives hold fc_relu / fc_mish (csrc/fcedge.hip, the search-stage
family), of its gradients, and the cases tests/test_fc_edges_kernels_gpu.py runs it at.  Needs no GPU;
tests/test_fc_sum_ref.py checks it against the CPU oracle, torch.autograd and a finite difference.

Per edge j (reading state src[j]) and participating column p of the weight rows w (n, P):

    out = sum_j [ (sum_{p in skip} w[j, p]) x_j + sum_f w[j, col_f] mask_jf BN_jf(act_f(W_jf x_j + bias_jf)) ]

with f over the FC primitives in list order, col_f their columns, `none` columns contributing nothing.  Training uses
batch statistics and the biased-variance gradient, eval the running statistics and da = dy."""
import numpy as np
import torch

from fc_edges_util import act64, dact64

EPS, MOMENTUM, P_DROP = 1e-5, 0.1, 0.25
KIND = {'fc_relu': 0, 'fc_mish': 1}
# the shifted-variance case (CASES[1]'s shape): the constant on every fc_relu bias and the seed of its inputs
SHIFT_BIAS, SHIFT_SEED = 128.0, 2100

# (C, L, b, prims (one per column), src (the state every edge reads), need_dx (per state))
CASES = [
    (16, 4, 3, ['fc_mish'], [0], [False]),
    (16, 4, 3, ['none', 'fc_relu', 'fc_mish', 'skip'], [0, 1], [True, True]),
    (48, 8, 9, ['fc_mish', 'skip', 'none', 'fc_relu'], [0, 1, 2], [True, True, True]),
    (80, 16, 33, ['none', 'skip', 'fc_relu'], [0, 1], [True, True]),
    (32, 8, 5, ['fc_relu', 'skip'], [0, 0], [True]),
    (32, 8, 5, ['skip', 'fc_mish', 'fc_relu'], [0, 1, 0, 2], [True, True, False]),
    (16, 4, 2, ['skip', 'none', 'fc_relu', 'none', 'skip', 'fc_mish', 'none', 'none'], list(range(15)), [True] * 15),
    (192, 16, 6, ['none', 'fc_relu', 'fc_mish', 'skip'], [0, 1], [True, True]),
]


def case_id(case):
    Cc, L, b, prims, src, _ = case
    return 'C%d_L%d_b%d_n%d_%s' % (Cc, L, b, len(src), '+'.join(prims))


def columns(prims):
    """-> (columns of the FC primitives in list order, their kinds (0 ReLU | 1 Mish), bit mask of the skip columns)."""
    fcols = [c for c, name in enumerate(prims) if name in KIND]
    assert all(name in KIND or name in ('none', 'skip') for name in prims)
    return fcols, [KIND[prims[c]] for c in fcols], sum(1 << c for c, name in enumerate(prims) if name == 'skip')


def make_case(case, seed, relu_bias_shift=0.0):
    """CPU fp32 inputs on dyadic grids (x multiples of 1/4, W of 1/64, bias an odd multiple of 1/512: every
    pre-activation is exact in fp32 in any summation order and an odd multiple of 1/512), a softmax weight row per edge
    and an incoming gradient.  relu_bias_shift: a dyadic constant added to every fc_relu bias.
    -> (xs, edges[j][f] dicts, w (n, P), g)."""
    Cc, L, b, prims, src, _ = case
    rng = np.random.Generator(np.random.PCG64(seed))
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    fcols, kinds, _ = columns(prims)
    n, P = len(src), len(prims)
    xs = [f32(np.maximum(np.round(rng.standard_normal((b, Cc, L)) * 4) / 4, 0.0)) for _ in range(max(src) + 1)]
    edges = []
    for _ in range(n):
        fc = []
        for kind in kinds:
            W = np.round(rng.uniform(-1, 1, (Cc, Cc)) / np.sqrt(Cc) * 64) / 64
            bias = np.round(0.1 * rng.standard_normal(Cc) * 256) / 256 + 1.0 / 512
            if kind == 0:
                bias = bias + relu_bias_shift
            fc.append(dict(mish=kind, W=f32(W), bias=f32(bias), bn_w=f32(1.0 + 0.1 * rng.standard_normal(Cc)),
                           bn_b=f32(0.1 * rng.standard_normal(Cc)), rm=f32(0.1 * rng.standard_normal(Cc)),
                           rv=f32(1.0 + 0.2 * np.abs(rng.standard_normal(Cc)))))
        edges.append(fc)
    w = torch.softmax(f32(0.5 * rng.standard_normal((n, P))), -1)
    g = f32(rng.standard_normal((b, Cc, L)))
    return xs, edges, w, g


def reference(case, xs, edges, w, g, masks, training):
    """float64.  masks[j][f]: the dropout multipliers of site (j, f), flat or (b, C, L).
    -> dict out, dw (n, P), dx (one per state, zero where no edge reads it), fc[j][f] = dict U, chan (mean, rstd, scale,
    shift), rm, rv (the updated running statistics), bn_grad (dBN.weight | dBN.bias), dU, dbias, dW."""
    Cc, L, b, prims, src, _ = case
    fcols, kinds, skip_cols = columns(prims)
    n, P, N = len(src), len(prims), b * L
    w, g = w.double(), g.double()
    out = torch.zeros(b, Cc, L, dtype=torch.float64)
    dw = torch.zeros(n, P, dtype=torch.float64)
    dxs = [torch.zeros(b, Cc, L, dtype=torch.float64) for _ in xs]
    res = []
    for j in range(n):
        x = xs[src[j]].double()
        ws = sum(w[j, p] for p in range(P) if (skip_cols >> p) & 1)
        if skip_cols:
            out += ws * x
            dxs[src[j]] += ws * g
            for p in range(P):
                if (skip_cols >> p) & 1:
                    dw[j, p] = (g * x).sum()
        row = []
        for f, q in enumerate(edges[j]):
            W, bias = q['W'].double(), q['bias'].double()
            U = torch.einsum('mk,bkl->bml', W, x) + bias[None, :, None]
            a = act64(U, kinds[f])
            if training:
                mean = a.mean(dim=(0, 2))
                var = a.var(dim=(0, 2), unbiased=False)
            else:
                mean, var = q['rm'].double(), q['rv'].double()
            rstd = 1.0 / torch.sqrt(var + EPS)
            scale = q['bn_w'].double() * rstd
            shift = q['bn_b'].double() - mean * scale
            m = masks[j][f].double().view(b, Cc, L)
            o = m * (scale[None, :, None] * a + shift[None, :, None])
            wf = w[j, fcols[f]]
            out += wf * o
            dw[j, fcols[f]] = (g * o).sum()
            r = dict(U=U, chan=[mean, rstd, scale, shift])
            if training:
                r['rm'] = (1 - MOMENTUM) * q['rm'].double() + MOMENTUM * mean
                r['rv'] = (1 - MOMENTUM) * q['rv'].double() + MOMENTUM * var * (N / (N - 1.0))
            else:
                r['rm'], r['rv'] = q['rm'].double(), q['rv'].double()
            dy = wf * m * g
            ah = (a - mean[None, :, None]) * rstd[None, :, None]
            s_da, s_dy = (dy * ah).sum(dim=(0, 2)), dy.sum(dim=(0, 2))
            r['bn_grad'] = torch.cat([s_da, s_dy])
            da = dy - (s_dy[None, :, None] + ah * s_da[None, :, None]) / N if training else dy
            dU = scale[None, :, None] * da * dact64(U, kinds[f])
            r['dU'], r['dbias'] = dU, dU.sum(dim=(0, 2))
            r['dW'] = torch.einsum('bml,bkl->mk', dU, x)
            dxs[src[j]] += torch.einsum('mk,bml->bkl', W, dU)
            row.append(r)
        res.append(row)
    return dict(out=out, dw=dw, dx=dxs, fc=res)


def emulated_batch_stats(U, bias, mish, shifted, tree):
    """fp32 numpy emulation of the two ways a kernel may form one channel's batch statistics from its N pre-activations
    U (N,) fp32: shifted — sums of d = act(u) - act(bias) and d^2, mean = act(bias) + E[d], var = E[d^2] - E[d]^2 (what
    fc_gemm_fwd_k / fc_mix_fwd_k do) — or not (sums of act(u) and act(u)^2).  tree: pairwise instead of sequential
    summation (the kernel sums lanes by a butterfly).  -> (mean, var) as fp32."""
    f = np.float32
    act = (lambda u: (u * np.tanh(np.log1p(np.exp(u, dtype=f)), dtype=f)).astype(f)) if mish else \
        (lambda u: np.maximum(u, f(0)))
    sh = act(np.asarray([bias], dtype=f))[0] if shifted else f(0)
    d = (act(U.astype(f)) - sh).astype(f)

    def total(v):
        v = [f(t) for t in v]
        if tree:
            while len(v) > 1:
                v = [f(v[i] + v[i + 1]) if i + 1 < len(v) else v[i] for i in range(0, len(v), 2)]
            return v[0]
        s = f(0)
        for t in v:
            s = f(s + t)
        return s
    nN = f(len(U))
    md = f(total(d) / nN)
    var = np.maximum(f(f(total((d * d).astype(f)) / nN) - f(md * md)), f(0))
    return f(sh + md), var
