"""-m gpu: the four entry points behind the FC edges of a found network (include/bmnas_hip.h: bmnas_fc_found_fwd,
bmnas_fc_found_bwd_reduce, bmnas_fc_found_bwd_du, bmnas_fc_found_bwd_gemm; the pre-activations come from
bmnas_fc_edges_gemm_fwd with F = 1, once per kind) called directly, against a float64 restatement of
h_e = Dropout(BatchNorm1d(act_e(Linear_e(x_e)))) (reference operations.py:22-65) and its gradients.

Shapes (C, L, b): one 16-channel slab with L / 4 = 1 and 12 columns in a 64-column tile; nsub = 4 with a column tail; a
row tile that ends inside 64; two sample blocks of the reduce / dU kernels (32 samples each), the second with one
sample; the production channel count.

x, W and bias lie on dyadic grids (multiples of 1/4, 1/64 and an odd multiple of 1/512), so every pre-activation is
exact in fp32 whatever the summation order and an odd multiple of 1/512: no ReLU decision is within round-off of zero
(tests/test_fc_edges_gpu.py explains what one such element does to a gradient column)."""
import ctypes as C

import numpy as np
import pytest
import torch

from fc_edges_util import act64, dact64, guarded, guards_intact
from gpu_util import assert_close_of_scale, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

SHAPES = [(16, 4, 3), (32, 16, 5), (80, 8, 9), (32, 8, 33), (192, 16, 6)]
KINDS = [(0,), (1,), (0, 1), (1, 0, 0, 1)]
EPS, MOMENTUM, P_DROP = 1e-5, 0.1, 0.25


def make_case(Cc, L, b, kinds, seed):
    """Per edge: source index, parameters, buffers, incoming gradient (CPU fp32).  E = 4: edges 0 and 2 read the same
    tensor; the last edge's source needs no gradient (E >= 2); a lone Mish edge has no destination at all."""
    rng = np.random.Generator(np.random.PCG64(seed))
    E = len(kinds)
    src = [0, 1, 0, 2][:E]
    n_src = max(src) + 1
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))
    xs = [f32(np.maximum(np.round(rng.standard_normal((b, Cc, L)) * 4) / 4, 0.0)) for _ in range(n_src)]
    edges = []
    for e in range(E):
        W = np.round(rng.uniform(-1, 1, (Cc, Cc)) / np.sqrt(Cc) * 64) / 64
        bias = np.round(0.1 * rng.standard_normal(Cc) * 256) / 256 + 1.0 / 512
        edges.append(dict(src=src[e], mish=kinds[e], W=f32(W), bias=f32(bias),
                          bn_w=f32(1.0 + 0.1 * rng.standard_normal(Cc)), bn_b=f32(0.1 * rng.standard_normal(Cc)),
                          rm=f32(0.1 * rng.standard_normal(Cc)), rv=f32(1.0 + 0.2 * np.abs(rng.standard_normal(Cc))),
                          g=f32(rng.standard_normal((b, Cc, L)))))
    if E == 1:
        need_dx = [kinds[0] == 0]
    else:
        need_dx = [s != src[-1] or src.count(s) > 1 for s in range(n_src)]
    return xs, edges, need_dx


def reference(xs, edges, masks, training, b, Cc, L):
    """float64: per edge U, chan, out, running statistics, bn_grad, dU, dbias, dW; per source dx."""
    n = b * L
    res, dxs = [], [torch.zeros(b, Cc, L, dtype=torch.float64) for _ in xs]
    for e, q in enumerate(edges):
        x = xs[q['src']].double()
        W, bias = q['W'].double(), q['bias'].double()
        U = torch.einsum('mk,bkl->bml', W, x) + bias[None, :, None]
        a = act64(U, q['mish'])
        if training:
            mean = a.mean(dim=(0, 2))
            var = a.var(dim=(0, 2), unbiased=False)
        else:
            mean, var = q['rm'].double(), q['rv'].double()
        rstd = 1.0 / torch.sqrt(var + EPS)
        scale = q['bn_w'].double() * rstd
        shift = q['bn_b'].double() - mean * scale
        m = masks[e].double().view(b, Cc, L)
        out = m * (scale[None, :, None] * a + shift[None, :, None])
        r = dict(U=U, out=out, chan=[mean, rstd, scale, shift])
        if training:
            r['rm'] = (1 - MOMENTUM) * q['rm'].double() + MOMENTUM * mean
            r['rv'] = (1 - MOMENTUM) * q['rv'].double() + MOMENTUM * var * (n / (n - 1.0))
        else:
            r['rm'], r['rv'] = q['rm'].double(), q['rv'].double()
        dy = m * q['g'].double()
        ah = (a - mean[None, :, None]) * rstd[None, :, None]
        s_da, s_dy = (dy * ah).sum(dim=(0, 2)), dy.sum(dim=(0, 2))
        r['bn_grad'] = torch.cat([s_da, s_dy])
        da = dy - (s_dy[None, :, None] + ah * s_da[None, :, None]) / n if training else dy
        dU = scale[None, :, None] * da * dact64(U, q['mish'])
        r['dU'], r['dbias'] = dU, dU.sum(dim=(0, 2))
        r['dW'] = torch.einsum('bml,bkl->mk', dU, x)
        dxs[q['src']] += torch.einsum('mk,bml->bkl', W, dU)
        res.append(r)
    return res, dxs


def run_gpu(xs, edges, need_dx, drops, training, b, Cc, L):
    from bmnas import lib
    E = len(edges)
    d = dev()
    nan = lambda *s: torch.full(s, float('nan'), device=d, dtype=torch.float32)
    xg = [x.to(d) for x in xs]
    prm = [{k: q[k].to(d).contiguous() for k in ('W', 'bias', 'bn_w', 'bn_b', 'rm', 'rv', 'g')} for q in edges]
    nbt = [torch.tensor(7, device=d, dtype=torch.int64) for _ in range(E)]
    U = nan(E, b, Cc, L)
    chan = nan(E, 4 * Cc)
    stat = torch.zeros(E, 2 * Cc, device=d) if training else None
    out_buf, outs, out_keep = guarded(E, (b, Cc, L))
    du_buf, dUs, du_keep = guarded(E, (b, Cc, L))
    pool = torch.zeros(E, 2 * Cc + Cc * Cc + Cc, device=d)
    recs = []
    for e in range(E):
        q = prm[e]
        recs.append(dict(x=xg[edges[e]['src']], U=U[e], dU=dUs[e],
                         fc=[dict(W=q['W'], bias=q['bias'], bn_w=q['bn_w'], bn_b=q['bn_b'], running_mean=q['rm'],
                                  running_var=q['rv'], num_batches_tracked=nbt[e],
                                  stat=None if stat is None else stat[e], chan=chan[e],
                                  bn_grad=pool[e, :2 * Cc], dW=pool[e, 2 * Cc:2 * Cc + Cc * Cc],
                                  dbias=pool[e, 2 * Cc + Cc * Cc:], drop=drops[e], col=0, mish=edges[e]['mish'])]))
    for kind in (0, 1):
        sub = [recs[e] for e in range(E) if edges[e]['mish'] == kind]
        if sub:
            lib.fc_edges_gemm_fwd(lib.make_fc_edges(sub), 1, training, b, Cc, L)
    arr = lib.make_fc_edges(recs)
    lib.fc_found_fwd(arr, training, outs, b, Cc, L)
    gs = [q['g'] for q in prm]
    lib.fc_found_bwd_reduce(arr, gs, b, Cc, L)
    lib.fc_found_bwd_du(arr, gs, training, b, Cc, L)
    src = [q['src'] for q in edges]
    dx_buf, dx_rows, dx_keep = guarded(len(xs), (b, Cc, L))
    targets, masks, which = [], [], []
    for s in range(len(xs)):
        if need_dx[s]:
            targets.append(dx_rows[s])
            masks.append(sum(1 << e for e in range(E) if src[e] == s))
            which.append(s)
    lib.fc_found_bwd_gemm(arr, targets, masks, b, Cc, L)
    torch.cuda.synchronize()
    assert guards_intact(out_buf, out_keep) and guards_intact(du_buf, du_keep)
    # (the rows of the sources that need no gradient are guards too)
    for s in range(len(xs)):
        if not need_dx[s]:
            dx_keep[2 + 3 * s] = True
    assert guards_intact(dx_buf, dx_keep)
    return dict(U=U, chan=chan, outs=outs, dUs=dUs, pool=pool, prm=prm, nbt=nbt, dx={s: dx_rows[s] for s in which})


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('kinds', KINDS, ids=lambda k: 'E%d_%s' % (len(k), ''.join('rm'[i] for i in k)))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'C%d_L%d_b%d' % s)
def test_entry_points_against_float64(shape, kinds, training):
    from bmnas import lib
    Cc, L, b = shape
    E = len(kinds)
    xs, edges, need_dx = make_case(Cc, L, b, kinds, 1100 + 7 * Cc + L + b + E)
    n = b * Cc * L
    # live dropout in the training cases with more than one edge: one site per edge, offsets as _DropState hands out
    live = training and E > 1
    drops = [lib.make_dropout(P_DROP, 1234, e * ((n + 3) // 4)) if live else lib.NO_DROP for e in range(E)]
    masks = [lib.dropout_mask(dr, n, dev()).cpu() for dr in drops]
    if live:
        assert 0.1 < float((torch.stack(masks) == 0).float().mean()) < 0.4
        assert not torch.equal(masks[0], masks[1])
    want, want_dx = reference(xs, edges, masks, training, b, Cc, L)
    got = run_gpu(xs, edges, need_dx, drops, training, b, Cc, L)
    for e in range(E):
        w = want[e]
        assert float(w['U'].abs().min()) >= 1.0 / 512 - 1e-12
        assert torch.equal(got['U'][e].cpu().double(), w['U']), f'U[{e}]'          # exact by construction
        assert_close_of_scale(f'out[{e}]', got['outs'][e], w['out'], rel=1e-4)
        for i, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
            assert_close_of_scale(f'chan[{e}].{name}', got['chan'][e, i * Cc:(i + 1) * Cc], w['chan'][i], rel=1e-4)
        assert_close_of_scale(f'running_mean[{e}]', got['prm'][e]['rm'], w['rm'], rel=1e-4)
        assert_close_of_scale(f'running_var[{e}]', got['prm'][e]['rv'], w['rv'], rel=1e-4)
        assert int(got['nbt'][e]) == 7 + int(training)
        pool = got['pool'][e]
        assert_close_scaled(f'bn_grad[{e}]', pool[:2 * Cc], w['bn_grad'], rel=2e-4)
        assert_close_scaled(f'dU[{e}]', got['dUs'][e], w['dU'], rel=2e-4)
        assert_close_scaled(f'dW[{e}]', pool[2 * Cc:2 * Cc + Cc * Cc].view(Cc, Cc), w['dW'], rel=2e-4)
        assert_close_scaled(f'dbias[{e}]', pool[2 * Cc + Cc * Cc:], w['dbias'], rel=2e-4)
    assert sorted(got['dx']) == [s for s in range(len(xs)) if need_dx[s]]
    for s, dx in got['dx'].items():
        assert_close_scaled(f'dx[{s}]', dx, want_dx[s], rel=2e-4)


def test_argument_errors():
    """BMNAS_E_ARG (-1) first, then BMNAS_E_SHAPE (-2), then BMNAS_E_LIMIT (-3); nothing is launched."""
    from bmnas import lib
    L_ = lib.load()
    Cc, L, b, E = 16, 4, 3, 2
    d = dev()
    t = lambda *s: torch.zeros(*s, device=d)
    x, U, dU, out, g, dx = t(b, Cc, L), t(E, b, Cc, L), t(E, b, Cc, L), t(E, b, Cc, L), t(E, b, Cc, L), t(b, Cc, L)
    chan, stat, pool = t(E, 4 * Cc), t(E, 2 * Cc), t(E, 2 * Cc + Cc * Cc + Cc)
    W, vec = t(Cc, Cc), t(Cc)
    nbt = torch.zeros((), device=d, dtype=torch.int64)

    rm, rv = t(Cc), t(Cc) + 1

    def recs(n=E):
        out_ = []
        for e in range(n):
            i = e % E
            out_.append(dict(x=x, U=U[i], dU=dU[i],
                             fc=[dict(W=W, bias=vec, bn_w=vec, bn_b=vec, running_mean=rm, running_var=rv,
                                      num_batches_tracked=nbt, stat=stat[i], chan=chan[i], bn_grad=pool[i, :2 * Cc],
                                      dW=pool[i, 2 * Cc:2 * Cc + Cc * Cc], dbias=pool[i, 2 * Cc + Cc * Cc:], col=0,
                                      mish=e % 2)]))
        return out_
    P = lambda ts: lib._ptrs(ts)
    masks = (C.c_uint32 * 1)(0b11)
    s = lib._stream()
    outs, gs = [out[0], out[1]], [g[0], g[1]]

    def all_four(arr, n, b_=b, C_=Cc, L_len=L, outs_=None, gs_=None, dxs=None, mk=masks, n_dx=1):
        outs_ = P(outs) if outs_ is None else outs_
        gs_ = P(gs) if gs_ is None else gs_
        dxs = P([dx]) if dxs is None else dxs
        return (L_.bmnas_fc_found_fwd(arr, n, 1, outs_, b_, C_, L_len, s),
                L_.bmnas_fc_found_bwd_reduce(arr, n, gs_, b_, C_, L_len, s),
                L_.bmnas_fc_found_bwd_du(arr, n, gs_, 1, b_, C_, L_len, s),
                L_.bmnas_fc_found_bwd_gemm(arr, n, dxs, mk, n_dx, b_, C_, L_len, s))
    good = lib.make_fc_edges(recs())
    assert all_four(good, E) == (0, 0, 0, 0)
    assert all_four(None, E) == (-1, -1, -1, -1)                         # no edges
    assert all_four(good, 0) == (-1, -1, -1, -1)
    assert all_four(good, E, b_=0) == (-1, -1, -1, -1)                   # b = 0
    assert all_four(lib.make_fc_edges(recs(16)), 16) == (-3, -3, -3, -3)         # E = 16: a limit
    assert all_four(good, E, C_=24) == (-2, -2, -2, -2)                  # C = 24
    assert all_four(good, E, L_len=12) == (-2, -2, -2, -2)               # L = 12
    # null pointers, entry point by entry point
    assert L_.bmnas_fc_found_fwd(good, E, 1, None, b, Cc, L, s) == -1
    assert L_.bmnas_fc_found_bwd_reduce(good, E, None, b, Cc, L, s) == -1
    assert L_.bmnas_fc_found_bwd_du(good, E, None, 1, b, Cc, L, s) == -1
    assert L_.bmnas_fc_found_bwd_gemm(good, E, None, masks, 1, b, Cc, L, s) == -1
    assert L_.bmnas_fc_found_bwd_gemm(good, E, P([dx]), None, 1, b, Cc, L, s) == -1
    assert L_.bmnas_fc_found_bwd_gemm(good, E, None, None, 0, b, Cc, L, s) == 0           # n_dx = 0: no destination
    assert L_.bmnas_fc_found_bwd_gemm(good, E, P([dx]), (C.c_uint32 * 1)(0), 1, b, Cc, L, s) == -1
    assert L_.bmnas_fc_found_bwd_gemm(good, E, P([dx]), (C.c_uint32 * 1)(0b100), 1, b, Cc, L, s) == -1
    assert L_.bmnas_fc_found_bwd_gemm(good, E, P([dx]), masks, 16, b, Cc, L, s) == -1
    for field, hits in (('chan', (-1, -1, -1, 0)), ('bias', (-1, 0, 0, 0)), ('bn_w', (-1, 0, 0, 0)),
                        ('running_mean', (-1, 0, 0, 0)), ('stat', (-1, 0, 0, 0)), ('bn_grad', (0, -1, -1, 0)),
                        ('dbias', (0, 0, -1, 0)), ('dW', (0, 0, 0, -1)), ('edge_dU', (0, 0, -1, -1))):
        r = recs()
        if field.startswith('edge_'):
            r[1][field[5:]] = None
        else:
            r[1]['fc'][0][field] = None
        arr = lib.make_fc_edges(r)
        assert all_four(arr, E) == hits, field
    # a kind outside {0, 1}; dropout configurations that differ in more than the offset
    r = recs()
    r[1]['fc'][0]['mish'] = 2
    assert all_four(lib.make_fc_edges(r), E)[:3] == (-1, -1, -1)
    r = recs()
    r[1]['fc'][0]['drop'] = lib.make_dropout(0.5, 1, 0)
    assert all_four(lib.make_fc_edges(r), E)[:3] == (-1, -1, -1)
    torch.cuda.synchronize()
