"""The whole head — bmnas_head_fwd / _lazy, then bmnas_head_bwd / _lazy and their _crit forms (csrc/head.hip) — against the
float64 statement of tests/lazy_ln_ref.py (K7 LayerNorm over the concatenation, ReLU, classifier, criterion; with the lazy
forms the node LayerNorm in front) and tests/crit_ref.py, at the shapes where the backward's tile phase changes path:

  C L = 64 | 128        one or two 64-k workgroups per state; 2 and 3 states
  b                     1, 15, 17, 33: ragged against the 16-row MFMA group and the chunk count; 65, 81: the 32-row chunks
                        (b >= 64, two sample groups per workgroup) with one row / one group and a row in the last chunk
  O                     1, 3, 16, 17, 23, 33, 65, 97: the class-step edge (O + 3) / 4, the class-tile edge, every change of
                        the class-tile count the kernel is built for (2, 4, 6, 8)
  modes 0, 1, 2; the lazy forms on and off; weighted BCE and weighted, smoothed CrossEntropy with ignore_index;
  acc_mask with no, one and both bits over pre-filled gradients; part = None (the architecture step).

The backward is fed what the forward launch left (hb, stats, the lazy source's node statistics).  Compared: state
gradients, the summed part rows (dW, dln_w, dln_b, dbias), lnpart and the loss.  Bounds: those of
tests/test_lazy_ln_kernels_gpu.py and tests/test_crit_head_gpu.py for the same quantities (1e-4 of the expected tensor's
scale against float64).  Every output buffer starts as NaN: an element no lane writes fails."""
import pytest
import torch

import crit_ref
import lazy_ln_ref as lr
from gpu_util import assert_close_scaled, dev
from test_lazy_ln_kernels_gpu import LOSS0, _criterion, _gen, _head_inputs, _nan, _rand, _records32

pytestmark = pytest.mark.gpu

BS = [1, 15, 17, 33, 65, 81]
OS = [1, 3, 16, 17, 23, 33, 65, 97]
GS = 0.37


def _to(x):
    return None if x is None else x.to(dev())


def _forward(t, C, L, O, b, lazy):
    """-> hb (3, b, O), stats (b, 2), per source the node statistics the backward's lazy form reads (the lazy source's:
    written by the launch), all on the device"""
    from bmnas import lib
    d = dev()
    n_src = len(t.pre)
    ln_w, ln_b, W, bias = _to(t.ln_w), _to(t.ln_b), _to(t.W), _to(t.bias)
    hb, stats = torch.zeros(3, b, O, device=d), _nan(b, 2)
    srcs, sums = [_to(n) for n in t.n32], [_to(s) for s in t.sums]
    nstats = [_to(s) for s in t.nstats]
    if lazy:
        q = n_src - 1
        rec, prm = _records32(t.pre[q], t.nw[q], t.nb[q])
        nstats[q] = _nan(b, 2)
        keep = (_to(t.pre[q]), _to(rec), _to(prm), _to(t.nw[q]), _to(t.nb[q]))    # (the descriptor holds addresses only)
        lz = lib.make_lazy(keep[0], keep[1], keep[2], keep[3], keep[4], nstats[q])
        srcs[q], sums[q] = keep[0], None
        lib.head_fwd_lazy(srcs, sums, q, lz, ln_w, ln_b, W, bias, hb, stats, b, C, L, O)
    else:
        lib.head_fwd(srcs, sums, ln_w, ln_b, W, bias, hb, stats, b, C, L, O)
    torch.cuda.synchronize()
    return hb, stats, nstats


def _backward(t, fwd, C, L, O, b, lazy, mode, labels, gl, gscale, acc=0, old=None, want_part=True, crit_kw=None):
    from bmnas import lib
    d = dev()
    n_src = len(t.pre)
    D = n_src * C * L
    hb, stats, nstats = fwd
    ln_w, ln_b, W = _to(t.ln_w), _to(t.ln_b), _to(t.W)
    dsrcs = [old[q].clone().to(d) if (acc >> q) & 1 else _nan(b, C, L) for q in range(n_src)]
    n_chunk = lib.head_chunks(b)
    part = _nan(n_chunk, O + 3, D) if want_part else None
    loss = torch.full((1,), LOSS0, device=d)
    gsc = torch.full((1,), GS, device=d) if gscale else None
    crit, keep = None, None
    if crit_kw is not None:
        keep = (_to(crit_kw['weight']), _to(crit_kw['pos_weight']))
        crit = lib.Criterion('bce' if mode == 1 else 'ce', weight=keep[0], pos_weight=keep[1],
                             label_smoothing=crit_kw['label_smoothing'], ignore_index=crit_kw['ignore_index'],
                             reduction=crit_kw['reduction'])
    res = dict(dsrcs=dsrcs, loss=loss)
    if lazy:
        srcs = [(_to(t.pre[q]), _to(t.nw[q]), _to(t.nb[q]), nstats[q]) for q in range(n_src)]
        lz = [lib.make_lazy(p, None, None, w_, b_, s_) for p, w_, b_, s_ in srcs]
        lnparts = [_nan(b, C * L // 64, 2) for _ in range(n_src)]
        lib.head_bwd_lazy(lz, lnparts, dsrcs, acc, ln_w, ln_b, W, hb, stats, mode, _to(gl), gsc, _to(labels), loss, part,
                          b, C, L, O, crit=crit)
        res['lnparts'] = lnparts
    else:
        lib.head_bwd([_to(n) for n in t.n32], [_to(s) for s in t.sums], dsrcs, acc, ln_w, ln_b, W, hb, stats, mode,
                     _to(gl), gsc, _to(labels), loss, part, b, C, L, O, crit=crit)
    if want_part:
        summed = _nan(O + 3, D)
        lib.sum_chunks(part, summed, n_chunk)
        res.update(dW=summed[:O], dln_w=summed[O], dln_b=summed[O + 1], dbias=summed[O + 2, :O])
    torch.cuda.synchronize()
    return res


def _check_forward(t, fwd, lazy, name):
    hb, stats, nstats = fwd
    for v, nm in enumerate(['logits', 'A', 'B']):
        assert_close_scaled(f'{nm} {name}', hb[v], t.fw[nm])
    for c_, nm in enumerate(('mean', 'rstd')):
        assert_close_scaled(f'stats {nm} {name}', stats[:, c_], t.fw[nm])
    if lazy:
        mean, rstd = lr.moments(t.pre[-1])
        assert_close_scaled(f'lazy->stats mean {name}', nstats[-1][:, 0], mean)
        assert_close_scaled(f'lazy->stats rstd {name}', nstats[-1][:, 1], rstd)


def _check_backward(t, got, dl, loss64, lazy, mode, name, acc=0, old=None, want_part=True):
    bw = lr.head_bwd(t.fw, t.ln_w, t.W, dl)
    for q in range(len(t.pre)):
        want = bw['dn'][q] + (old[q].double() if (acc >> q) & 1 else 0.0)
        assert_close_scaled(f'dsrcs[{q}] {name}', got['dsrcs'][q], want)
        if lazy:
            lnp = lr.ln_partials(bw['dn'][q], t.nw[q], t.xhat[q], lr.GROUP)
            assert_close_scaled(f'lnpart[{q}] S(gy w) {name}', got['lnparts'][q][:, :, 0], lnp[:, :, 0])
            assert_close_scaled(f'lnpart[{q}] S(gy w xhat) {name}', got['lnparts'][q][:, :, 1], lnp[:, :, 1])
    if want_part:
        for k in ('dW', 'dln_w', 'dln_b', 'dbias'):
            assert_close_scaled(f'{k} {name}', got[k], bw[k])
    if mode == 0:
        assert float(got['loss']) == LOSS0
    else:
        assert_close_scaled('loss ' + name, got['loss'] - LOSS0, torch.as_tensor(loss64, dtype=torch.float64).reshape(1))


def _shape(io, ib):
    """(C, L, n_src) of the (O, b) pair: both C L and both state counts meet every O and every b"""
    return (4, 8)[(io + ib) % 2], 16, 2 + ((io + (ib >> 1)) % 2)


@pytest.mark.parametrize('b', BS)
@pytest.mark.parametrize('O', OS)
def test_head_forward_then_backward(O, b):
    io, ib = OS.index(O), BS.index(b)
    C, L, n_src = _shape(io, ib)
    g = _gen(9000 + 131 * O + b)
    t = _head_inputs(g, C, L, n_src, O, b, False)
    for lazy in (False, True):
        fwd = _forward(t, C, L, O, b, lazy)
        _check_forward(t, fwd, lazy, f'lazy={lazy}')
        for mode in (0, 1, 2):
            gscale = (io + ib + mode) % 2 == 1
            labels, gl, loss64, dl = _criterion(g, t, mode, O, b, gscale)
            got = _backward(t, fwd, C, L, O, b, lazy, mode, labels, gl, gscale)
            _check_backward(t, got, dl, loss64, lazy, mode, f'lazy={lazy} mode={mode}')


@pytest.mark.parametrize('lazy', [False, True])
@pytest.mark.parametrize('C,n_src,O,b', [(4, 2, 23, 17), (8, 3, 33, 33), (4, 3, 65, 65), (8, 2, 17, 81)])
def test_weighted_criteria(C, n_src, O, b, lazy):
    """one weighted BCE (weight and pos_weight, sum) and one weighted, smoothed CrossEntropy with ignore_index (mean)"""
    L = 16
    g = _gen(9100 + C + n_src + O + b)
    t = _head_inputs(g, C, L, n_src, O, b, False)
    fwd = _forward(t, C, L, O, b, lazy)
    w, p = 0.25 + 2.0 * torch.rand(O, generator=g), 0.25 + 2.0 * torch.rand(O, generator=g)
    y = (torch.rand(b, O, generator=g) < 0.3).float()
    loss64, dl = crit_ref.bce(t.fw['logits'], y, w, p, 'sum')
    kw = dict(weight=w, pos_weight=p, label_smoothing=0.0, ignore_index=-100, reduction='sum')
    got = _backward(t, fwd, C, L, O, b, lazy, 1, y, None, True, crit_kw=kw)
    _check_backward(t, got, dl * GS, loss64, lazy, 1, 'weighted bce')
    ign = O - 1
    lab = torch.randint(0, O - 1, (b,), generator=g)
    lab[::3] = ign
    lab[-1] = 0                                                   # (b = 17: at least one row counts)
    loss64, dl = crit_ref.ce(t.fw['logits'], lab, w, 0.1, ign, 'mean')
    kw = dict(weight=w, pos_weight=None, label_smoothing=0.1, ignore_index=ign, reduction='mean')
    got = _backward(t, fwd, C, L, O, b, lazy, 2, lab, None, False, crit_kw=kw)
    _check_backward(t, got, dl, loss64, lazy, 2, 'weighted smoothed ce')


@pytest.mark.parametrize('lazy', [False, True])
@pytest.mark.parametrize('acc', [0b00, 0b10, 0b11])
@pytest.mark.parametrize('C,O,b', [(4, 23, 33), (8, 65, 81)])
def test_accumulating_calls(C, O, b, acc, lazy):
    L, n_src = 16, 2
    g = _gen(9200 + C + O + b)
    t = _head_inputs(g, C, L, n_src, O, b, False)
    fwd = _forward(t, C, L, O, b, lazy)
    old = [_rand(g, b, C, L) for _ in range(n_src)]
    labels, gl, loss64, dl = _criterion(g, t, 1, O, b, False)
    got = _backward(t, fwd, C, L, O, b, lazy, 1, labels, gl, False, acc=acc, old=old)
    _check_backward(t, got, dl, loss64, lazy, 1, f'acc={acc:02b}', acc=acc, old=old)


@pytest.mark.parametrize('lazy', [False, True])
@pytest.mark.parametrize('C,n_src,O,b,mode', [(4, 2, 23, 15, 1), (8, 3, 17, 65, 2), (4, 3, 97, 33, 0)])
def test_no_part(C, n_src, O, b, mode, lazy):
    """part = NULL: the state gradients, lnpart and the loss alone"""
    L = 16
    g = _gen(9300 + C + n_src + O + b)
    t = _head_inputs(g, C, L, n_src, O, b, False)
    fwd = _forward(t, C, L, O, b, lazy)
    labels, gl, loss64, dl = _criterion(g, t, mode, O, b, True)
    got = _backward(t, fwd, C, L, O, b, lazy, mode, labels, gl, True, want_part=False)
    _check_backward(t, got, dl, loss64, lazy, mode, 'no part', want_part=False)
