"""The weighted / smoothed criteria inside the head's backward launch (csrc/head.hip:
bmnas_head_bwd_crit, bmnas_head_bwd_lazy_crit and its loss_part form) against float64 — the head of
tests/lazy_ln_ref.py fed with the dlogits of tests/crit_ref.py — and against the SAME launch in mode 0
given those dlogits, at the kernel-vs-kernel bound of tests/test_lazy_ln_kernels_gpu.py.

(C, L, n_src, O, b): O = 5 a partly filled class stripe; O = 17 a second stripe holding one class; O = 128 every
stripe of the widest instantiation with O == D; O = 83 and b = 65 the 32-sample chunks with a ragged last one (one
row); b = 37 the 16-sample chunks with a ragged last one; O = 23, C L = 3072 the MM-IMDB head."""
import pytest
import torch

import crit_ref
import lazy_ln_ref as lr
from gpu_util import assert_close_scaled, dev
from test_lazy_ln_kernels_gpu import KK, LOSS0, _gen, _head_inputs, _nan, _rand

pytestmark = pytest.mark.gpu

SHAPES = [(16, 4, 1, 5, 1), (16, 4, 2, 17, 17), (16, 4, 2, 128, 33), (128, 8, 2, 83, 65), (192, 16, 2, 23, 37)]
GS = 0.37
CONFIGS = [  # kind, weight, pos_weight, label_smoothing, ignore ('none' | 'some' | 'neg' | 'all'), reduction, gscale
    ('bce', False, True, 0.0, 'none', 'mean', False),
    ('bce', True, True, 0.0, 'none', 'sum', True),
    ('bce', True, False, 0.0, 'none', 'mean', False),
    ('ce', True, False, 0.0, 'none', 'mean', False),
    ('ce', True, False, 0.1, 'some', 'mean', True),
    ('ce', False, False, 0.1, 'neg', 'sum', False),
    ('ce', True, False, 0.1, 'all', 'mean', False),
]


def _vec(g, O, on):
    return (0.25 + 2.0 * torch.rand(O, generator=g)) if on else None


def _case(g, t, O, b, cfg):
    """-> labels (CPU, as the kernel takes them), lib.Criterion arguments, float64 loss and dlogits (gscale applied)"""
    kind, use_w, use_p, eps, ignore, reduction, gscale = cfg
    w, p = _vec(g, O, use_w), _vec(g, O, use_p)
    z = t.fw['logits']
    if kind == 'bce':
        y = (torch.rand(b, O, generator=g) < 0.3).float()
        loss, dl = crit_ref.bce(z, y, w, p, reduction)
        ign = -100
    else:
        y = torch.randint(0, O, (b,), generator=g)
        ign = {'none': -100, 'some': O - 1, 'neg': -1, 'all': -1}[ignore]
        if ignore == 'some':
            y[y == ign] = 0
        if ignore in ('some', 'neg') and b > 1:
            y[::3] = ign
        if ignore == 'all':
            y[:] = ign
        loss, dl = crit_ref.ce(z, y, w, eps, ign, reduction)
    return y, dict(weight=w, pos_weight=p, label_smoothing=eps, ignore_index=ign, reduction=reduction), loss, \
        dl * (GS if gscale else 1.0)


def _launch(t, C, L, O, b, form, mode, labels, gl, gscale, crit_kw):
    """form: 'plain' | 'lazy' | 'det' (lazy with loss_part).  mode 0: gl = dlogits; else the criterion `crit_kw`."""
    from bmnas import lib
    d = dev()
    n_src = len(t.pre)
    D = n_src * C * L
    to = lambda x: None if x is None else x.to(d)
    ln_w, ln_b, W = to(t.ln_w), to(t.ln_b), to(t.W)
    hb = torch.stack([t.fw['logits'], t.fw['A'], t.fw['B']]).float().contiguous().to(d)
    stats = torch.stack([t.fw['mean'], t.fw['rstd']], 1).float().contiguous().to(d)
    dsrcs = [_nan(b, C, L) for _ in range(n_src)]
    n_chunk = lib.head_chunks(b)
    part = _nan(n_chunk, O + 3, D)
    loss = torch.full((1,), LOSS0, device=d)
    gsc = torch.full((1,), GS, device=d) if gscale else None
    crit, keep = None, None
    if mode != 0:
        keep = (to(crit_kw['weight']), to(crit_kw['pos_weight']))
        crit = lib.Criterion('bce' if mode == 1 else 'ce', weight=keep[0], pos_weight=keep[1],
                             label_smoothing=crit_kw['label_smoothing'], ignore_index=crit_kw['ignore_index'],
                             reduction=crit_kw['reduction'])
    res = dict(dsrcs=dsrcs, loss=loss)
    if form == 'plain':
        lib.head_bwd([to(n) for n in t.n32], [to(s) for s in t.sums], dsrcs, 0, ln_w, ln_b, W, hb, stats, mode, to(gl),
                     gsc, to(labels), loss, part, b, C, L, O, crit=crit)
    else:
        srcs = [(to(t.pre[q]), to(t.nw[q]), to(t.nb[q]), to(t.nstats[q])) for q in range(n_src)]
        lz = [lib.make_lazy(p, None, None, w_, b_, s_) for p, w_, b_, s_ in srcs]
        lnparts = [_nan(b, C * L // 64, 2) for _ in range(n_src)]
        loss_part = _nan(n_chunk) if (form == 'det' and mode != 0) else None
        lib.head_bwd_lazy(lz, lnparts, dsrcs, 0, ln_w, ln_b, W, hb, stats, mode, to(gl), gsc, to(labels), loss, part,
                          b, C, L, O, loss_part=loss_part, crit=crit)
        res.update(lnparts=lnparts, loss_part=loss_part)
    summed = _nan(O + 3, D)
    lib.sum_chunks(part, summed, n_chunk)
    torch.cuda.synchronize()
    res.update(dW=summed[:O], dln_w=summed[O], dln_b=summed[O + 1], dbias=summed[O + 2, :O])
    return res


@pytest.mark.parametrize('form', ['plain', 'lazy', 'det'])
@pytest.mark.parametrize('C,L,n_src,O,b', SHAPES)
def test_head_bwd_with_criterion_descriptor(C, L, n_src, O, b, form):
    g = _gen(8000 + C + L + n_src + O + b)
    t = _head_inputs(g, C, L, n_src, O, b, False)
    for cfg in CONFIGS:
        kind, gscale, name = cfg[0], cfg[6], ' '.join(map(str, cfg))
        labels, crit_kw, loss64, dl = _case(g, t, O, b, cfg)
        bw = lr.head_bwd(t.fw, t.ln_w, t.W, dl)
        mode = 1 if kind == 'bce' else 2
        got = _launch(t, C, L, O, b, form, mode, labels, None, gscale, crit_kw)
        # mode 0 of the same launch on the float64 dlogits (rounded to fp32; gscale applied by the launch as well)
        ref = _launch(t, C, L, O, b, form, 0, None, (dl / (GS if gscale else 1.0)).float(), gscale, None)
        for q in range(n_src):
            assert_close_scaled(f'dsrcs[{q}] {name}', got['dsrcs'][q], bw['dn'][q])
            assert_close_scaled(f'dsrcs[{q}] vs mode 0 {name}', got['dsrcs'][q], ref['dsrcs'][q].cpu(), rel=KK)
            if form != 'plain':
                for c_, nm in enumerate(('S(gy w)', 'S(gy w xhat)')):
                    assert_close_scaled(f'lnpart[{q}] {nm} vs mode 0 {name}', got['lnparts'][q][:, :, c_],
                                        ref['lnparts'][q][:, :, c_].cpu(), rel=KK)
        for k in ('dW', 'dbias', 'dln_w', 'dln_b'):
            assert_close_scaled(f'{k} {name}', got[k], bw[k])
            assert_close_scaled(f'{k} vs mode 0 {name}', got[k], ref[k].cpu(), rel=KK)
        if form == 'det':
            assert float(got['loss']) == LOSS0                    # the caller sums the chunks' shares: *loss stays
            loss = got['loss_part'].sum().reshape(1)
        else:
            loss = got['loss'] - LOSS0
        if cfg[4] == 'all':                                       # mean over no row: NaN loss, zero gradients (torch)
            assert torch.isnan(loss).all() and torch.isnan(loss64)
            assert all(float(ds.abs().sum()) == 0.0 for ds in got['dsrcs']) and float(got['dW'].abs().sum()) == 0.0
        else:
            assert_close_scaled('loss ' + name, loss, loss64.reshape(1))
        if form == 'det':                                         # plain stores, fixed order: bit-identical again
            again = _launch(t, C, L, O, b, form, mode, labels, None, gscale, crit_kw)
            assert torch.equal(got['loss_part'], again['loss_part']) or cfg[4] == 'all'
            for k in ('dW', 'dbias', 'dln_w', 'dln_b'):
                assert torch.equal(got[k], again[k]), (k, name)
            for q in range(n_src):
                assert torch.equal(got['dsrcs'][q], again['dsrcs'][q])


def test_ignored_rows_get_exactly_zero_dlogits():
    """dbias = sum over rows of dlogits: with every row but one ignored it IS that row's dlogits."""
    C, L, n_src, O, b = 16, 4, 2, 17, 17
    g = _gen(8100)
    t = _head_inputs(g, C, L, n_src, O, b, False)
    w = _vec(g, O, True)
    y = torch.full((b,), 5, dtype=torch.int64)
    y[7] = 16                                                     # the one class of the second stripe
    kw = dict(weight=w, pos_weight=None, label_smoothing=0.1, ignore_index=5, reduction='mean')
    _, dl = crit_ref.ce(t.fw['logits'], y, w, 0.1, 5, 'mean')
    got = _launch(t, C, L, O, b, 'plain', 2, y, None, False, kw)
    assert_close_scaled('dbias', got['dbias'], dl[7])
    assert float(dl.abs().sum() - dl[7].abs().sum()) == 0.0


def test_refusals():
    from bmnas import lib
    d = dev()
    C, L, b, O = 16, 4, 2, 5
    z = lambda *s: torch.zeros(*s, device=d)
    a, sums, w7, W, hb, st = z(b, C, L), z(b, 2), z(C, L), z(O, C * L), z(3, b, O), torch.ones(b, 2, device=d)
    y, lab, loss, part, w = z(b, O), torch.zeros(b, dtype=torch.int64, device=d), z(1), z(1, O + 3, C * L), torch.ones(O, device=d)
    lnp = z(b, 1, 2)
    lazy = lib.make_lazy(a, None, None, w7, w7, st)
    E_ARG, E_LIMIT = r'rc=-1\)', r'rc=-3\)'

    def plain(crit, mode, labels, O_=O, W_=W, hb_=hb):
        lib.head_bwd([a], [sums], [z(b, C, L)], 0, w7, w7, W_, hb_, st, mode, None, None, labels, loss, part, b, C, L,
                     O_, crit=crit)

    def lazyf(crit, mode, labels):
        lib.head_bwd_lazy([lazy], [lnp], [z(b, C, L)], 0, w7, w7, W, hb, st, mode, None, None, labels, loss, part, b, C,
                          L, O, crit=crit)

    bad = [(lib.Criterion('ce', label_smoothing=1.0), 2, lab), (lib.Criterion('ce', label_smoothing=-0.5), 2, lab),
           (lib.Criterion('ce', pos_weight=w), 2, lab), (lib.Criterion('bce', label_smoothing=0.1), 1, y)]
    for crit, mode, labels in bad:
        for call in (plain, lazyf):
            with pytest.raises(lib.BmnasError, match=E_ARG):
                call(crit, mode, labels)
    # the options are judged first: a bad descriptor with O = 129 is a bad argument, a good one is over the limit
    W9, hb9 = z(129, C * L), z(3, b, 129)
    with pytest.raises(lib.BmnasError, match=E_ARG):
        plain(lib.Criterion('ce', label_smoothing=1.0), 2, lab, 129, W9, hb9)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        plain(lib.Criterion('ce', label_smoothing=0.1), 2, lab, 129, W9, hb9)
    # ... in the lazy form too: C L = 4160 lies outside bmnas_lazy_ln_ok (a limit), C L = 80 is not tiled by the 64-k
    # groups (a shape); with a bad descriptor both are a bad argument first
    for C2, L2, rule in ((260, 16, E_LIMIT), (20, 4, r'rc=-2\)')):
        a2, w2, W2 = z(b, C2, L2), z(C2, L2), z(O, C2 * L2)
        lazy2, lnp2, part2 = lib.make_lazy(a2, None, None, w2, w2, st), z(b, C2 * L2 // 64 + 1, 2), z(1, O + 3, C2 * L2)

        def lazy_at(crit, mode, labels):
            lib.head_bwd_lazy([lazy2], [lnp2], [z(b, C2, L2)], 0, w2, w2, W2, hb, st, mode, None, None, labels, loss,
                              part2, b, C2, L2, O, crit=crit)
        for crit, mode, labels in bad:
            with pytest.raises(lib.BmnasError, match=E_ARG):
                lazy_at(crit, mode, labels)
        with pytest.raises(lib.BmnasError, match=rule):
            lazy_at(lib.Criterion('ce', label_smoothing=0.1), 2, lab)
    # kind 0 (a given dlogits) is the plain entry points' business
    so = lib.load()
    rc = so.bmnas_head_bwd_crit(lib._ptrs([a]), lib._ptrs([sums]), lib._ptrs([z(b, C, L)]), 1, 0, w7.data_ptr(),
                                w7.data_ptr(), W.data_ptr(), hb.data_ptr(), st.data_ptr(), 0, None, lab.data_ptr(),
                                loss.data_ptr(), part.data_ptr(), b, C, L, O, None, 0, lib.Criterion('ce').desc(), None)
    assert rc == -1
    plain(lib.Criterion('ce', weight=w, label_smoothing=0.1, ignore_index=0, reduction='sum'), 2, lab)
    lazyf(lib.Criterion('bce', weight=w, pos_weight=w), 1, y)
    torch.cuda.synchronize()
