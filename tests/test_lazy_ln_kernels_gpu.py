"""The streaming-LayerNorm kernel family (csrc/lazyln.hip, the lazy forms of csrc/head.hip), entry point by entry
point, against the float64 statement in tests/lazy_ln_ref.py (pinned by tests/test_lazy_ln_ref.py on the CPU) and
against the per-sample kernels they replaced, which tests/test_kernels_gpu.py and the oracle tests pin.

Bounds: 1e-4 of the expected tensor's scale against float64 (assert_close_scaled), rel = 2e-5 kernel against kernel on
identical inputs.  Offset inputs (lazy_ln_ref.offset_resid): max(1e-4, 3 x the error of the per-sample kernel against
the same float64 reference), both errors measured and printed (the rule of tests/test_numerics_gpu.py).
Every output buffer starts as NaN unless the ABI wants it zero-filled (hb, bn_grad, dgamma, dw): an element that a
kernel never writes fails its comparison.  The head's ReLU is the only discontinuity a float64 comparison crosses: the
K7 bias is redrawn on the CPU until no ReLU argument lies within 1e-3 of zero, and no element is left out anywhere.

(C, L) at the part and tile edges — C L / 4 = 16: a quarter wave of one part, 48 idle columns in node_mix_lnp_bwd;
256: exactly one part; 272: two parts, the second with 16 float4; 768: three parts, the workload's; 1024: the limit."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import lazy_ln_ref as lr
from gpu_util import assert_close_scaled, dev

pytestmark = pytest.mark.gpu

SHAPES = [(16, 4), (128, 8), (68, 16), (192, 16), (256, 16)]
KK = 2e-5                                          # kernel against kernel, same math, same inputs
E_ARG, E_SHAPE, E_LIMIT = r'rc=-1\)', r'rc=-2\)', r'rc=-3\)'


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


def _nan(*shape):
    return torch.full(shape, float('nan'), device=dev())


def _err(got, want):
    """largest deviation in units of the expected tensor's scale (NaN if anything was left unwritten)"""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((got - want).abs().max() / max(float(want.abs().max()), 1e-30))


def _offset_rule(name, streaming, pinned, want):
    e_s, e_p = _err(streaming, want), _err(pinned, want)
    bound = max(1e-4, 3.0 * e_p)
    print(f'offset {name}: streaming {e_s:.2e}, per-sample kernel {e_p:.2e}, bound {bound:.2e}')
    assert np.isfinite(e_s) and e_s <= bound, (name, e_s, e_p, bound)


def _cmp(name, got, want64, pinned=None, offset=False):
    """against float64 at the project's bound — under the offset rule where a pinned kernel computed the same —
    and against that kernel at 2e-5"""
    if offset and pinned is not None:
        _offset_rule(name, got, pinned, want64)                  # (offset inputs: this rule IS the bound)
        return
    assert_close_scaled(name, got, want64)
    if pinned is not None:
        assert_close_scaled(name + ' (kernel vs kernel)', got, pinned.cpu(), rel=KK)


def _cmp_cols(name, cols, got, want64, pinned=None, offset=False):
    """(b, 2) pairs of unlike scale (mean | rstd, sum | sum of squares): each column on its own"""
    for c, nm in enumerate(cols):
        _cmp(f'{name} {nm}', got[:, c], want64[:, c], None if pinned is None else pinned[:, c], offset)


def _mix_inputs(g, b, C, L, same=True, offset=False, drop=False):
    d = dev()
    x, p1, U = _rand(g, b, C, L).to(d), _rand(g, b, C, L).to(d), _rand(g, b, 3 * C, L).to(d)
    y = x if same else _rand(g, b, C, L).to(d)
    resid = (lr.offset_resid(g, b, C, L) if offset else _rand(g, b, C, L)).to(d)
    ln_w, ln_b = (_rand(g, C, L) * 0.3 + 1.0).to(d), (_rand(g, C, L) * 0.2).to(d)
    gamma = torch.softmax(_rand(g, 4), 0).to(d)
    M = 3 * C
    Ud = U.double()
    mean = Ud.mean(dim=(0, 2))
    rstd = 1.0 / torch.sqrt(Ud.var(dim=(0, 2), unbiased=False) + 1e-5)
    bn_w, bn_b = (_rand(g, M) * 0.3 + 1.0).to(d).double(), (_rand(g, M) * 0.2).to(d).double()
    scale = rstd * bn_w
    chan = torch.cat([mean, rstd, scale, bn_b - mean * scale]).float().contiguous()
    from bmnas import lib
    dglu = lib.make_dropout(0.1, 1234, 0) if drop else lib.NO_DROP
    dfc = lib.make_dropout(0.2, 1234, b * C * L // 4) if drop else lib.NO_DROP
    return SimpleNamespace(x=x, y=y, p1=p1, U=U, resid=resid, ln_w=ln_w, ln_b=ln_b, gamma=gamma, chan=chan, dglu=dglu,
                           dfc=dfc, b=b, C=C, L=L, same=same)


def _records32(pre, ln_w, ln_b):
    """The records a producer hands over, from float64: m_k rounded to fp32, the moments centred on THAT m_k."""
    rec0, _ = lr.records(pre, ln_w, ln_b)
    rec, prm = lr.records(pre, ln_w, ln_b, centre=rec0[:, :, 0].float().double())
    return rec.float().contiguous(), prm.float().contiguous()


def _pinned_fwd(m):
    """bmnas_node_mix_ln_fwd on the mix inputs: pre, out, stats, out_sums"""
    from bmnas import lib
    pre, out, stats, sums = _nan(m.b, m.C, m.L), _nan(m.b, m.C, m.L), _nan(m.b, 2), _nan(m.b, 2)
    lib.node_mix_ln_fwd(m.x, m.y, m.p1, m.U, m.chan.clone(), m.gamma, m.resid, m.ln_w, m.ln_b, pre, out, stats, m.b,
                        m.C, m.L, m.dglu, m.dfc, out_sums=sums)
    torch.cuda.synchronize()
    return pre, out, stats, sums


def _softmax_cols(g, rows):
    """(rows, 2) softmaxed weight rows; the kernels read column 1 (stride 2)"""
    w = torch.softmax(_rand(g, rows, 2), dim=1).to(dev()).contiguous()
    return w, w.reshape(-1)[1:]


# ------------------------------------------------------------------------------------------------ a. the producer
@pytest.mark.parametrize('variant', ['plain', 'drop', 'xy', 'drop_xy', 'offset'])
@pytest.mark.parametrize('b', [1, 5])
@pytest.mark.parametrize('C,L', SHAPES)
def test_node_mix_pre_fwd(C, L, b, variant):
    from bmnas import lib
    assert (C * L) % 64 == 0 and lib.lazy_ln_ok(C, L)
    offset = variant == 'offset'
    m = _mix_inputs(_gen(1000 + C + L + b), b, C, L, same='xy' not in variant, offset=offset, drop='drop' in variant)
    P = lib.lazy_ln_parts(C, L)
    assert P == lr.n_parts(C * L)
    pre, rec, prm = _nan(b, C, L), _nan(b, P, 8), _nan(P, 8)
    lib.node_mix_pre_fwd(m.x, m.y, m.p1, m.U, m.chan.clone(), m.gamma, m.resid, m.ln_w, m.ln_b, pre, rec, prm, b, C, L,
                         m.dglu, m.dfc)
    torch.cuda.synchronize()
    pre_p, out_p, stats_p, sums_p = _pinned_fwd(m)
    assert torch.equal(pre, pre_p)                               # the same compiled expression: bit-equal
    pre64, w64, b64 = pre.cpu().double(), m.ln_w.cpu().double(), m.ln_b.cpu().double()
    rec_c, prm_c = rec.cpu(), prm.cpu()
    assert torch.isfinite(rec_c).all() and torch.isfinite(prm_c).all()
    assert float(rec_c[:, :, 6:].abs().max()) == 0.0 and float(prm_c[:, 6:].abs().max()) == 0.0
    want_rec, want_prm = lr.records(pre64, w64, b64)
    names = ['m_k', 'S(c^2)', 'S(c w)', 'S(c^2 w^2)', 'S(c w b)', 'S(c w^2)']
    if offset:
        # the part means are ~50 +- 20: m_k carries an fp32 rounding of ~4e-6, and the moments are centred on the STORED
        # m_k (which is what makes the combination exact) — so they are compared with the float64 moments about it.
        # That takes a kernel output into the reference for these five fields, and m_k itself is only held to 1e-4
        # of ~50 here; a wrong m_k is still caught below: combine(rec) must give the sample's mean, rstd, S(o) and
        # S(o^2) under the offset rule, and a part mean that is off by e moves the combined mean by e n_k / N.
        assert_close_scaled('rec m_k', rec_c[:, :, 0], want_rec[:, :, 0])
        want_rec, _ = lr.records(pre64, w64, b64, centre=rec_c[:, :, 0].double())
    for f, nm in enumerate(names):
        assert_close_scaled('rec ' + nm, rec_c[:, :, f], want_rec[:, :, f])
    for f, nm in enumerate(['S(w^2)', 'S(w)', 'S(w b)', 'S(b)', 'S(b^2)', 'n_k']):
        assert_close_scaled('prm ' + nm, prm_c[:, f], want_prm[:, f])
    assert torch.equal(prm_c[:, 5].double(), want_prm[:, 5])
    # what a consumer makes of them, against the direct moments (and, offset, against the per-sample kernel's error)
    mean, rstd, osum, osq = lr.combine(rec_c, prm_c)
    n64, mean64, rstd64, _ = lr.node_ln(pre64, w64, b64)
    s64 = lr.out_sums(n64)
    stats_p, sums_p = stats_p.cpu(), sums_p.cpu()
    for nm, got, pin, want in [('mean', mean, stats_p[:, 0], mean64), ('rstd', rstd, stats_p[:, 1], rstd64),
                               ('S(o)', osum, sums_p[:, 0], s64[:, 0]), ('S(o^2)', osq, sums_p[:, 1], s64[:, 1])]:
        if offset:
            _offset_rule('combine(rec) ' + nm, got, pin, want)
        else:
            assert_close_scaled('combine(rec) ' + nm, got, want)


# -------------------------------------------------------------------------------------- b. the first consumer (K1 pair)
@pytest.mark.parametrize('variant', ['sums', 'nosums', 'offset'])
@pytest.mark.parametrize('n_in', [1, 3, 8])
@pytest.mark.parametrize('C,L', SHAPES)
def test_mixsum_pair_fwd_lazy(C, L, n_in, variant):
    from bmnas import lib
    offset = variant == 'offset'
    b = 1 if (n_in == 3 and variant == 'sums') else 5
    g = _gen(2000 + C + L + n_in)
    m = _mix_inputs(g, b, C, L, offset=offset)
    d = dev()
    pre, out_p, stats_p, sums_p = _pinned_fwd(m)
    pre64, w64, b64 = pre.cpu().double(), m.ln_w.cpu().double(), m.ln_b.cpu().double()
    rec, prm = _records32(pre64, w64, b64)
    xs = [_rand(g, b, C, L).to(d) for _ in range(n_in)]
    w_full, w = _softmax_cols(g, n_in + 1)
    w2_full, w2 = _softmax_cols(g, 2)
    stats, nout, out, out2 = _nan(b, 2), _nan(b, C, L), _nan(b, C, L), _nan(b, C, L)
    sums = _nan(b, 2) if variant != 'nosums' else None
    rec, prm = rec.to(d), prm.to(d)
    lazy = lib.make_lazy(pre, rec, prm, m.ln_w, m.ln_b, stats)
    lib.mixsum_pair_fwd_lazy(xs, w, 2, w2, 2, lazy, nout, sums, out, out2, b, C, L)
    torch.cuda.synchronize()
    n64, mean64, rstd64, _ = lr.node_ln(pre64, w64, b64)
    wc = w_full[:, 1].cpu().double()
    h64 = sum(wc[j] * xs[j].cpu().double() for j in range(n_in)) + wc[n_in] * n64
    s2 = float(w2_full[0, 1].cpu().double() + w2_full[1, 1].cpu().double())
    _cmp('last_out', nout, n64, out_p, offset)
    _cmp_cols('stats', ('mean', 'rstd'), stats, torch.stack([mean64, rstd64], 1), stats_p, offset)
    if sums is not None:
        _cmp_cols('last_sums', ('S(o)', 'S(o^2)'), sums, lr.out_sums(n64), sums_p, offset)
    assert_close_scaled('out', out, h64)
    assert_close_scaled('out2', out2, s2 * h64)


# ------------------------------------------------------------------------------------------------ c. the K1 backward
_BWD_VARIANTS = {            # gh, gz2, dots, g_full, extra stride, accumulate: 'all' | 'lazy' | 'alt' | 'none'
    'v0': (True, True, True, False, 0, 'all'),
    'v1': (False, False, False, True, 3, 'lazy'),
    'v2': (True, False, True, True, 3, 'alt'),
    'v3': (False, True, False, False, 0, 'none'),
}


@pytest.mark.parametrize('variant', sorted(_BWD_VARIANTS))
@pytest.mark.parametrize('n_in,n_lazy', [(2, 1), (3, 2), (8, 2)])
@pytest.mark.parametrize('C,L', SHAPES)
def test_mixsum_pair_bwd_lazy(C, L, n_in, n_lazy, variant):
    from bmnas import lib
    have_gh, have_gz2, dots, full, extra, accs = _BWD_VARIANTS[variant]
    b, d = 5, dev()
    g = _gen(3000 + C + L + 10 * n_in + n_lazy)
    P = lib.lazy_ln_parts(C, L)
    first = n_in - n_lazy
    lazy_bits = sum(1 << j for j in range(first, n_in))
    acc = {'all': (1 << n_in) - 1, 'lazy': lazy_bits, 'alt': (0x5555 & ((1 << n_in) - 1)) | (1 << (n_in - 1)),
           'none': 0}[accs]
    # the lazy inputs: pre, affine, fp32 statistics; xs holds their normalised values
    pres, lnws, stats, xhats, xs = [], [], [], [], [_rand(g, b, C, L).to(d) for _ in range(first)]
    for t in range(n_lazy):
        pre = (_rand(g, b, C, L) * 1.5 + 0.2)
        lw, lb = _rand(g, C, L) * 0.3 + 1.0, _rand(g, C, L) * 0.2
        n64, mean, rstd, _ = lr.node_ln(pre, lw, lb)
        st = torch.stack([mean, rstd], 1).float().contiguous()
        xhats.append((pre.double() - st[:, 0].double()[:, None, None]) * st[:, 1].double()[:, None, None])
        pres.append(pre.to(d)); lnws.append(lw.to(d)); stats.append(st.to(d)); xs.append(n64.float().to(d))
    w_full, w = _softmax_cols(g, n_in)
    w2_full, w2 = _softmax_cols(g, 2)
    h, gz = _rand(g, b, C, L).to(d), _rand(g, b, C, L).to(d)
    gh = _rand(g, b, C, L).to(d) if have_gh else None
    gz2 = _rand(g, b, C, L).to(d) if have_gz2 else None
    old = [_rand(g, b, C, L).to(d) for _ in range(n_in)]
    skip0 = full                                                 # with g_full the first input's gradient is not wanted
    stride = P + extra
    SENT = -777.25

    def run(lazy_form):
        dxs = [o.clone() if (acc >> j) & 1 else _nan(b, C, L) for j, o in enumerate(old)]
        if skip0:
            dxs[0] = None
        dw_full = torch.zeros(n_in, 2, device=d) if dots else None
        dw2_full = torch.zeros(2, 2, device=d) if dots else None
        dw = dw_full.reshape(-1)[1:] if dots else None
        dw2 = dw2_full.reshape(-1)[1:] if dots else None
        res = dict(dxs=dxs, dw=dw_full, dw2=dw2_full)
        if not lazy_form:
            lib.mixsum_pair_bwd(xs, dxs, w, 2, w2, 2, h, gh, gz, dw, dw2, acc, gz2=gz2)
        else:
            # a shared buffer per lazy input, this consumer's view starting at pair 2
            bufs = [torch.full((b * stride + 4, 2), SENT, device=d) for _ in range(n_lazy)]
            gfull = _nan(b, C, L) if full else None
            lz = [lib.make_lazy(pres[t], None, None, lnws[t], None, stats[t]) for t in range(n_lazy)]
            lib.mixsum_pair_bwd_lazy(xs, dxs, w, 2, w2, 2, h, gh, gz, dw, dw2, acc, lz,
                                     [bf.reshape(-1)[4:] for bf in bufs], [stride] * n_lazy, b, C, L, gz2=gz2,
                                     g_full=gfull)
            res.update(bufs=bufs, g_full=gfull)
        torch.cuda.synchronize()
        return res

    got, pin = run(True), run(False)
    wc = w_full[:, 1].cpu().double()
    s2 = float(w2_full[0, 1].cpu().double() + w2_full[1, 1].cpu().double())
    Z = gz.cpu().double() + (gz2.cpu().double() if have_gz2 else 0.0)
    G = s2 * Z + (gh.cpu().double() if have_gh else 0.0)
    for j in range(n_in):
        if got['dxs'][j] is None:
            continue
        want = wc[j] * G + (old[j].cpu().double() if (acc >> j) & 1 else 0.0)
        _cmp(f'dxs[{j}]', got['dxs'][j], want, pin['dxs'][j])
    if dots:
        want_dw = torch.zeros(n_in, 2, dtype=torch.float64)
        want_dw[:, 1] = torch.stack([(G * xs[j].cpu().double()).sum() for j in range(n_in)])
        want_dw2 = torch.zeros(2, 2, dtype=torch.float64)
        want_dw2[:, 1] = (Z * h.cpu().double()).sum()
        _cmp('dw', got['dw'], want_dw, pin['dw'])
        _cmp('dw2', got['dw2'], want_dw2, pin['dw2'])
        assert float(got['dw'][:, 0].abs().max()) == 0.0 and float(got['dw2'][:, 0].abs().max()) == 0.0
    if full:
        assert_close_scaled('g_full', got['g_full'], G)
    for t in range(n_lazy):
        want = lr.ln_partials(wc[first + t] * G, lnws[t].cpu(), xhats[t], lr.PART)
        assert want.shape == (b, P, 2)
        buf = got['bufs'][t].cpu()
        idx = (2 + torch.arange(b)[:, None] * stride + torch.arange(P)[None, :]).reshape(-1)
        assert_close_scaled(f'lnpart[{t}] S(gy w)', buf[idx, 0].reshape(b, P), want[:, :, 0])
        assert_close_scaled(f'lnpart[{t}] S(gy w xhat)', buf[idx, 1].reshape(b, P), want[:, :, 1])
        keep = torch.ones(buf.shape[0], dtype=torch.bool)
        keep[idx] = False
        assert bool((buf[keep] == SENT).all()), 'a pair outside this consumer\'s P slots was written'
        assert int(keep.sum()) == 4 + b * extra


def test_mixsum_pair_bwd_lazy_refuses_aliased_lazy_destinations():
    from bmnas import lib
    b, C, L, d = 2, 16, 4, dev()
    t = [torch.zeros(b, C, L, device=d) for _ in range(8)]
    st = torch.ones(b, 2, device=d)
    w = torch.full((6,), 0.5, device=d)
    lz = [lib.make_lazy(t[0], None, None, t[1][0], None, st) for _ in range(2)]
    lnp = [torch.zeros(b, 1, 2, device=d) for _ in range(2)]
    shared = torch.zeros(b, C, L, device=d)
    for dxs in ([t[5], shared, shared], [shared, t[5], shared], [shared, shared, t[5]]):
        with pytest.raises(lib.BmnasError, match=E_ARG):
            lib.mixsum_pair_bwd_lazy(t[2:5], dxs, w, 2, w, 2, t[6], None, t[7], None, None, 0, lz, lnp, [1, 1], b, C, L)
    # (two plain destinations may alias: in-order read-modify-write)
    lib.mixsum_pair_bwd_lazy([t[2], t[3], t[4]], [shared, shared, t[5]], w, 2, w, 2, t[6], None, t[7], None, None, 0,
                             lz[:1], lnp[:1], [1], b, C, L)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------ d. LayerNorm + mix backward, streaming
def _split_partials(g, total, n):
    """n pieces (b, n, 2) that sum to total (b, 2): random shares plus zero-sum noise"""
    b = total.shape[0]
    sh = torch.rand(n, generator=g).double() + 0.1
    sh = sh / sh.sum()
    noise = torch.randn(b, n, 2, generator=g).double()
    noise = noise - noise.mean(dim=1, keepdim=True)
    return total[:, None, :] * sh[None, :, None] + noise


_LNP_CASES = [
    # C, L, b, split, racc, xacc, nulls, shards, drop, same, offset, det
    (16, 4, 1, 'P', 0, 0, '', 1, False, True, False, False),
    (16, 4, 5, '0+3', 1, 1, '', 4, True, False, False, False),
    (16, 4, 37, '17+65', 0, 1, 'g_in', 1, True, True, False, False),
    (16, 4, 130, 'P', 1, 0, '', 4, False, False, False, False),
    (16, 4, 257, '17+65', 0, 1, '', 1, True, True, False, False),
    (16, 4, 257, '0+3', 1, 0, '', 4, False, False, False, True),
    (128, 8, 1, '0+3', 1, 1, 'dresid', 1, True, True, False, False),
    (128, 8, 5, '17+65', 0, 0, 'dxdy', 4, False, False, False, False),
    (128, 8, 37, 'P', 1, 1, '', 1, True, False, False, True),
    (68, 16, 1, '17+65', 0, 0, '', 4, False, True, False, False),
    (68, 16, 5, 'P', 1, 1, 'g_in', 1, True, False, False, True),
    (68, 16, 37, '0+3', 0, 1, '', 4, True, True, False, False),
    (192, 16, 1, 'P', 1, 0, '', 1, True, False, False, False),
    (192, 16, 5, '0+3', 0, 1, '', 4, False, True, False, True),
    (192, 16, 37, '17+65', 1, 1, 'dresid', 1, True, False, False, False),
    (256, 16, 1, '17+65', 0, 1, '', 4, True, True, False, False),
    (256, 16, 5, 'P', 1, 0, '', 1, False, False, False, False),
    (256, 16, 37, '0+3', 0, 0, '', 4, True, True, False, True),
    (16, 4, 5, 'P', 0, 0, '', 1, False, True, True, False),
    (128, 8, 5, '17+65', 1, 1, '', 1, False, True, True, False),
    (68, 16, 5, 'P', 0, 1, '', 4, True, False, True, False),
    (192, 16, 5, '17+65', 1, 0, '', 1, True, True, True, False),
    (256, 16, 5, 'P', 0, 0, '', 1, False, False, True, False),
]


@pytest.mark.parametrize('C,L,b,split,racc,xacc,nulls,shards,drop,same,offset,det', _LNP_CASES)
def test_node_mix_lnp_bwd(C, L, b, split, racc, xacc, nulls, shards, drop, same, offset, det):
    from bmnas import lib
    d = dev()
    g = _gen(4000 + C + L + b + len(split))
    m = _mix_inputs(g, b, C, L, same=same, drop=drop)
    P, M, N = lib.lazy_ln_parts(C, L), 3 * C, C * L
    pre_c = lr.offset_resid(g, b, C, L) if offset else _rand(g, b, C, L) * 1.5 + 0.2
    gy_c = _rand(g, b, C, L)
    mean, rstd = lr.moments(pre_c)
    stats_c = torch.stack([mean, rstd], 1).float().contiguous()
    xhat = (pre_c.double() - stats_c[:, 0].double()[:, None, None]) * stats_c[:, 1].double()[:, None, None]
    parts = lr.ln_partials(gy_c, m.ln_w.cpu(), xhat, lr.PART)
    total = parts.sum(1)
    if split == 'P':
        lnp0, lnp1 = parts.float().contiguous().to(d), None
        assert lnp0.shape == (b, P, 2)
    elif split == '0+3':
        lnp0, lnp1 = None, _split_partials(g, total, 3).float().contiguous().to(d)
    else:                                                        # 82 pairs: the column-strided loop wraps
        pieces = _split_partials(g, total, 82).float()
        lnp0, lnp1 = pieces[:, :17].contiguous().to(d), pieces[:, 17:].contiguous().to(d)
    pre, gy, stats = pre_c.to(d), gy_c.to(d), stats_c.to(d)
    old_r, old_x, old_y = _rand(g, b, C, L).to(d), _rand(g, b, C, L).to(d), _rand(g, b, C, L).to(d)
    acc = xacc | (0 if same else (xacc << 1))
    use_ln_bwd = b <= 128
    assert lib.node_mix_ln_bwd_ok(b, C, L) == use_ln_bwd
    rows = lib.node_mix_lnp_bwd_rows(b)
    assert rows == (b + (8 if b > 256 else 4) - 1) // (8 if b > 256 else 4)

    def run(kind):
        dres = None if nulls == 'dresid' else (old_r.clone() if racc else _nan(b, C, L))
        ra = 0 if dres is None else racc
        if nulls == 'dxdy':
            dx = dy = None
        else:
            dx = old_x.clone() if xacc else _nan(b, C, L)
            dy = None if same else (old_y.clone() if xacc else _nan(b, C, L))
        gin = None if (nulls == 'g_in' and kind != 'sep') else _nan(b, C, L)
        dgam = torch.zeros(shards, 4, device=d)
        dV, bn_grad = _nan(b, M, L), torch.zeros(2 * M, device=d)
        out = dict(dV=dV, bn_grad=bn_grad)
        if kind in ('lnp', 'det'):
            bn_part = _nan(rows, 6 * C) if kind == 'det' else None
            lib.node_mix_lnp_bwd(gy, pre, m.ln_w, stats, lnp0, lnp1, gin, dres, ra, m.x, m.y, m.p1, m.U, m.chan, m.gamma,
                                 dgam, dx, dy, acc, dV, bn_grad, b, C, L, m.dglu, m.dfc, dg_shards=shards, dg_stride=4,
                                 bn_part=bn_part)
            if kind == 'det':
                out['bn_part'] = bn_part
        elif use_ln_bwd:
            lib.node_mix_ln_bwd(gy, pre, m.ln_w, stats, gin, dres, ra, m.x, m.y, m.p1, m.U, m.chan, m.gamma, dgam, dx,
                                dy, acc, dV, bn_grad, b, C, L, m.dglu, m.dfc, dg_shards=shards, dg_stride=4)
        else:                                                    # as test_node_mix_ln_bwd_matches_separate_launches
            lib.cat_ln_bwd(gy, [pre], None, m.ln_w, m.ln_b, stats, [gin], dres, ra << 31, None, None, b, C, L, False)
            lib.node_mix_bwd(gin, m.x, m.y, m.p1, m.U, m.chan, m.gamma, dgam, dx, dy, acc, dV, bn_grad, b, C, L, m.dglu,
                             m.dfc, dg_shards=shards, dg_stride=4)
        torch.cuda.synchronize()
        out['dgamma'] = dgam.sum(0)
        for k, v in (('g_in', gin), ('dresid', dres), ('dx', dx), ('dy', dy)):
            if v is not None:
                out[k] = v
        return out

    got = run('lnp')
    pin = run('pin' if use_ln_bwd else 'sep')
    want_gin = lr.node_ln_bwd(gy_c, m.ln_w.cpu(), xhat, stats_c[:, 1], total)
    if 'g_in' in got:
        _cmp('g_in', got['g_in'], want_gin, pin['g_in'], offset)
    if 'dresid' in got:
        _cmp('dresid', got['dresid'], want_gin + (old_r.cpu().double() if racc else 0.0), pin['dresid'], offset)
    for k in ('dx', 'dy', 'dV', 'bn_grad', 'dgamma'):
        if k in got:
            assert_close_scaled(k + ' (kernel vs kernel)', got[k], pin[k].cpu(), rel=KK)
    if 'dx' in got:                                              # and the Sum term's share in float64
        g0 = float(m.gamma[0].cpu().double())
        assert_close_scaled('dx', got['dx'], (2.0 if same else 1.0) * g0 * want_gin +
                            (old_x.cpu().double() if xacc else 0.0))
    if drop:
        assert float((got['dV'] == 0).float().mean()) > 0.05
    if det:
        d1, d2 = run('det'), run('det')
        for k in got:
            assert_close_scaled(k + ' (bn_part form vs atomic form)', d1[k], got[k].cpu(), rel=KK)
        for k in ('bn_part', 'bn_grad', 'dV'):
            assert torch.equal(d1[k], d2[k]), k


# ------------------------------------------------------------------------------------------------ e. the head consumers
def _head_inputs(g, C, L, n_src, O, b, offset):
    """CPU fp32 inputs with a K7 bias that keeps every ReLU argument clear of zero, and their float64 head."""
    t = SimpleNamespace(pre=[], nw=[], nb=[], n64=[], nstats=[], xhat=[])
    for q in range(n_src):
        pre = lr.offset_resid(g, b, C, L) if offset else _rand(g, b, C, L) * 1.5 + 0.2 * q
        nw, nb = _rand(g, C, L) * 0.3 + 1.0, _rand(g, C, L) * 0.2
        n64, mean, rstd, _ = lr.node_ln(pre, nw, nb)
        st = torch.stack([mean, rstd], 1).float().contiguous()
        t.pre.append(pre); t.nw.append(nw); t.nb.append(nb); t.n64.append(n64); t.nstats.append(st)
        t.xhat.append((pre.double() - st[:, 0].double()[:, None, None]) * st[:, 1].double()[:, None, None])
    D = n_src * C * L
    t.ln_w = _rand(g, n_src * C, L) * 0.3 + 1.0
    t.ln_b = lr.clear_relu_bias(g, t.n64, t.ln_w, _rand(g, n_src * C, L) * 0.2)
    t.W, t.bias = _rand(g, O, D) / D ** 0.5, _rand(g, O) * 0.1
    t.fw = lr.head_fwd(t.n64, t.ln_w, t.ln_b, t.W, t.bias)
    lr.assert_relu_clear(t.fw)
    t.n32 = [n.float().contiguous() for n in t.n64]
    t.sums = [lr.out_sums(n.double()).float().contiguous() for n in t.n32]
    return t


def _run_head_fwd(t, C, L, O, b, lazy_q, form):
    """form: 'pinned' (bmnas_head_fwd on the materialised sources), 'lazy' (atomics), 'det' (hb_part)"""
    from bmnas import lib
    d = dev()
    n_src = len(t.pre)
    to = lambda x: x.to(d)
    ln_w, ln_b, W, bias = to(t.ln_w), to(t.ln_b), to(t.W), to(t.bias)
    stats = _nan(b, 2)
    srcs, sums = [to(n) for n in t.n32], [to(s) for s in t.sums]
    res = dict(stats=stats)
    if form == 'pinned':
        hb = torch.zeros(3, b, O, device=d)
        lib.head_fwd(srcs, sums, ln_w, ln_b, W, bias, hb, stats, b, C, L, O)
    else:
        rec, prm = _records32(t.pre[lazy_q], t.nw[lazy_q], t.nb[lazy_q])
        nstats = _nan(b, 2)
        pre = to(t.pre[lazy_q])
        keep = (to(rec), to(prm), to(t.nw[lazy_q]), to(t.nb[lazy_q]))       # (the descriptor holds addresses only)
        lazy = lib.make_lazy(pre, keep[0], keep[1], keep[2], keep[3], nstats)
        srcs[lazy_q], sums[lazy_q] = pre, None
        if form == 'det':
            hb = _nan(3, b, O)                                   # (summed INTO by plain stores: no zero-fill needed)
            part = _nan(lib.head_fwd_part_floats(b, C, L, n_src, O))
            lib.head_fwd_lazy(srcs, sums, lazy_q, lazy, ln_w, ln_b, W, bias, hb, stats, b, C, L, O, hb_part=part)
        else:
            hb = torch.zeros(3, b, O, device=d)
            lib.head_fwd_lazy(srcs, sums, lazy_q, lazy, ln_w, ln_b, W, bias, hb, stats, b, C, L, O)
        res['nstats'] = nstats
    torch.cuda.synchronize()
    res['hb'] = hb
    return res


def _criterion(g, t, mode, O, b, gscale):
    """-> labels / g as the kernels take them (CPU), float64 loss and dlogits"""
    gs = 0.37 if gscale else 1.0
    if mode == 0:
        gl = _rand(g, b, O) / b
        return None, gl, 0.0, gl.double() * gs
    if mode == 1:
        y = (torch.rand(b, O, generator=g) < 0.3).float()
        loss, dl = lr.bce_logits(t.fw['logits'], y)
        return y, None, float(loss), dl * gs
    lab = torch.randint(0, O, (b,), generator=g)
    loss, dl = lr.cross_entropy(t.fw['logits'], lab)
    return lab, None, float(loss), dl * gs


LOSS0 = 0.75                                                     # *loss is added to, not overwritten


def _run_head_bwd(t, C, L, O, b, mode, labels, gl, gscale, acc, old, form):
    """form: 'pinned' (bmnas_head_bwd, materialised sources), 'lazy', 'det' (loss_part).  hb / stats: float64's."""
    from bmnas import lib
    d = dev()
    n_src = len(t.pre)
    D = n_src * C * L
    to = lambda x: None if x is None else x.to(d)
    ln_w, ln_b, W = to(t.ln_w), to(t.ln_b), to(t.W)
    hb = torch.stack([t.fw['logits'], t.fw['A'], t.fw['B']]).float().contiguous().to(d)
    stats = torch.stack([t.fw['mean'], t.fw['rstd']], 1).float().contiguous().to(d)
    dsrcs = [old[q].clone().to(d) if (acc >> q) & 1 else _nan(b, C, L) for q in range(n_src)]
    n_chunk = lib.head_chunks(b)
    assert n_chunk == (b + (32 if b >= 64 else 16) - 1) // (32 if b >= 64 else 16)
    part = _nan(n_chunk, O + 3, D)
    loss = torch.full((1,), LOSS0, device=d)
    gsc = torch.full((1,), 0.37, device=d) if gscale else None
    res = dict(dsrcs=dsrcs, loss=loss)
    if form == 'pinned':
        lib.head_bwd([to(n) for n in t.n32], [to(s) for s in t.sums], dsrcs, acc, ln_w, ln_b, W, hb, stats, mode,
                     to(gl), gsc, to(labels), loss, part, b, C, L, O)
    else:
        keep = [(to(t.pre[q]), to(t.nw[q]), to(t.nb[q]), to(t.nstats[q])) for q in range(n_src)]
        lz = [lib.make_lazy(p, None, None, w_, b_, s_) for p, w_, b_, s_ in keep]
        lnparts = [_nan(b, C * L // 64, 2) for _ in range(n_src)]
        loss_part = _nan(n_chunk) if form == 'det' else None
        lib.head_bwd_lazy(lz, lnparts, dsrcs, acc, ln_w, ln_b, W, hb, stats, mode, to(gl), gsc, to(labels), loss, part,
                          b, C, L, O, loss_part=loss_part)
        res.update(lnparts=lnparts, loss_part=loss_part)
    summed = _nan(O + 3, D)
    lib.sum_chunks(part, summed, n_chunk)
    torch.cuda.synchronize()
    res.update(dW=summed[:O], dln_w=summed[O], dln_b=summed[O + 1], dbias=summed[O + 2, :O], part=part)
    return res


_HEAD_CASES = [
    # C, L, n_src, lazy_q, O, b, mode, gscale, acc ('none' | 'all' | 'mix'), offset
    (16, 4, 1, 0, 5, 1, 0, False, 'none', False),
    (16, 4, 2, 0, 60, 17, 1, True, 'all', False),
    (16, 4, 3, 2, 83, 63, 2, False, 'none', False),
    (16, 4, 2, 0, 83, 5, 2, True, 'all', True),
    (128, 8, 2, 1, 128, 64, 0, True, 'all', False),
    (128, 8, 3, 0, 5, 65, 1, False, 'mix', False),
    (128, 8, 1, 0, 128, 1, 0, False, 'none', True),
    (68, 16, 1, 0, 60, 17, 2, True, 'all', False),
    (68, 16, 2, 1, 83, 65, 0, False, 'none', True),
    (68, 16, 3, 2, 5, 64, 1, True, 'mix', False),
    (192, 16, 2, 1, 23, 40, 1, False, 'all', False),             # the launcher's J = 2 form
    (192, 16, 2, 0, 23, 49, 2, True, 'none', False),             # J = 3
    (192, 16, 3, 2, 128, 17, 0, True, 'all', True),
    (256, 16, 1, 0, 5, 17, 1, True, 'none', False),
    (256, 16, 3, 2, 60, 1, 2, False, 'all', False),
    (256, 16, 2, 0, 83, 5, 1, False, 'all', True),
]


def _acc_mask(acc, n_src):
    return {'none': 0, 'all': (1 << n_src) - 1, 'mix': 0b101 & ((1 << n_src) - 1)}[acc]


@pytest.mark.parametrize('C,L,n_src,lazy_q,O,b,mode,gscale,acc,offset', _HEAD_CASES)
def test_head_fwd_lazy(C, L, n_src, lazy_q, O, b, mode, gscale, acc, offset):
    g = _gen(5000 + C + L + n_src + O + b)
    t = _head_inputs(g, C, L, n_src, O, b, offset)
    got, pin = _run_head_fwd(t, C, L, O, b, lazy_q, 'lazy'), _run_head_fwd(t, C, L, O, b, lazy_q, 'pinned')
    for v, nm in enumerate(['logits', 'A', 'B']):
        _cmp(nm, got['hb'][v], t.fw[nm], pin['hb'][v], offset)
    _cmp_cols('stats', ('mean', 'rstd'), got['stats'], torch.stack([t.fw['mean'], t.fw['rstd']], 1), pin['stats'],
              offset)
    mean, rstd = lr.moments(t.pre[lazy_q])
    _cmp_cols('lazy->stats', ('mean', 'rstd'), got['nstats'], torch.stack([mean, rstd], 1))


@pytest.mark.parametrize('C,L,n_src,lazy_q,O,b,mode,gscale,acc,offset', _HEAD_CASES)
def test_head_bwd_lazy(C, L, n_src, lazy_q, O, b, mode, gscale, acc, offset):
    g = _gen(5000 + C + L + n_src + O + b)
    t = _head_inputs(g, C, L, n_src, O, b, offset)
    labels, gl, loss64, dl = _criterion(g, t, mode, O, b, gscale)
    bw = lr.head_bwd(t.fw, t.ln_w, t.W, dl)
    mask = _acc_mask(acc, n_src)
    old = [_rand(g, b, C, L) for _ in range(n_src)]
    got = _run_head_bwd(t, C, L, O, b, mode, labels, gl, gscale, mask, old, 'lazy')
    pin = _run_head_bwd(t, C, L, O, b, mode, labels, gl, gscale, mask, old, 'pinned')
    for q in range(n_src):
        want = bw['dn'][q] + (old[q].double() if (mask >> q) & 1 else 0.0)
        _cmp(f'dsrcs[{q}]', got['dsrcs'][q], want, pin['dsrcs'][q], offset)
        lnp = lr.ln_partials(bw['dn'][q], t.nw[q], t.xhat[q], lr.GROUP)
        assert lnp.shape == (b, C * L // 64, 2)
        assert_close_scaled(f'lnpart[{q}] S(gy w)', got['lnparts'][q][:, :, 0], lnp[:, :, 0])
        assert_close_scaled(f'lnpart[{q}] S(gy w xhat)', got['lnparts'][q][:, :, 1], lnp[:, :, 1])
    for k in ('dW', 'dln_w', 'dln_b', 'dbias'):
        _cmp(k, got[k], bw[k], pin[k], offset)
    if mode == 0:
        assert float(got['loss']) == LOSS0
    else:
        assert_close_scaled('loss', got['loss'] - LOSS0, torch.tensor([loss64], dtype=torch.float64))
        assert_close_scaled('loss (kernel vs kernel)', got['loss'], pin['loss'].cpu(), rel=KK)


@pytest.mark.parametrize('C,L,n_src,lazy_q,O,b,mode', [(16, 4, 1, 0, 1, 1, 1), (128, 8, 2, 0, 5, 17, 1),
                                                         (68, 16, 3, 2, 60, 65, 2), (192, 16, 2, 1, 23, 40, 1)])
def test_head_lazy_deterministic_forms(C, L, n_src, lazy_q, O, b, mode):
    """hb_part / loss_part: the atomic forms' values at 2e-5, bit-identical between two calls; b = 1, O = 1 leaves
    three floats to sum — no float4 at all."""
    g = _gen(6000 + C + L + n_src + O + b)
    t = _head_inputs(g, C, L, n_src, O, b, False)
    atom = _run_head_fwd(t, C, L, O, b, lazy_q, 'lazy')
    d1, d2 = _run_head_fwd(t, C, L, O, b, lazy_q, 'det'), _run_head_fwd(t, C, L, O, b, lazy_q, 'det')
    for v, nm in enumerate(['logits', 'A', 'B']):
        assert_close_scaled(nm, d1['hb'][v], t.fw[nm])
        assert_close_scaled(nm + ' (hb_part form vs atomic form)', d1['hb'][v], atom['hb'][v].cpu(), rel=KK)
    for k in ('hb', 'stats', 'nstats'):
        assert torch.equal(d1[k], d2[k]), k
    labels, gl, loss64, dl = _criterion(g, t, mode, O, b, False)
    old = [_rand(g, b, C, L) for _ in range(n_src)]
    atom = _run_head_bwd(t, C, L, O, b, mode, labels, gl, False, 0, old, 'lazy')
    d1 = _run_head_bwd(t, C, L, O, b, mode, labels, gl, False, 0, old, 'det')
    d2 = _run_head_bwd(t, C, L, O, b, mode, labels, gl, False, 0, old, 'det')
    from bmnas import lib
    assert d1['loss_part'].shape == (lib.head_chunks(b),)
    assert_close_scaled('loss_part', d1['loss_part'].sum().reshape(1), torch.tensor([loss64], dtype=torch.float64))
    assert_close_scaled('loss_part vs atomic', d1['loss_part'].sum().reshape(1), (atom['loss'] - LOSS0).cpu(), rel=KK)
    assert float(d1['loss']) == LOSS0                            # the caller sums the partials: *loss stays
    assert torch.equal(d1['loss_part'], d2['loss_part'])
    for q in range(n_src):
        assert_close_scaled(f'dsrcs[{q}]', d1['dsrcs'][q], atom['dsrcs'][q].cpu(), rel=KK)
        assert torch.equal(d1['dsrcs'][q], d2['dsrcs'][q]) and torch.equal(d1['lnparts'][q], d2['lnparts'][q])
    for k in ('dW', 'dln_w', 'dln_b', 'dbias'):
        assert torch.equal(d1[k], d2[k]), k


# ------------------------------------------------------------------------------------------------------ f. one chain
@pytest.mark.parametrize('C,L,b', [(192, 16, 37), (68, 16, 5)])
def test_chain_producer_to_consumers_and_back(C, L, b):
    """pre_fwd -> mixsum_pair_fwd_lazy (node 0) and head_fwd_lazy (node 1) -> head_bwd_lazy -> mixsum_pair_bwd_lazy ->
    node_mix_lnp_bwd, the real lnpart buffers handed from producer to consumer (per part, per 64-k group, and the
    shared stride of a K1 buffer), against float64 autograd of the same graph from `pre` on."""
    from bmnas import lib
    d = dev()
    g = _gen(7000 + C + b)
    P, O, CL = lib.lazy_ln_parts(C, L), 23, C * L
    nodes = [_mix_inputs(g, b, C, L, same=(k == 0), drop=(k == 1)) for k in range(2)]
    pres, lazies, nstats = [], [], []
    for m in nodes:
        pre, rec, prm, st = _nan(b, C, L), _nan(b, P, 8), _nan(P, 8), _nan(b, 2)
        lib.node_mix_pre_fwd(m.x, m.y, m.p1, m.U, m.chan.clone(), m.gamma, m.resid, m.ln_w, m.ln_b, pre, rec, prm, b, C,
                             L, m.dglu, m.dfc)
        pres.append(pre); nstats.append(st)
        lazies.append(lib.make_lazy(pre, rec, prm, m.ln_w, m.ln_b, st))
        m.keep = (rec, prm)
    torch.cuda.synchronize()
    # the rest of the inputs, on the CPU: the K7 bias kept clear of the ReLU for THESE node outputs
    pre64 = [p.cpu().double() for p in pres]
    n64 = [lr.node_ln(pre64[k], nodes[k].ln_w.cpu(), nodes[k].ln_b.cpu())[0] for k in range(2)]
    ln_w7 = _rand(g, 2 * C, L) * 0.3 + 1.0
    ln_b7 = lr.clear_relu_bias(g, n64, ln_w7, _rand(g, 2 * C, L) * 0.2)
    W, bias = _rand(g, O, 2 * CL) / (2 * CL) ** 0.5, _rand(g, O) * 0.1
    lr.assert_relu_clear(lr.head_fwd(n64, ln_w7, ln_b7, W, bias))
    y = (torch.rand(b, O, generator=g) < 0.3).float()
    xa, xb, gz = _rand(g, b, C, L), _rand(g, b, C, L), _rand(g, b, C, L) / (40 * b * O)
    w_full, w = _softmax_cols(g, 3)
    w2_full, w2 = _softmax_cols(g, 2)
    to = lambda x: x.to(d)
    xa_d, xb_d, gz_d, ln_w7d, ln_b7d, W_d, bias_d, y_d = map(to, (xa, xb, gz, ln_w7, ln_b7, W, bias, y))
    # forward consumers
    n0, sums0, h, z = _nan(b, C, L), _nan(b, 2), _nan(b, C, L), _nan(b, C, L)
    lib.mixsum_pair_fwd_lazy([xa_d, xb_d], w, 2, w2, 2, lazies[0], n0, sums0, h, z, b, C, L)
    hb, stats7 = torch.zeros(3, b, O, device=d), _nan(b, 2)
    lib.head_fwd_lazy([n0, pres[1]], [sums0, None], 1, lazies[1], ln_w7d, ln_b7d, W_d, bias_d, hb, stats7, b, C, L, O)
    # backward: the head, then node 0's K1 consumer (its view starts at pair P of a (b, 2 P, 2) buffer whose first P
    # pairs belong to another consumer, here one that contributed nothing), then the two nodes
    lnh = [_nan(b, CL // 64, 2) for _ in range(2)]
    dn = [_nan(b, C, L) for _ in range(2)]
    loss = torch.zeros(1, device=d)
    part = _nan(lib.head_chunks(b), O + 3, 2 * CL)
    lib.head_bwd_lazy(lazies, lnh, dn, 0, ln_w7d, ln_b7d, W_d, hb, stats7, 1, None, None, y_d, loss, part, b, C, L, O)
    k1 = _nan(b, 2 * P, 2)
    k1[:, :P] = 0.0
    dxa, dxb = _nan(b, C, L), _nan(b, C, L)
    dw, dw2 = torch.zeros(3, 2, device=d), torch.zeros(2, 2, device=d)
    lib.mixsum_pair_bwd_lazy([xa_d, xb_d, n0], [dxa, dxb, dn[0]], w, 2, w2, 2, h, None, gz_d, dw.reshape(-1)[1:],
                             dw2.reshape(-1)[1:], 0b100, [lazies[0]], [k1.reshape(-1)[2 * P:]], [2 * P], b, C, L)
    gin = []
    for k, m in enumerate(nodes):
        g_in, dV, bn_grad, dgam = _nan(b, C, L), _nan(b, 3 * C, L), torch.zeros(6 * C, device=d), torch.zeros(4, device=d)
        dx = _nan(b, C, L)
        dy = None if m.same else _nan(b, C, L)
        lib.node_mix_lnp_bwd(dn[k], pres[k], m.ln_w, nstats[k], lnh[k], k1 if k == 0 else None, g_in, None, 0, m.x, m.y,
                             m.p1, m.U, m.chan, m.gamma, dgam, dx, dy, 0, dV, bn_grad, b, C, L, m.dglu, m.dfc)
        gin.append(g_in)
    torch.cuda.synchronize()
    # float64 autograd of the same graph
    p64 = [p.clone().requires_grad_(True) for p in pre64]
    nn_ = [F.layer_norm(p64[k], (C, L), nodes[k].ln_w.cpu().double(), nodes[k].ln_b.cpu().double(), lr.EPS)
           for k in range(2)]
    wc = w_full[:, 1].cpu().double()
    s2 = w2_full[0, 1].cpu().double() + w2_full[1, 1].cpu().double()
    h64 = wc[0] * xa.double() + wc[1] * xb.double() + wc[2] * nn_[0]
    feat = F.relu(F.layer_norm(torch.cat(nn_, dim=1), (2 * C, L), ln_w7.double(), ln_b7.double(), lr.EPS))
    logits = F.linear(feat.reshape(b, -1), W.double(), bias.double())
    loss64 = F.binary_cross_entropy_with_logits(logits, y.double())
    want = torch.autograd.grad(loss64 + (s2 * h64 * gz.double()).sum(), p64)
    assert_close_scaled('logits', hb[0], logits.detach())
    assert_close_scaled('loss', loss, loss64.detach().reshape(1))
    assert_close_scaled('h', h, h64.detach())
    for k in range(2):
        assert_close_scaled(f'g_in of node {k}', gin[k], want[k])
    assert bool(torch.isfinite(k1).all())


# ------------------------------------------------------------------------------------------------------ g. refusals
def test_refusals():
    from bmnas import lib
    d = dev()
    assert not lib.lazy_ln_ok(16, 12) and not lib.lazy_ln_ok(260, 16)
    assert lib.lazy_ln_ok(256, 16) and lib.lazy_ln_ok(16, 4) and lib.lazy_ln_ok(128, 8)

    def bufs(C, L, b=1, O=5, n_src=1):
        z = lambda *s: torch.zeros(*s, device=d)
        P = (C * L // 4 + 255) // 256
        t = SimpleNamespace(a=z(b, C, L), U=z(b, 3 * C, L), chan=z(12 * C), gamma=z(4), w=z(C, L), rec=z(b, P, 8),
                            prm=z(P, 8), st=torch.ones(b, 2, device=d), col=z(8), lnp=z(b, max(P, C * L // 64 + 1), 2),
                            dV=z(b, 3 * C, L), bn=z(6 * C), W=z(O, n_src * C * L), bias=z(O), hb=z(3, b, O),
                            part=z(2, O + 3, n_src * C * L), loss=z(1), y=z(b, O), w7=z(n_src * C, L))
        t.lazy = lib.make_lazy(t.a, t.rec, t.prm, t.w, t.w, t.st)
        return t

    C, L, b = 260, 16, 1                                         # 1040 float4: a fifth part
    t = bufs(C, L)
    out = lambda: torch.zeros(b, C, L, device=d)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.node_mix_pre_fwd(t.a, t.a, t.a, t.U, t.chan, t.gamma, t.a, t.w, t.w, out(), t.rec, t.prm, b, C, L,
                             lib.NO_DROP, lib.NO_DROP)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.mixsum_pair_fwd_lazy([t.a], t.col, 2, t.col, 2, t.lazy, out(), None, out(), out(), b, C, L)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.mixsum_pair_bwd_lazy([t.a, t.a], [out(), out()], t.col, 2, t.col, 2, t.a, None, t.a, None, None, 0,
                                 [t.lazy], [t.lnp], [5], b, C, L)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.node_mix_lnp_bwd(t.a, t.a, t.w, t.st, t.lnp, None, out(), None, 0, t.a, t.a, t.a, t.U, t.chan, t.gamma,
                             None, out(), None, 0, t.dV, t.bn, b, C, L, lib.NO_DROP, lib.NO_DROP)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.head_fwd_lazy([t.a], [None], 0, t.lazy, t.w7, t.w7, t.W, t.bias, t.hb, t.st.clone(), b, C, L, 5)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.head_bwd_lazy([t.lazy], [t.lnp], [out()], 0, t.w7, t.w7, t.W, t.hb, t.st, 1, None, None, t.y, t.loss,
                          t.part, b, C, L, 5)
    # O = 129: one class beyond the widest instantiation
    C, L, O = 16, 4, 129
    t = bufs(C, L, O=O)
    out = lambda: torch.zeros(b, C, L, device=d)
    sums = torch.zeros(b, 2, device=d)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.head_fwd([t.a], [sums], t.w7, t.w7, t.W, t.bias, t.hb, t.st.clone(), b, C, L, O)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.head_fwd_lazy([t.a], [None], 0, t.lazy, t.w7, t.w7, t.W, t.bias, t.hb, t.st.clone(), b, C, L, O)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.head_bwd([t.a], [sums], [out()], 0, t.w7, t.w7, t.W, t.hb, t.st, 1, None, None, t.y, t.loss, t.part, b, C,
                     L, O)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.head_bwd_lazy([t.lazy], [t.lnp], [out()], 0, t.w7, t.w7, t.W, t.hb, t.st, 1, None, None, t.y, t.loss,
                          t.part, b, C, L, O)
    # more classes than features: the dbias row of `part` (D floats) cannot hold O entries
    t = bufs(16, 4, O=83)
    for call in (lambda: lib.head_bwd([t.a], [sums], [out()], 0, t.w7, t.w7, t.W, t.hb, t.st, 1, None, None, t.y, t.loss,
                                      t.part, b, 16, 4, 83),
                 lambda: lib.head_bwd_lazy([t.lazy], [t.lnp], [out()], 0, t.w7, t.w7, t.W, t.hb, t.st, 1, None, None, t.y,
                                           t.loss, t.part, b, 16, 4, 83)):
        with pytest.raises(lib.BmnasError, match=E_SHAPE):
            call()
    # C L = 80: the lazy backward's 64-k groups do not tile it (the plain head, 16-k blocks, takes it)
    C, L = 20, 4
    assert lib.lazy_ln_ok(C, L)
    t = bufs(C, L)
    with pytest.raises(lib.BmnasError, match=E_SHAPE):
        lib.head_bwd_lazy([t.lazy], [t.lnp], [torch.zeros(b, C, L, device=d)], 0, t.w7, t.w7, t.W, t.hb, t.st, 1, None,
                          None, t.y, t.loss, t.part, b, C, L, 5)
    torch.cuda.synchronize()
