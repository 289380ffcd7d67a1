"""The launches whose loads were regrouped into one batch per round trip — bmnas_node_mix_lnp_bwd (csrc/lazyln.hip),
bmnas_backward_epilogue and bmnas_ln_affine_bwd_multi (csrc/layernorm.hip, csrc/arch_body.hpp) — at the shapes where the
regrouped code takes another path, against float64 statements: the mix backward written out below, the epilogue's jobs
from tests/step_ends_ref.py.

What the regrouping introduced and a test here has to reach:
  node_mix_lnp_bwd   the partial pairs as 1 .. 4 clamped loads per lane (64, 65, 68, 193, 256 pairs, either list empty)
                     and the loop form above 256 (257, 300); the three old-value loads unconditional and selected
                     afterwards (every NULL / accumulate combination); idle columns (C L / 4 = 32 < 64) and idle sample
                     lanes (b = 5: a chunk of one sample) reading clamped addresses
  LayerNorm affine   four sample trips per batch, clamped: b = 1 (three idle lanes), 37 (ragged last chunk), 300 (chunks of
                     19 = five trips: a second, ragged group); a width that is no multiple of 64; absent operands that read
                     g instead (resid, stats, ln_w / ln_b, gscale)
  chunk sums         four chunks per batch: n_chunk = 1, 4, 9, lengths that are no multiple of 1024 floats
  arch rows          scalar tensor walk over all 16 slots, 1 .. 4 columns, n_shards = 1, 16, 17, 33 (one lane takes two
                     trips)
  cell prologue      the pair sum's first operand batch requested ahead of the edge weights, later trips at the end of
                     the loop (one element, a ragged workgroup, the stride loop where some lanes take two trips and
                     the rest one); a softmax row's logits as four clamped loads (1 .. 4 columns, 16 tensors, a second
                     row workgroup)
  mixsum_pair_bwd_x  the first trip's operands requested ahead of the edge weights, lanes without a first trip repeating
                     the last element (one element, a ragged workgroup), later trips of the stride loop

Bounds: assert_close_scaled at its default (1e-4 of the expected tensor's scale) against float64.  Every output starts
as NaN between NaN guards unless the ABI accumulates into it; where no atomics are involved two runs must be bit-equal.
The two ReLUs a float64 comparison crosses (ConcatFC's, the K7 LayerNorm's) are kept 1e-3 clear of zero by the inputs."""
from types import SimpleNamespace

import pytest
import torch

import step_ends_ref as sr
from gpu_util import assert_close_scaled, dev

pytestmark = pytest.mark.gpu

GUARD = 8
NAN = float('nan')
MARGIN = 1e-3


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g)


class _Pool:
    """outputs as views into NaN buffers with GUARD floats on either side"""

    def __init__(self):
        self.bufs = []

    def new(self, *shape, base=None):
        n = 1
        for s in shape:
            n *= int(s)
        buf = torch.full((n + 2 * GUARD,), NAN, device=dev())
        view = buf[GUARD:GUARD + n].view(*shape)
        if base is not None:
            view.copy_(base)
        self.bufs.append((buf, n))
        return view

    def check(self):
        torch.cuda.synchronize()
        for buf, n in self.bufs:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), \
                f'a guard of a {n}-float output was written'


# ------------------------------------------------------------------------------------------ node_mix_lnp_bwd: float64
def _lnp_inputs(seed, b, C, L, n0, n1, drop):
    """Everything the kernel reads, as the fp32 values it sees, and their float64 copies."""
    from bmnas import lib
    g, d = _gen(seed), dev()
    M = 3 * C
    c = SimpleNamespace(b=b, C=C, L=L, n0=n0, n1=n1)
    c.x, c.y, c.p1 = _rand(g, b, C, L), _rand(g, b, C, L), _rand(g, b, C, L)
    c.U = _rand(g, b, M, L)
    c.pre, c.gy = _rand(g, b, C, L) * 1.5 + 0.2, _rand(g, b, C, L)
    c.ln_w = _rand(g, C, L) * 0.3 + 1.0
    c.gamma = torch.softmax(_rand(g, 4), 0)
    mu = c.U.double().mean(dim=(0, 2))
    rs = 1.0 / torch.sqrt(c.U.double().var(dim=(0, 2), unbiased=False) + 1e-5)
    sc = rs * (_rand(g, M) * 0.3 + 1.0).double()
    c.chan = torch.cat([mu, rs, sc, (_rand(g, M) * 0.2).double() - mu * sc]).float().contiguous()
    # ConcatFC's ReLU argument at least MARGIN from zero (the fp32 kernel and float64 must agree on its sign)
    ch = c.chan.double().reshape(4, M)
    for _ in range(8):
        vf = c.U[:, 2 * C:].double() * ch[2, 2 * C:, None] + ch[3, 2 * C:, None]
        near = vf.abs() < 2.0 * MARGIN
        if not bool(near.any()):
            break
        c.U[:, 2 * C:][near] += 0.05
    else:
        raise AssertionError('could not clear the ConcatFC ReLU arguments')
    x64 = c.pre.double().reshape(b, -1)
    mean = x64.mean(1)
    c.stats = torch.stack([mean, 1.0 / torch.sqrt(((x64 - mean[:, None]) ** 2).mean(1) + 1e-5)], 1).float().contiguous()
    # the partial pairs: any values will do — the kernel only adds them up
    c.lnp0 = (_rand(g, b, n0, 2) * 3.0).contiguous() if n0 else None
    c.lnp1 = (_rand(g, b, n1, 2) * 3.0).contiguous() if n1 else None
    c.old_r, c.old_x, c.old_y = _rand(g, b, C, L), _rand(g, b, C, L), _rand(g, b, C, L)
    c.dglu = lib.make_dropout(0.1, 99 + seed, 0) if drop else lib.NO_DROP
    c.dfc = lib.make_dropout(0.2, 99 + seed, b * C * L // 4) if drop else lib.NO_DROP
    n = b * C * L
    c.m2 = lib.dropout_mask(c.dglu, n, d).cpu().double().reshape(b, C, L)
    c.m3 = lib.dropout_mask(c.dfc, n, d).cpu().double().reshape(b, C, L)
    if drop:
        assert 0.02 < float((c.m2 == 0).double().mean()) < 0.3 and 0.05 < float((c.m3 == 0).double().mean()) < 0.4
    c.dev = {k: getattr(c, k).to(d) for k in ('x', 'y', 'p1', 'U', 'pre', 'gy', 'ln_w', 'gamma', 'chan', 'stats')}
    c.dev['lnp0'] = None if c.lnp0 is None else c.lnp0.to(d)
    c.dev['lnp1'] = None if c.lnp1 is None else c.lnp1.to(d)
    c.want = _lnp_ref(c)
    return c


def _lnp_ref(c):
    """g = rstd (gy w - S1 / N - xhat S2 / N) with S = the sum of every partial pair, then the mix backward:
    dgamma, da | dg | df (gradients of the BatchNorm outputs), their per-channel sums sw = S(d xhat_bn), sb = S(d)."""
    b, C, L = c.b, c.C, c.L
    N, M = C * L, 3 * C
    S = torch.zeros(b, 2, dtype=torch.float64)
    for p in (c.lnp0, c.lnp1):
        if p is not None:
            S = S + p.double().sum(1)
    mean, rstd = c.stats[:, 0].double()[:, None, None], c.stats[:, 1].double()[:, None, None]
    xhat = (c.pre.double() - mean) * rstd
    g = rstd * (c.gy.double() * c.ln_w.double() - S[:, 0, None, None] / N - xhat * S[:, 1, None, None] / N)
    ch = c.chan.double().reshape(4, M)
    gam = c.gamma.double()
    U = c.U.double()
    blk = lambda t, k: t[k * C:(k + 1) * C][None, :, None]
    u = [U[:, k * C:(k + 1) * C] for k in range(3)]
    v = [u[k] * blk(ch[2], k) + blk(ch[3], k) for k in range(3)]
    sg = torch.sigmoid(v[1])
    dgamma = torch.stack([(g * (c.x.double() + c.y.double())).sum(), (g * c.p1.double()).sum(),
                          (g * v[0] * sg * c.m2).sum(), (g * v[2].clamp(min=0) * c.m3).sum()])
    gm = gam[2] * g * c.m2
    dk = [gm * sg, gm * v[0] * sg * (1.0 - sg), torch.where(v[2] > 0, gam[3] * g * c.m3, torch.zeros_like(g))]
    sw = [(dk[k] * (u[k] - blk(ch[0], k)) * blk(ch[1], k)).sum(dim=(0, 2)) for k in range(3)]
    sb = [dk[k].sum(dim=(0, 2)) for k in range(3)]
    return SimpleNamespace(g=g, dgamma=dgamma, dV=torch.cat(dk, dim=1), bn_grad=torch.cat(sw + sb), g0=gam[0])


def _lnp_run(c, racc, acc, has, det, shards=3):
    """One launch.  has: which of g_in, dresid, dx, dy are given.  -> the outputs, on the CPU, and the expectations."""
    from bmnas import lib
    d, v = dev(), c.dev
    b, C, L = c.b, c.C, c.L
    pool = _Pool()
    gin = pool.new(b, C, L) if 'g_in' in has else None
    dres = pool.new(b, C, L, base=c.old_r if racc else None) if 'dresid' in has else None
    dx = pool.new(b, C, L, base=c.old_x if acc & 1 else None) if 'dx' in has else None
    dy = pool.new(b, C, L, base=c.old_y if acc & 2 else None) if 'dy' in has else None
    dV = pool.new(b, 3 * C, L)
    bn_grad = torch.zeros(6 * C, device=d)
    dgam = torch.zeros(shards, 4, device=d)
    bn_part = pool.new(lib.node_mix_lnp_bwd_rows(b), 6 * C) if det else None
    lib.node_mix_lnp_bwd(v['gy'], v['pre'], v['ln_w'], v['stats'], v['lnp0'], v['lnp1'], gin, dres, racc, v['x'], v['y'],
                         v['p1'], v['U'], v['chan'], v['gamma'], dgam, dx, dy, acc, dV, bn_grad, b, C, L, c.dglu, c.dfc,
                         dg_shards=shards, dg_stride=4, bn_part=bn_part)
    pool.check()
    w = c.want
    got = dict(dV=dV, bn_grad=bn_grad, dgamma=dgam.sum(0))
    want = dict(dV=w.dV, bn_grad=w.bn_grad, dgamma=w.dgamma)
    if gin is not None:
        got['g_in'], want['g_in'] = gin, w.g
    if dres is not None:
        got['dresid'], want['dresid'] = dres, w.g + (c.old_r.double() if racc else 0.0)
    if dx is not None:
        got['dx'] = dx
        want['dx'] = (2.0 if dy is None else 1.0) * w.g0 * w.g + (c.old_x.double() if acc & 1 else 0.0)
    if dy is not None:
        got['dy'], want['dy'] = dy, w.g0 * w.g + (c.old_y.double() if acc & 2 else 0.0)
    if det:
        got['bn_part'] = bn_part
    return {k: t.detach().cpu() for k, t in got.items()}, want


def _lnp_check(tag, got, want):
    for k, wv in want.items():
        assert_close_scaled(f'{tag} {k}', got[k], wv)


_ALL = ('g_in', 'dresid', 'dx', 'dy')


def _subsets():
    for m in range(16):
        yield tuple(n for i, n in enumerate(_ALL) if m >> i & 1)


@pytest.mark.parametrize('det', [False, True])
@pytest.mark.parametrize('drop', [False, True])
def test_lnp_bwd_half_empty_workgroup_every_switch(drop, det):
    """C L / 4 = 32 of a workgroup's 64 columns, b = 5 (the second sample chunk holds one sample): accumulate_resid x
    accumulate_mask x every NULL / given combination of g_in, dresid, dx, dy (accumulate_resid needs dresid)."""
    c = _lnp_inputs(11 + 2 * drop + det, 5, 32, 4, 3, 2, drop)
    n = 0
    for has in _subsets():
        for racc in (0, 1):
            if racc and 'dresid' not in has:
                continue
            for acc in range(4):
                got, want = _lnp_run(c, racc, acc, has, det)
                _lnp_check(f'has={has} racc={racc} acc={acc}', got, want)
                n += 1
    assert n == 96


# n0, n1: pair counts at the edges of the per-lane load count (64 | 65, 128 | 129 via 68 and 193, 256 | 257) and past it
_PAIRS = [(64, 0), (0, 64), (64, 1), (64, 4), (0, 4), (4, 0), (189, 4), (17, 239), (257, 0), (200, 100)]


@pytest.mark.parametrize('n0,n1', _PAIRS)
def test_lnp_bwd_pair_counts_small(n0, n1):
    c = _lnp_inputs(100 + n0 + 3 * n1, 5, 32, 4, n0, n1, True)
    for det in (False, True):
        got, want = _lnp_run(c, 1, 3, _ALL, det)
        _lnp_check(f'n0={n0} n1={n1} det={det}', got, want)


@pytest.mark.parametrize('b', [5, 4])
@pytest.mark.parametrize('n0,n1', [(64, 4), (64, 0), (64, 1), (0, 4), (200, 100)])
def test_lnp_bwd_pair_counts_full_width(n0, n1, b):
    """C = 256, L = 16: sixteen column blocks, four lanes per channel row; b = 4 fills the sample lanes, b = 5 adds a
    chunk of one"""
    c = _lnp_inputs(200 + n0 + 3 * n1 + b, b, 256, 16, n0, n1, b == 5)
    got, want = _lnp_run(c, 1, 1, ('g_in', 'dresid', 'dx'), False)           # dy NULL: both halves of the Sum term to dx
    _lnp_check(f'n0={n0} n1={n1} atomics', got, want)
    d1, want = _lnp_run(c, 0, 2, _ALL, True)
    _lnp_check(f'n0={n0} n1={n1} bn_part', d1, want)
    d2, _ = _lnp_run(c, 0, 2, _ALL, True)
    for k in ('g_in', 'dresid', 'dx', 'dy', 'dV', 'bn_part', 'bn_grad'):     # plain stores only: bit-equal
        assert torch.equal(d1[k], d2[k]), k


def test_lnp_bwd_long_sample_chunks():
    """b = 261: chunks of eight samples, two trips per lane — the second trip's loads are requested behind the first
    trip's stores"""
    c = _lnp_inputs(300, 261, 32, 4, 64, 4, True)
    got, want = _lnp_run(c, 1, 3, _ALL, False)
    _lnp_check('b=261', got, want)
    d1, want = _lnp_run(c, 0, 0, _ALL, True)
    _lnp_check('b=261 bn_part', d1, want)
    d2, _ = _lnp_run(c, 0, 0, _ALL, True)
    for k in ('g_in', 'dresid', 'dx', 'dy', 'dV', 'bn_part', 'bn_grad'):
        assert torch.equal(d1[k], d2[k]), k


# --------------------------------------------------------------------------------------------- the backward epilogue
LN_KINDS = ['k7', 'k6', 'attn']                     # relu over cat(srcs) | one source + resid | prenorm


def _ln_problem(g, kind, Cc, L, n_src, b, gscale):
    d = dev()
    if kind != 'k7':
        n_src = 1
    N = n_src * Cc * L
    srcs = [_rand(g, b, Cc, L) * 1.5 + 0.2 for _ in range(n_src)]
    resid = _rand(g, b, Cc, L) if kind == 'k6' else None
    ln_w, ln_b = _rand(g, N) * 0.3 + 1.0, _rand(g, N) * 0.2
    gy = _rand(g, b, N)
    x = torch.cat([s.double().reshape(b, -1) for s in srcs], dim=1)
    if resid is not None:
        x = x + resid.double().reshape(b, -1)
    mean = x.mean(1)
    rstd = 1.0 / torch.sqrt(((x - mean[:, None]) ** 2).mean(1) + 1e-5)
    stats = torch.stack([mean, rstd], dim=1).float().contiguous()
    relu = prenorm = 0
    if kind == 'k7':
        relu = 1
        ln_b = sr.clear_relu_bias(g, srcs, ln_w, ln_b)
        xhat = (x - stats[:, 0:1].double()) * stats[:, 1:2].double()
        assert float((xhat * ln_w.double() + ln_b.double()).abs().min()) >= sr.RELU_MARGIN
    if kind == 'attn':
        prenorm = 1
        srcs = [((x - mean[:, None]) * rstd[:, None]).float().reshape(b, Cc, L)]
        stats, ln_w, ln_b = None, None, None
    gs = torch.tensor([0.37]) if gscale else None
    dw, db = sr.ln_affine(gy, gs, srcs, resid, ln_w, ln_b, stats, relu, prenorm)
    base_w, base_b = _rand(g, N), _rand(g, N)
    dv = lambda t: None if t is None else t.to(d)
    dev_in = dict(g=dv(gy), gscale=dv(gs), srcs=[dv(s) for s in srcs], resid=dv(resid), ln_w=dv(ln_w), ln_b=dv(ln_b),
                  stats=dv(stats), C=Cc, relu=relu, prenorm=prenorm)           # (the ABI's C is per source)

    def prob(pool):
        o = (pool.new(N, base=base_w), pool.new(N, base=base_b))
        return dict(dev_in, dln_w=o[0], dln_b=o[1]), o
    return SimpleNamespace(N=N, b=b, want_w=base_w.double() + dw, want_b=base_b.double() + db, prob=prob)


def _ln_check(tag, p, outs):
    assert_close_scaled(tag + ' dln_w', outs[0], p.want_w)
    assert_close_scaled(tag + ' dln_b', outs[1], p.want_b)


# per-source (C, L), sources of the k7 kind: C L / 4 x sources = 64 (one full block), 65, 129 (three blocks, the last of one
# column), 3 x 16 + ... = 48 (a source boundary inside a block)
LN_SHAPES = [(64, 4, 1), (65, 4, 1), (129, 4, 1), (16, 4, 3)]


@pytest.mark.parametrize('b', [1, 37, 300])
@pytest.mark.parametrize('kind', LN_KINDS)
@pytest.mark.parametrize('Cc,L,n_src', LN_SHAPES)
def test_ln_affine_one_problem_both_entry_points(Cc, L, n_src, kind, b):
    from bmnas import lib
    for gscale in (False, True):
        g = _gen(1000 + Cc + n_src + b + 7 * gscale + len(kind))
        p = _ln_problem(g, kind, Cc, L, n_src, b, gscale)
        pool = _Pool()
        pm, om = p.prob(pool)
        pe, oe = p.prob(pool)
        lib.ln_affine_bwd_multi([pm], b, L)
        lib.backward_epilogue([pe], b, L, [], [], [], 1, 0)
        pool.check()
        _ln_check(f'{kind} b={b} gscale={gscale} ln_affine_bwd_multi', p, om)
        _ln_check(f'{kind} b={b} gscale={gscale} backward_epilogue', p, oe)


def _eight(g, b):
    spec = [('k7', 16, 3), ('k6', 65, 1), ('attn', 64, 1), ('k7', 129, 1), ('k6', 1, 1), ('attn', 129, 1), ('k7', 33, 2),
            ('k6', 64, 1)]
    return [_ln_problem(g, kind, Cc, 4, n_src, b, i % 2 == 1) for i, (kind, Cc, n_src) in enumerate(spec)]


ARCH_MAX16 = [(t + 1, t % 4 + 1) for t in range(16)]                # 16 tensors, 1 .. 4 columns, 136 rows
ARCH_NET = [(8, 2), (2, 2), (3, 4)]


def _arch(g, shapes, n_shards, pad=12):
    total = sum(r * c for r, c in shapes)
    stride = total + pad
    ws = [sr.row_softmax(_rand(g, r, c)).float() for r, c in shapes]
    shards = torch.full((n_shards, stride), NAN)
    shards[:, :total] = _rand(g, n_shards, total)
    sd = shards.to(dev())
    dws, views, at = [], [], 0
    for r, c in shapes:
        dws.append(sd[0, at:at + r * c].view(r, c))
        views.append(shards[:, at:at + r * c].reshape(n_shards, r, c))
        at += r * c
    return ws, [w.to(dev()) for w in ws], dws, views, stride, sd


SUMS = [(1, 4), (4, 1020), (9, 4100), (4, 4096)]                    # (n_chunk, n floats)


@pytest.mark.parametrize('b', [1, 37, 300])
@pytest.mark.parametrize('n_shards', [1, 16, 17, 33])
def test_full_epilogue_eight_problems_sixteen_tensors_two_sums(n_shards, b):
    from bmnas import lib
    g, d = _gen(2000 + n_shards + b), dev()
    ps = _eight(g, b)
    ws, wd, dws, views, stride, _keep = _arch(g, ARCH_MAX16, n_shards)
    which = [(SUMS[1], SUMS[2]), (SUMS[0], SUMS[3]), (SUMS[2], SUMS[0])][b % 3]
    parts = [_rand(g, c * n) for c, n in which]
    pool = _Pool()
    probs, outs = zip(*[p.prob(pool) for p in ps])
    arch_o = [pool.new(r, c) for r, c in ARCH_MAX16]
    sum_o = [pool.new(n) for _, n in which]
    lib.backward_epilogue(list(probs), b, 4, wd, dws, arch_o, n_shards, stride,
                          sums=[(p.to(d), o, c) for p, o, (c, _) in zip(parts, sum_o, which)])
    pool.check()
    for i, p in enumerate(ps):
        _ln_check(f'problem {i}', p, outs[i])
    for t, (r, c) in enumerate(ARCH_MAX16):
        assert_close_scaled(f'arch tensor {t}', arch_o[t], sr.row_softmax_bwd(ws[t], views[t]))
        if c == 1:
            assert float(arch_o[t].abs().max()) == 0.0
    for k, (c, _) in enumerate(which):
        assert_close_scaled(f'sum {k}', sum_o[k], sr.chunk_sum(parts[k], c))
    # ... and the eight problems through the entry point without the other jobs
    pool2 = _Pool()
    probs2, outs2 = zip(*[p.prob(pool2) for p in ps])
    lib.ln_affine_bwd_multi(list(probs2), b, 4)
    pool2.check()
    for i, p in enumerate(ps):
        _ln_check(f'multi problem {i}', p, outs2[i])


@pytest.mark.parametrize('n_chunk,n', SUMS)
def test_epilogue_one_problem_net_tensors_one_sum(n_chunk, n):
    """the smallest launch that carries every job; the arch rows and the sums are plain stores: two runs bit-equal"""
    from bmnas import lib
    g, d = _gen(3000 + n_chunk + n), dev()
    p = _ln_problem(g, 'k6', 65, 4, 1, 37, False)
    ws, wd, dws, views, stride, _keep = _arch(g, ARCH_NET, 16, pad=0)
    part = _rand(g, n_chunk * n)
    runs = []
    for _ in range(2):
        pool = _Pool()
        pr, o = p.prob(pool)
        arch_o = [pool.new(r, c) for r, c in ARCH_NET]
        out = pool.new(n)
        lib.backward_epilogue([pr], 37, 4, wd, dws, arch_o, 16, stride, sums=[(part.to(d), out, n_chunk)])
        pool.check()
        _ln_check('LN', p, o)
        for t in range(len(ARCH_NET)):
            assert_close_scaled(f'arch tensor {t}', arch_o[t], sr.row_softmax_bwd(ws[t], views[t]))
        assert_close_scaled('sum', out, sr.chunk_sum(part, n_chunk))
        runs.append([t.cpu() for t in arch_o] + [out.cpu()])
    for a, bb in zip(*runs):
        assert torch.equal(a, bb)


# ------------------------------------------------------------------------------------------------- the cell prologue
PAIR_BIG = 4 * (2048 * 256 + 300)                   # 300 lanes take a second trip of the stride loop
ARCH_257 = [(200, 4), (57, 3)]                      # a second workgroup of rows, holding one row


@pytest.mark.parametrize('n_in,n_elem', [(1, 4), (6, 4), (6, 1020), (15, 1020), (6, 192 * 16 * 5), (1, PAIR_BIG),
                                         (3, PAIR_BIG)])
@pytest.mark.parametrize('shapes', [ARCH_MAX16, ARCH_257], ids=['max16', 'rows257'])
def test_cell_prologue_pair_rows_and_trips(shapes, n_in, n_elem):
    from bmnas import lib
    g, d = _gen(4000 + n_in + n_elem % 1013 + len(shapes)), dev()
    xs = [_rand(g, n_elem) for _ in range(n_in)]
    alpha, beta = _rand(g, n_in, 2) * 2.0, _rand(g, 2, 2) * 2.0
    logits = [_rand(g, r, c) * 3.0 for r, c in shapes]
    logits[0][0] += 1e4                                              # a common offset on one row
    logits[-1][-1, 0] += 90.0                                        # a winner on another
    M, Cc = 48, 16
    Ws = [_rand(g, M, 2 * Cc) for _ in range(2)]
    pool = _Pool()
    outs = [pool.new(r, c) for r, c in shapes]
    Weffs = [pool.new(M, Cc) for _ in Ws]
    h, z = pool.new(n_elem), pool.new(n_elem)
    lib.cell_prologue_pair([a.to(d) for a in logits], outs, [w.to(d) for w in Ws], Weffs, M, Cc, None, None,
                           [x.to(d) for x in xs], alpha.to(d), beta.to(d), h, z)
    pool.check()
    want_h, want_z = sr.pair_sum(xs, alpha, beta)
    assert_close_scaled('h', h, want_h)
    assert_close_scaled('z', z, want_z)
    for t, a in enumerate(logits):
        assert_close_scaled(f'softmax {t}', outs[t], sr.row_softmax(a))
        if a.shape[1] == 1:
            assert bool((outs[t] == 1.0).all())
    assert float(outs[-1][-1, 0]) == 1.0                             # the winner is exactly 1
    for q, w in enumerate(Ws):
        assert torch.equal(Weffs[q].cpu(), w[:, :Cc] + w[:, Cc:])
    # the stand-alone prologue shares the row code
    pool2 = _Pool()
    outs2 = [pool2.new(r, c) for r, c in shapes]
    lib.cell_prologue([a.to(d) for a in logits], outs2, [], [], 0, 0)
    pool2.check()
    for t in range(len(shapes)):
        assert torch.equal(outs[t], outs2[t]), t


# ------------------------------------------------------------------------- the first step's pair backward (write-once form)
@pytest.mark.parametrize('dots', [True, False])
@pytest.mark.parametrize('n_in,n_more,n_elem,have_gh,have_gz2', [
    (1, 1, 4, False, False), (6, 1, 4, True, True), (6, 1, 1020, True, False), (6, 2, 192 * 16 * 5, False, True),
    (15, 2, 1020, True, True), (9, 1, 4100, True, True), (2, 1, PAIR_BIG, True, True)])
def test_mixsum_pair_bwd_x_trips(n_in, n_more, n_elem, have_gh, have_gz2, dots):
    """dx_j = w_j G + sum_t wm_t[j] G_t (+ old), G = (b0 + b1) (gz + gz2) + gh;  dw_j = S(G x_j), dw2 = S((gz + gz2) h)"""
    from bmnas import lib
    g, d = _gen(5000 + n_in + 3 * n_more + n_elem % 1013), dev()
    xs = [_rand(g, n_elem) for _ in range(n_in)]
    h, gz = _rand(g, n_elem), _rand(g, n_elem)
    gh = _rand(g, n_elem) if have_gh else None
    gz2 = _rand(g, n_elem) if have_gz2 else None
    aw, bw = torch.softmax(_rand(g, n_in, 2), -1), torch.softmax(_rand(g, 2, 2), -1)
    g_more = [_rand(g, n_elem) for _ in range(n_more)]
    w_more = [torch.softmax(_rand(g, n_in, 2), -1) for _ in range(n_more)]
    old = [_rand(g, n_elem) for _ in range(n_in)]
    acc = 0b101011 & ((1 << n_in) - 1)
    dv = lambda t: None if t is None else t.to(d)
    pool = _Pool()
    dxs = [None if j % 4 == 3 else pool.new(n_elem, base=old[j] if acc >> j & 1 else None) for j in range(n_in)]
    shards, S = 3, 2 * n_in + 4                                      # per shard: the (n_in, 2) dalpha rows | the (2, 2) dbeta rows
    arena = torch.zeros(shards, S, device=d)
    awd, bwd = aw.to(d), bw.to(d)
    wmd = [w.to(d) for w in w_more]
    lib.mixsum_pair_bwd_x([dv(x) for x in xs], dxs, awd[:, 1], 2, bwd[:, 1], 2, dv(h), dv(gh), dv(gz),
                          arena[0, 1:] if dots else None, arena[0, 2 * n_in + 1:] if dots else None, acc,
                          [dv(t) for t in g_more], [w[:, 1] for w in wmd], shards, S, dv(gz2))
    pool.check()
    z = gz.double() + (gz2.double() if have_gz2 else 0.0)
    G = (bw[0, 1].double() + bw[1, 1].double()) * z + (gh.double() if have_gh else 0.0)
    for j in range(n_in):
        if dxs[j] is None:
            continue
        want = aw[j, 1].double() * G + sum(w_more[t][j, 1].double() * g_more[t].double() for t in range(n_more))
        if acc >> j & 1:
            want = want + old[j].double()
        assert_close_scaled(f'dx {j}', dxs[j], want)
    tot = arena.sum(0).cpu()
    if dots:
        assert_close_scaled('dw', tot[1:2 * n_in:2], torch.stack([(G * x.double()).sum() for x in xs]))
        zh = (z * h.double()).sum()
        assert_close_scaled('dw2', tot[2 * n_in + 1::2], torch.stack([zh, zh]))
    assert float(tot[0::2].abs().max()) == 0.0                       # column 0 of every row is nobody's
    if not dots:
        assert float(tot.abs().max()) == 0.0
