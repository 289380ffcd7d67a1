"""The first and the last value of every run-time range that csrc/launch.hpp turns into a template argument
(dispatch_range, dispatch_of, dispatch_ln), through the C ABI against float64: a dispatcher that is off by one at an end
— a range one short, a list without its last value, the two block sizes swapped — launches the wrong instantiation or
refuses a count the entry promises.  The references are the ones the neighbouring kernel tests use (tests/mix_ref.py,
tests/lazy_ln_ref.py, tests/bn_ref.py), the tolerance helper is theirs (gpu_util.assert_close_scaled: 1e-4 of
|want| + max |want|, the setting of tests/test_lazy_ln_kernels_gpu.py for sums, LayerNorm outputs and input gradients;
3e-5 / 5e-5 for dV / bn_grad as in tests/test_mix_kernels_gpu.py); a scalar dot product over a whole tensor has no scale
of its own and is held to 5e-5 x the float64 sum of |terms| (the dw rule of tests/test_mix_kernels_gpu.py).  Every
output is a view into a NaN buffer with guard floats on each side (gpu_util.Pool).

Here:
    bmnas_mixsum_fwd, _bwd, _pair_fwd            n_in 1 and 16
    bmnas_mixsum_pair_bwd                        n_in 1 and 15, with and without dw / dw2
    bmnas_mixsum_pair_bwd_x                      n_in 15 with n_more 1 and 2
    bmnas_mixsum_pair_fwd_lazy                   n_in 15: the body of test_lazy_ln_kernels_gpu.py::test_mixsum_pair_fwd_lazy
    bmnas_mixsum_pair_bwd_lazy                   (n_in, n_lazy) = (15, 2), with and without dw: ...::test_mixsum_pair_bwd_lazy
    bmnas_bn_relu_ln_bwd_pair                    n_prev 15
    bmnas_cat_ln_fwd, _bwd                       once per <values per thread, block size> of ln_launch_shape: b = 2 (512
                                                 threads from 512 float4 on) and b = 257 (256 threads at any width), the
                                                 sample one float4 short of each edge — the last trip partly filled
Ends that an existing test already runs, not repeated:
    bmnas_mixsum_pair_fwd_lazy n_in 1, bmnas_mixsum_pair_bwd_lazy (2, 1)
                                                 test_lazy_ln_kernels_gpu.py::test_mixsum_pair_fwd_lazy, ::test_mixsum_pair_bwd_lazy
    bmnas_bn_relu_ln_fwd_pair n_prev 1 and 15    test_kernels_gpu.py::test_bn_relu_ln_fwd_with_next_pair_sum
    bmnas_bn_relu_ln_bwd_pair n_prev 1           test_kernels_gpu.py::test_bn_relu_ln_bwd_with_next_pair_backward
    bmnas_node_mix_fwd_next / _bwd_next n_prev 0 and 5
                                                 test_mix_kernels_gpu.py::test_node_mix_fwd_next, ::test_node_mix_bwd_next
    bmnas_node_mix_ln_fwd, every <VPT, BS>       test_mix_kernels_gpu.py::test_node_mix_ln_fwd (B_CASES names each)
    bmnas_cell_prologue_pair n_in 1 and 15       test_step_ends_kernels_gpu.py::test_cell_prologue_pair
    bmnas_node_mix_sel_act_fwd / _bwd, all 23    test_mix_kernels_gpu.py::test_node_mix_sel_every_instantiation
    bmnas_node_mix_lnp_bwd, 1 .. 4 pairs per lane and the loop form
                                                 test_lazy_ln_kernels_gpu.py::test_node_mix_lnp_bwd
All cases pass on the library of the parent commit (0c58601, hand-written switches) as well: BMNAS_LIB pointed at a
build of it, this file run once on an MI355X."""
import pytest
import torch

import bn_ref as br
import lazy_ln_ref as lr
import mix_ref as mr
import test_lazy_ln_kernels_gpu as tl
from gpu_util import Pool, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

R_DV, R_GRAD, R_DOT = 3e-5, 5e-5, 5e-5
SHAPE = (3, 43, 12)           # 1548 floats = 387 float4: two workgroups, the second partly filled


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _f32(g, *shape):
    return torch.randn(*shape, generator=g)


def _d(t):
    return t.to(dev()).contiguous()


def _weights(g, n):
    """(n, 2) on the device, the kernels read column 1 at stride 2 -> (device view, float32 values on the CPU)"""
    full = _d(_f32(g, n, 2))
    return full.reshape(-1)[1:], full[:, 1].cpu()


def _dots(name, got, want, abs_sum):
    got, want = got.detach().double().cpu(), want.double()
    bad = (got - want).abs() > R_DOT * abs_sum.double() + 1e-30
    assert torch.isfinite(got).all() and not bool(bad.any()), (name, got, want, abs_sum)


def _dests(pool, old, acc, skip=()):
    """destination j: NULL (skip), a NaN buffer (overwritten) or a copy of old[j] (bit j of acc: accumulated into)"""
    return [None if j in skip else pool.new(*o.shape, base=o if (acc >> j) & 1 else None) for j, o in enumerate(old)]


@pytest.mark.parametrize('n_in', [1, 16])
def test_mixsum_fwd_and_pair_fwd(n_in):
    from bmnas import lib
    g, pool = _gen(100 + n_in), Pool()
    xs = [_f32(g, *SHAPE) for _ in range(n_in)]
    xd = [_d(x) for x in xs]
    w, wc = _weights(g, n_in)
    w2, w2c = _weights(g, 2)
    out, h, z = pool.new(*SHAPE), pool.new(*SHAPE), pool.new(*SHAPE)
    lib.mixsum_fwd(xd, w, 2, out)
    lib.mixsum_pair_fwd(xd, w, 2, w2, 2, h, z)
    pool.check()
    want = mr.next_fwd(xs[:-1], wc, xs[-1])
    assert_close_scaled('out', out, want)
    assert_close_scaled('h', h, want)
    assert_close_scaled('z', z, (w2c[0].double() + w2c[1].double()) * want)


@pytest.mark.parametrize('n_in', [1, 16])
def test_mixsum_bwd(n_in):
    from bmnas import lib
    g, pool = _gen(200 + n_in), Pool()
    xs = [_f32(g, *SHAPE) for _ in range(n_in)]
    gz, gz2 = _f32(g, *SHAPE), _f32(g, *SHAPE)
    old = [_f32(g, *SHAPE) for _ in range(n_in)]
    acc = 0x5555 & ((1 << n_in) - 1)
    w, wc = _weights(g, n_in)
    dxs = _dests(pool, old, acc)
    dw_full = pool.new(n_in, 2, base=torch.zeros(n_in, 2))
    lib.mixsum_bwd([_d(x) for x in xs], dxs, w, 2, _d(gz), dw_full.reshape(-1)[1:], acc, 1, 0, _d(gz2))
    pool.check()
    G = gz.double() + gz2.double()
    for j in range(n_in):
        assert_close_scaled(f'dxs[{j}]', dxs[j], wc[j].double() * G + (old[j].double() if (acc >> j) & 1 else 0.0))
    terms = [G * x.double() for x in xs]
    _dots('dw', dw_full[:, 1], torch.stack([t.sum() for t in terms]), torch.stack([t.abs().sum() for t in terms]))
    assert float(dw_full[:, 0].abs().max()) == 0.0


def _pair_bwd_case(g, n_in):
    xs = [_f32(g, *SHAPE) for _ in range(n_in)]
    t = dict(xs=xs, h=_f32(g, *SHAPE), gh=_f32(g, *SHAPE), gz=_f32(g, *SHAPE), gz2=_f32(g, *SHAPE),
             old=[_f32(g, *SHAPE) for _ in range(n_in)], acc=0x2AAA & ((1 << n_in) - 1))
    t['w'], t['wc'] = _weights(g, n_in)
    t['w2'], t['w2c'] = _weights(g, 2)
    t['Z'] = t['gz'].double() + t['gz2'].double()
    t['G'] = (t['w2c'][0].double() + t['w2c'][1].double()) * t['Z'] + t['gh'].double()
    return t


def _pair_bwd_check(t, dxs, dw_full, dw2_full, extra=None):
    """dxs[j] = w_j G (+ extra[j]) (+ old); dw_j = <G, x_j>; dw2_0 = dw2_1 = <gz + gz2, h>"""
    for j, dx in enumerate(dxs):
        if dx is None:
            continue
        want = t['wc'][j].double() * t['G'] + (t['old'][j].double() if (t['acc'] >> j) & 1 else 0.0)
        assert_close_scaled(f'dxs[{j}]', dx, want if extra is None else want + extra[j])
    if dw_full is None:
        return
    terms = [t['G'] * x.double() for x in t['xs']]
    _dots('dw', dw_full[:, 1], torch.stack([v.sum() for v in terms]), torch.stack([v.abs().sum() for v in terms]))
    zh = t['Z'] * t['h'].double()
    _dots('dw2', dw2_full[:, 1], zh.sum().repeat(2), zh.abs().sum().repeat(2))
    assert float(dw_full[:, 0].abs().max()) == 0.0 and float(dw2_full[:, 0].abs().max()) == 0.0


@pytest.mark.parametrize('dots', [True, False])
@pytest.mark.parametrize('n_in', [1, 15])
def test_mixsum_pair_bwd(n_in, dots):
    from bmnas import lib
    g, pool = _gen(300 + n_in), Pool()
    t = _pair_bwd_case(g, n_in)
    dxs = _dests(pool, t['old'], t['acc'], skip=(3,) if n_in > 3 else ())
    dw_full = pool.new(n_in, 2, base=torch.zeros(n_in, 2)) if dots else None
    dw2_full = pool.new(2, 2, base=torch.zeros(2, 2)) if dots else None
    lib.mixsum_pair_bwd([_d(x) for x in t['xs']], dxs, t['w'], 2, t['w2'], 2, _d(t['h']), _d(t['gh']), _d(t['gz']),
                        dw_full.reshape(-1)[1:] if dots else None, dw2_full.reshape(-1)[1:] if dots else None, t['acc'],
                        1, 0, _d(t['gz2']))
    pool.check()
    _pair_bwd_check(t, dxs, dw_full, dw2_full)


@pytest.mark.parametrize('n_more', [1, 2])
def test_mixsum_pair_bwd_x_at_15_inputs(n_more):
    """dx_j = w_j G + sum_t wm_t[j] G_t, once; n_more 1 with the dot products, n_more 2 without"""
    from bmnas import lib
    n_in, dots = 15, n_more == 1
    g, pool = _gen(400 + n_more), Pool()
    t = _pair_bwd_case(g, n_in)
    g_more = [_f32(g, *SHAPE) for _ in range(n_more)]
    wm = [_weights(g, n_in) for _ in range(n_more)]
    dxs = _dests(pool, t['old'], t['acc'], skip=(7,))
    dw_full = pool.new(n_in, 2, base=torch.zeros(n_in, 2)) if dots else None
    dw2_full = pool.new(2, 2, base=torch.zeros(2, 2)) if dots else None
    lib.mixsum_pair_bwd_x([_d(x) for x in t['xs']], dxs, t['w'], 2, t['w2'], 2, _d(t['h']), _d(t['gh']), _d(t['gz']),
                          dw_full.reshape(-1)[1:] if dots else None, dw2_full.reshape(-1)[1:] if dots else None,
                          t['acc'], [_d(x) for x in g_more], [w for w, _ in wm], 1, 0, _d(t['gz2']))
    pool.check()
    extra = [sum(wm[k][1][j].double() * g_more[k].double() for k in range(n_more)) for j in range(n_in)]
    _pair_bwd_check(t, dxs, dw_full, dw2_full, extra)


def test_mixsum_pair_fwd_lazy_at_15_inputs():
    tl.test_mixsum_pair_fwd_lazy(68, 16, 15, 'sums')             # C L / 4 = 272: two parts, the second 16 float4


@pytest.mark.parametrize('variant', ['v0', 'v1'])                # with the dot products (v0) and without (v1)
def test_mixsum_pair_bwd_lazy_at_15_inputs_2_lazy(variant):
    tl.test_mixsum_pair_bwd_lazy(68, 16, 15, 2, variant)


def test_bn_relu_ln_bwd_pair_at_15_inputs():
    """G = gh + (w2_0 + w2_1) (gz + gz2); dxs[j] (=|+=) w_j G; gy = g + w_15 G = g_full; dw_j += <G, xs[j]>,
    dw_15 += <G, out>, dw2 += <gz + gz2, h>; then the tail: LayerNorm backward of gy over pre = o + resid, dresid +=,
    dV = [v > 0] g_in, bn_grad += (S(dV u_hat) | S(dV)).  chan holds scale 1 and shift 0, so v = U bit for bit, and no U
    lies within 0.05 of zero: the ReLU decision cannot differ between fp32 and float64."""
    from bmnas import lib
    n_prev, b, C, L = 15, 3, 20, 8                                # C L / 4 = 40 of the kernel's 256 lanes
    g, pool = _gen(515), Pool()
    shape = (b, C, L)
    U = _f32(g, *shape)
    U = torch.where(U >= 0, U + 0.05, U - 0.05)
    chan = torch.cat([_f32(g, C) * 0.2, _f32(g, C).abs() + 0.5, torch.ones(C), torch.zeros(C)])
    o, resid, gy_part = _f32(g, *shape).abs(), _f32(g, *shape), _f32(g, *shape)
    ln_w = _f32(g, C, L) * 0.3 + 1.0
    _, mean, rstd, _ = lr.node_ln(o.double() + resid.double(), ln_w, torch.zeros(C, L))
    stats = torch.stack([mean, rstd], 1).float().contiguous()
    xs, out_fwd = [_f32(g, *shape) for _ in range(n_prev)], _f32(g, *shape)
    h, gh, gz, gz2 = (_f32(g, *shape) for _ in range(4))
    old, old_res, old_bn = [_f32(g, *shape) for _ in range(n_prev)], _f32(g, *shape), _f32(g, 2 * C)
    acc = 0x5555 & ((1 << n_prev) - 1)
    w, wc = _weights(g, n_prev + 1)
    w2, w2c = _weights(g, 2)
    dxs = _dests(pool, old, acc, skip=(4,))
    dw_full, dw2_full = pool.new(n_prev + 1, 2, base=torch.zeros(n_prev + 1, 2)), pool.new(2, 2, base=torch.zeros(2, 2))
    g_full, dV, dres = pool.new(*shape), pool.new(*shape), pool.new(*shape, base=old_res)
    bn_grad = pool.new(2 * C, base=old_bn)
    lib.bn_relu_ln_bwd(_d(gy_part), _d(o), _d(resid), _d(ln_w), _d(stats), _d(U), _d(chan), dV, bn_grad, dres, 1, b, C,
                       L, lib.NO_DROP, ([_d(x) for x in xs], dxs, acc, _d(out_fwd), w, 2, w2, 2, _d(h), _d(gh), _d(gz),
                                        _d(gz2), dw_full.reshape(-1)[1:], dw2_full.reshape(-1)[1:], 1, 0, g_full))
    pool.check()
    Z = gz.double() + gz2.double()
    G = (w2c[0].double() + w2c[1].double()) * Z + gh.double()
    for j, dx in enumerate(dxs):
        if dx is not None:
            assert_close_scaled(f'dxs[{j}]', dx, wc[j].double() * G + (old[j].double() if (acc >> j) & 1 else 0.0))
    gy = gy_part.double() + wc[n_prev].double() * G
    assert_close_scaled('g_full', g_full, gy)
    terms = [G * x.double() for x in xs + [out_fwd]]
    _dots('dw', dw_full[:, 1], torch.stack([v.sum() for v in terms]), torch.stack([v.abs().sum() for v in terms]))
    _dots('dw2', dw2_full[:, 1], (Z * h.double()).sum().repeat(2), (Z * h.double()).abs().sum().repeat(2))
    g_in, want_res = mr.mix_ln_bwd(gy, o.double() + resid.double(), ln_w, stats, dresid_old=old_res, accumulate_resid=True)
    assert_close_scaled('dresid', dres, want_res)
    want_dV, want_bn = br.tail_bwd('relu', g_in, U, chan, prev_bn_grad=old_bn)
    assert_close_scaled('dV', dV, want_dV, rel=R_DV)
    assert_close_scaled('bn_grad', bn_grad, want_bn, rel=R_GRAD)


# (b, float4 per sample, n_src) -> <VPT, BS>; the width is n_src * C at L = 4
LN_CASES = [(2, 255, 1, '<1,256>'), (2, 510, 2, '<2,256>'), (2, 512, 1, '<1,512>'), (2, 1023, 1, '<2,512>'),
            (2, 1535, 1, '<3,512>'), (2, 2046, 2, '<4,512>'), (2, 4095, 1, '<8,512>'), (2, 8191, 1, '<16,512>'),
            (257, 767, 1, '<3,256>'), (257, 1023, 1, '<4,256>'), (257, 2047, 1, '<8,256>'), (257, 4095, 1, '<16,256>')]


@pytest.mark.parametrize('b,d4,n_src,inst', LN_CASES)
def test_cat_ln_every_launch_shape(b, d4, n_src, inst):
    from bmnas import lib
    C, L = d4 // n_src, 4
    assert C * n_src == d4
    g, pool = _gen(600 + d4 + b), Pool()
    srcs = [_f32(g, b, C, L) for _ in range(n_src)]
    resid = _f32(g, b, d4, L) if n_src == 1 else None
    ln_w, ln_b = _f32(g, d4, L) * 0.3 + 1.0, _f32(g, d4, L) * 0.2
    sd, wd, bd = [_d(s) for s in srcs], _d(ln_w), _d(ln_b)
    rd = None if resid is None else _d(resid)
    out, stats, sums = pool.new(b, d4, L), pool.new(b, 2), pool.new(b, 2)
    lib.cat_ln_fwd(sd, rd, wd, bd, out, stats, b, C, L, False, out_sums=sums)
    pool.check()
    pre = torch.cat([s.double() for s in srcs], 1) + (0.0 if resid is None else resid.double())
    want, mean, rstd, _ = lr.node_ln(pre, ln_w, ln_b)
    assert_close_scaled('out', out, want)
    assert_close_scaled('stats: mean', stats[:, 0], mean)
    assert_close_scaled('stats: rstd', stats[:, 1], rstd)
    want_sums = lr.out_sums(want)
    assert_close_scaled('out_sums: S(o)', sums[:, 0], want_sums[:, 0])
    assert_close_scaled('out_sums: S(o^2)', sums[:, 1], want_sums[:, 1])
    # backward from the float64 statistics rounded to fp32 (what the forward saves)
    st32 = torch.stack([mean, rstd], 1).float().contiguous()
    gy = _f32(g, b, d4, L)
    old = [_f32(g, b, C, L) for _ in range(n_src)]
    dsrcs = _dests(pool, old, 0b10)
    dres = None if resid is None else pool.new(b, d4, L)
    lib.cat_ln_bwd(_d(gy), sd, rd, wd, bd, _d(st32), dsrcs, dres, 0b10, None, None, b, C, L, False)
    pool.check()
    g_in, _ = mr.mix_ln_bwd(gy, pre, ln_w, st32)
    for q in range(n_src):
        assert_close_scaled(f'dsrcs[{q}]', dsrcs[q], g_in[:, q * C:(q + 1) * C] + (old[q].double() if q == 1 else 0.0))
    if dres is not None:
        assert_close_scaled('dresid', dres, g_in)
