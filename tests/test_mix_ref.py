"""CPU: tests/mix_ref.py (the float64 statement the mix kernels are held to in tests/test_mix_kernels_gpu.py) against
torch autograd in float64 — every function, every presence mask, both activations, x is y, aliased dprev — and
mix_ref.clear_fc_relu at the largest shape the GPU file uses."""
import pytest
import torch
import torch.nn.functional as F

import mix_ref as mr

F64 = torch.float64
TOL = dict(rtol=1e-11, atol=1e-11)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _r(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _drop_mask(g, p, *shape):
    return (torch.rand(*shape, generator=g) >= p).double() / (1.0 - p)


def _problem(g, mask, b, C, L, same=False, drop=True):
    M, fo = mr.conv_rows(mask, C)
    n = bin(mask).count('1')
    perm = torch.randperm(n, generator=g).tolist()
    cols, at = [-1] * 4, 0
    for k in range(4):
        if mask >> k & 1:
            cols[k] = perm[at]
            at += 1
    x = _r(g, b, C, L)
    y = x if same else _r(g, b, C, L)
    p1, U, gamma, grad = _r(g, b, C, L), (_r(g, b, M, L) * 1.5 + 0.3 if M else None), _r(g, n), _r(g, b, C, L)
    bn_w, bn_b = 1.0 + 0.3 * _r(g, max(M, 1))[:M], 0.2 * _r(g, max(M, 1))[:M]
    m2 = _drop_mask(g, 0.1, b, C, L) if drop else None
    m3 = _drop_mask(g, 0.2, b, C, L) if drop else None
    return dict(mask=mask, cols=cols, x=x, y=y, p1=p1, U=U, gamma=gamma, g=grad, bn_w=bn_w, bn_b=bn_b, m2=m2, m3=m3,
                M=M, fo=fo, b=b, C=C, L=L)


def _torch_mix(p, act, x, y, p1, U, gamma, bn_w, bn_b):
    """the module's own op sequence in torch (training-mode batch_norm, glu, relu / mish), dropout as given masks"""
    C, mask, cols = p['C'], p['mask'], p['cols']
    s = 0.0
    if mask & 1:
        s = s + gamma[cols[0]] * (x + y)
    if mask & 2:
        s = s + gamma[cols[1]] * p1
    if p['M']:
        V = F.batch_norm(U, None, None, bn_w, bn_b, training=True, eps=1e-5)
        if mask & 4:
            t = F.glu(V[:, :2 * C], dim=1)
            s = s + gamma[cols[2]] * (t if p['m2'] is None else t * p['m2'])
        if mask & 8:
            vf = V[:, p['fo']:]
            t = torch.relu(vf) if act == 'relu' else F.mish(vf)
            s = s + gamma[cols[3]] * (t if p['m3'] is None else t * p['m3'])
    return s


def _chan(U, bn_w, bn_b):
    mean = U.mean(dim=(0, 2))
    rstd = 1.0 / torch.sqrt(U.var(dim=(0, 2), unbiased=False) + 1e-5)
    scale = bn_w * rstd
    return torch.cat([mean, rstd, scale, bn_b - mean * scale])


CASES = [(m, 'relu') for m in range(1, 16)] + [(m, 'mish') for m in range(8, 16)]


@pytest.mark.parametrize('mask,act', CASES)
@pytest.mark.parametrize('same', [False, True])
def test_mix_fwd_and_bwd_match_autograd(mask, act, same):
    g = _gen(100 * mask + (act == 'mish') + 2 * same)
    p = _problem(g, mask, 3, 4, 8, same=same)
    M = p['M']
    leaves = {k: p[k].clone().requires_grad_(True) for k in ('x', 'p1', 'gamma')}
    if not same:
        leaves['y'] = p['y'].clone().requires_grad_(True)
    if M:
        leaves.update(U=p['U'].clone().requires_grad_(True), bn_w=p['bn_w'].clone().requires_grad_(True),
                      bn_b=p['bn_b'].clone().requires_grad_(True))
    s_t = _torch_mix(p, act, leaves['x'], leaves['x'] if same else leaves['y'], leaves['p1'], leaves.get('U'),
                     leaves['gamma'], leaves.get('bn_w'), leaves.get('bn_b'))
    chan = _chan(p['U'], p['bn_w'], p['bn_b']) if M else None
    sc, sh = (chan[2 * M:3 * M], chan[3 * M:]) if M else (None, None)
    s = mr.mix_fwd(mask, act, p['cols'], p['gamma'], p['x'], p['y'], p['p1'], p['U'], sc, sh, p['m2'], p['m3'])
    torch.testing.assert_close(s, s_t.detach(), **TOL)
    s_t.backward(p['g'])
    prev = _r(g, 2 * M) if M else None
    old_x, old_y = _r(g, 3, 4, 8), _r(g, 3, 4, 8)
    r = mr.mix_bwd(mask, act, p['cols'], p['gamma'], p['g'], p['x'], p['y'], p['p1'], p['U'], chan, p['m2'], p['m3'],
                   dx_old=old_x, dy_old=None if same else old_y, acc_mask=2, prev_bn_grad=prev)
    torch.testing.assert_close(r['dgamma'], leaves['gamma'].grad, **TOL)
    assert bool((r['dgamma_abs'] >= r['dgamma'].abs() - 1e-12).all())
    if M:
        # dV is the gradient at the BatchNorm OUTPUT: bn_grad are the affine gradients, and the train-mode input
        # gradient follows from dV and bn_grad (bn_ref.phase_b's formula)
        bg = r['bn_grad'] - prev
        torch.testing.assert_close(bg[:M], leaves['bn_w'].grad, **TOL)
        torch.testing.assert_close(bg[M:], leaves['bn_b'].grad, **TOL)
        N = 3 * 8
        uhat = (p['U'] - chan[:M][None, :, None]) * chan[M:2 * M][None, :, None]
        dU = chan[2 * M:3 * M][None, :, None] * (r['dV'] - bg[M:][None, :, None] / N - uhat * bg[:M][None, :, None] / N)
        torch.testing.assert_close(dU, leaves['U'].grad, **TOL)
    else:
        assert r['dV'] is None and r['bn_grad'] is None
    if mask & 1:
        assert r['dx_rule'] == 'write'
        torch.testing.assert_close(r['dx'], leaves['x'].grad, **TOL)                  # bit 0 clear: overwrite
        if same:
            assert r['dy'] is None                                                    # both halves went to dx
            torch.testing.assert_close(r['dx'], 2.0 * p['gamma'][p['cols'][0]] * p['g'], **TOL)
        else:
            torch.testing.assert_close(r['dy'], leaves['y'].grad + old_y, **TOL)      # bit 1 set: accumulate
    else:
        assert leaves['x'].grad is None or float(leaves['x'].grad.abs().max()) == 0.0
        assert r['dx_rule'] == 'zero' and float(r['dx'].abs().max()) == 0.0
        if not same:
            assert r['dy_rule'] == 'keep' and torch.equal(r['dy'], old_y)


def test_relu_gradient_at_exactly_zero_is_zero():
    g = _gen(7)
    p = _problem(g, 15, 2, 4, 4, drop=False)
    chan = _chan(p['U'], p['bn_w'], p['bn_b'])
    chan[3 * 12 + 2 * 4 + 1] = 0.0                         # shift of FC channel 1
    p['U'][:, 2 * 4 + 1, :2] = 0.0
    r = mr.mix_bwd(15, 'relu', mr.IDENT, p['gamma'], p['g'], p['x'], p['y'], p['p1'], p['U'], chan)
    assert float(r['dV'][:, 9, :2].abs().max()) == 0.0 and float(r['dV'][:, 9, 2:].abs().min()) >= 0.0


@pytest.mark.parametrize('n,alias', [(0, False), (1, False), (3, False), (5, False), (2, True), (3, True), (5, True)])
def test_next_step_rider_matches_autograd(n, alias):
    g = _gen(300 + n)
    b, C, L = 2, 3, 4
    prevs = [_r(g, b, C, L).requires_grad_(True) for _ in range(n)]
    w = _r(g, n + 1).requires_grad_(True)
    s = _r(g, b, C, L).requires_grad_(True)
    z = mr.next_fwd([p.detach() for p in prevs], w.detach(), s.detach())
    z_t = sum((w[j] * prevs[j] for j in range(n)), w[n] * s)
    torch.testing.assert_close(z, z_t.detach(), **TOL)
    gz, gz2, g_in = _r(g, b, C, L), _r(g, b, C, L), _r(g, b, C, L)
    z_t.backward(gz + gz2)
    dest = [f'd{j}' for j in range(n)]
    if n >= 3:
        dest[1] = None                                     # a NULL destination in the middle
    if alias:
        dest[-1] = 'd0'
    old = {k: _r(g, b, C, L) for k in set(dest) if k is not None}
    acc = 0b10101 & ((1 << n) - 1)
    if alias:
        acc |= 1 << (n - 1)                                # the aliasing write accumulates onto what j = 0 left
    r = mr.next_bwd([p.detach() for p in prevs], w.detach(), s.detach(), gz, gz2, g_in, old, dest, acc)
    torch.testing.assert_close(r['G'], gz + gz2, **TOL)
    torch.testing.assert_close(r['g_out'], g_in + s.grad, **TOL)
    torch.testing.assert_close(r['dw'], w.grad, **TOL)
    assert bool((r['dw_abs'] >= r['dw'].abs() - 1e-12).all())
    want = {k: None for k in old}
    for j in range(n):
        if dest[j] is None:
            continue
        base = want[dest[j]] if want[dest[j]] is not None else old[dest[j]]
        want[dest[j]] = prevs[j].grad + (base if acc >> j & 1 else 0.0)
    for k in old:
        torch.testing.assert_close(r['dprev'][k], want[k], **TOL)
    r0 = mr.next_bwd([p.detach() for p in prevs], w.detach(), s.detach(), gz, None, None, old, dest, acc)
    torch.testing.assert_close(r0['g_out'], w.detach()[n] * gz, **TOL)


@pytest.mark.parametrize('C,L', [(2, 4), (6, 8), (5, 16)])
def test_layernorm_tail_matches_autograd(C, L):
    g = _gen(400 + C)
    b = 3
    s, resid = _r(g, b, C, L).requires_grad_(True), _r(g, b, C, L).requires_grad_(True)
    ln_w, ln_b = 1.0 + 0.3 * _r(g, C, L), 0.2 * _r(g, C, L)
    out_t = F.layer_norm(s + resid, (C, L), ln_w, ln_b, eps=1e-5)
    f = mr.mix_ln_fwd(s.detach(), resid.detach(), ln_w, ln_b)
    torch.testing.assert_close(f['out'], out_t.detach(), **TOL)
    torch.testing.assert_close(f['pre'], (s + resid).detach(), **TOL)
    pre = (s + resid).detach().reshape(b, -1)
    torch.testing.assert_close(f['stats'][:, 0], pre.mean(1), **TOL)
    torch.testing.assert_close(f['stats'][:, 1], 1.0 / torch.sqrt(pre.var(1, unbiased=False) + 1e-5), **TOL)
    torch.testing.assert_close(f['out_sums'], torch.stack([out_t.detach().reshape(b, -1).sum(1),
                                                            (out_t.detach() ** 2).reshape(b, -1).sum(1)], 1), **TOL)
    gy, old = _r(g, b, C, L), _r(g, b, C, L)
    out_t.backward(gy)
    g_in, dres = mr.mix_ln_bwd(gy, f['pre'], ln_w, f['stats'], old, True)
    torch.testing.assert_close(g_in, s.grad, **TOL)
    torch.testing.assert_close(dres, resid.grad + old, **TOL)
    _, dres = mr.mix_ln_bwd(gy, f['pre'], ln_w, f['stats'], old, False)
    torch.testing.assert_close(dres, resid.grad, **TOL)
    assert mr.mix_ln_bwd(gy, f['pre'], ln_w, f['stats'])[1] is None


@pytest.mark.parametrize('n_src,b,L,shards', [(1, 3, 8, 0), (2, 7, 4, 3), (3, 2, 16, 1)])
def test_mix_conv_matches_conv1d(n_src, b, L, shards):
    g = _gen(500 + n_src)
    C = 5
    K, ldw = (n_src + 1) * C, (n_src + 1) * C + 4
    srcs, s = [_r(g, b, C, L) for _ in range(n_src)], _r(g, b, C, L)
    W, bias = _r(g, C, ldw), _r(g, C)
    V, stat = mr.mix_conv(srcs, s, W, bias, shards)
    V_t = F.conv1d(torch.cat(srcs + [s], 1), W[:, :K, None], bias)
    torch.testing.assert_close(V, V_t, **TOL)
    if not shards:
        assert stat is None
        return
    assert stat.shape == (shards, C, 2)
    d = (V_t - bias[None, :, None]).permute(1, 0, 2).reshape(C, -1)
    torch.testing.assert_close(stat.sum(0), torch.stack([d.sum(1), (d * d).sum(1)], 1), **TOL)
    n_g = (b * L + 15) // 16
    for sh in range(shards):                               # 16-column group g goes to shard g % shards
        cols = torch.cat([torch.arange(16 * q, min(16 * q + 16, b * L)) for q in range(sh, n_g, shards)] or
                         [torch.zeros(0, dtype=torch.long)])
        torch.testing.assert_close(stat[sh, :, 0], d[:, cols].sum(1), **TOL)


def _fc_case(g, b, C, L):
    U = (torch.randn(b, C, L, generator=g, dtype=F64) * 1.5 + 0.3).float()
    mean = U.double().mean(dim=(0, 2))
    rstd = 1.0 / torch.sqrt(U.double().var(dim=(0, 2), unbiased=False) + 1e-5)
    bn_w = (1.0 + 0.3 * torch.randn(C, generator=g, dtype=F64)).float()
    bn_b = (0.2 * torch.randn(C, generator=g, dtype=F64)).float()
    return U, mean, rstd, bn_w, bn_b


def test_clear_fc_relu_reaches_the_margin_at_the_largest_gpu_shape():
    """b 129, C 1024, L 16: 2064 elements per channel, about one within 1e-3 of any given bias — every channel has to be
    looked at, most of them placed in a gap"""
    g = _gen(600)
    U, mean, rstd, bn_w, bn_b = _fc_case(g, 129, 1024, 16)
    out, margin = mr.clear_fc_relu(g, U, mean, rstd, bn_w, bn_b)
    assert out.dtype == torch.float32 and out.shape == bn_b.shape
    assert margin >= mr.RELU_MARGIN, margin
    scale = (bn_w.double() * rstd).float()
    shift = (out.double() - mean * scale.double()).float()
    assert mr.fc_margin(U, scale, shift) >= mr.RELU_MARGIN         # and with chan rounded to float32 as a case gives it
    assert float(out.abs().max()) <= 1.0


def test_clear_fc_relu_leaves_clear_channels_alone_and_reports_the_margin():
    g = _gen(601)
    U, mean, rstd, bn_w, bn_b = _fc_case(g, 2, 8, 4)
    t = (U.double() - mean[None, :, None]) * (bn_w.double() * rstd)[None, :, None]
    bn_b[3] = float(-t[1, 3, 2]) + 1e-4                            # channel 3: one vf at 1e-4
    before = bn_b.clone()
    out, margin = mr.clear_fc_relu(g, U, mean, rstd, bn_w, bn_b)
    keep = [c for c in range(8) if c != 3 and float((t[:, c] + before[c].double()).abs().min()) >= 2e-3]
    assert keep and torch.equal(out[keep], before[keep]) and float(out[3]) != float(before[3])
    assert margin >= mr.RELU_MARGIN
    assert abs(margin - float((t + out.double()[None, :, None]).abs().min())) < 1e-15
