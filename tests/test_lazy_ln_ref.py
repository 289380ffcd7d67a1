"""CPU self-check of tests/lazy_ln_ref.py: the hand-written float64 formulas tests/test_lazy_ln_kernels_gpu.py holds
the streaming-LayerNorm kernels to are pinned here against torch (F.layer_norm, F.linear, the two criteria, autograd),
and combine(records(x)) against the direct moments — for the offset inputs too.  A GPU mismatch is then the kernel's."""
import pytest
import torch
import torch.nn.functional as F

import lazy_ln_ref as lr

SHAPES = [(16, 4), (128, 8), (68, 16), (192, 16), (256, 16)]       # the GPU test's (C, L)
TOL = 1e-11                                                        # float64 against float64, of the tensor's scale


def _close(name, got, want, rel=TOL):
    got, want = got.double(), want.double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= rel * scale, f'{name}: {err:.3e} of scale {scale:.3e}'


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _affine(g, *shape):
    return (torch.randn(*shape, generator=g) * 0.3 + 1.0).double(), (torch.randn(*shape, generator=g) * 0.2).double()


@pytest.mark.parametrize('offset', [False, True])
@pytest.mark.parametrize('C,L', SHAPES)
def test_records_combine_to_the_direct_moments(C, L, offset):
    g = _gen(100 + C + L)
    b = 3
    pre = (lr.offset_resid(g, b, C, L) if offset else torch.randn(b, C, L, generator=g) * 1.5 + 0.2).double()
    w, bias = _affine(g, C, L)
    rec, prm = lr.records(pre, w, bias)
    P = lr.n_parts(C * L)
    assert rec.shape == (b, P, 8) and prm.shape == (P, 8)
    assert float(prm[:, 5].sum()) == C * L and float(prm[-1, 5]) == C * L - (P - 1) * lr.PART
    assert float(rec[:, :, 6:].abs().max()) == 0.0 and float(prm[:, 6:].abs().max()) == 0.0
    mean, rstd, osum, osq = lr.combine(rec, prm)
    n, m_d, r_d, xhat = lr.node_ln(pre, w, bias)
    # (rstd: M2 / D is a difference of nothing — centred sums — so 1e-11 holds with the +-20 part shifts as well)
    _close('mean', mean, m_d)
    _close('rstd', rstd, r_d)
    sums = lr.out_sums(n)
    _close('S(o)', osum, sums[:, 0], rel=1e-10)
    _close('S(o^2)', osq, sums[:, 1], rel=1e-10)
    if offset and P >= 2:                                          # the part means really lie far from each other
        assert float((rec[:, 0, 0] - rec[:, 1, 0]).min()) > 35.0
    # centre = the part means given explicitly: the same records
    rec2, _ = lr.records(pre, w, bias, centre=rec[:, :, 0])
    assert torch.equal(rec2, rec)


@pytest.mark.parametrize('C,L', SHAPES)
def test_node_layernorm_and_its_backward_match_autograd(C, L):
    g = _gen(200 + C + L)
    b = 4
    pre = (torch.randn(b, C, L, generator=g) * 1.5 + 0.2).double().requires_grad_(True)
    w, bias = _affine(g, C, L)
    gy = torch.randn(b, C, L, generator=g).double()
    want = F.layer_norm(pre, (C, L), w, bias, lr.EPS)
    n, mean, rstd, xhat = lr.node_ln(pre.detach(), w, bias)
    _close('n', n, want.detach())
    want_g, = torch.autograd.grad(want, pre, gy)
    for group in (lr.PART, lr.GROUP):                              # the partials of either layout sum to the whole
        part = lr.ln_partials(gy, w, xhat, group)
        assert part.shape == (b, (C * L + group - 1) // group, 2)
        _close(f'g_in (groups of {group})', lr.node_ln_bwd(gy, w, xhat, rstd, part.sum(1)), want_g)


@pytest.mark.parametrize('mode', ['given', 'bce', 'ce'])
@pytest.mark.parametrize('C,L,n_src,O,b', [(16, 4, 1, 5, 3), (68, 16, 2, 23, 5), (128, 8, 3, 60, 4)])
def test_head_matches_autograd(C, L, n_src, O, b, mode):
    g = _gen(300 + C + O)
    ns = [(torch.randn(b, C, L, generator=g) * 0.8 + 0.1 * q).double().requires_grad_(True) for q in range(n_src)]
    D = n_src * C * L
    w, bias_ln = _affine(g, n_src * C, L)
    w.requires_grad_(True)
    bias_ln = lr.clear_relu_bias(g, [n.detach() for n in ns], w.detach(), bias_ln).requires_grad_(True)
    W = (torch.randn(O, D, generator=g) / D ** 0.5).double().requires_grad_(True)
    bias = (torch.randn(O, generator=g) * 0.1).double().requires_grad_(True)
    feat = F.relu(F.layer_norm(torch.cat(ns, dim=1), (n_src * C, L), w, bias_ln, lr.EPS))
    logits = F.linear(feat.reshape(b, -1), W, bias)
    fw = lr.head_fwd([n.detach() for n in ns], w.detach(), bias_ln.detach(), W.detach(), bias.detach())
    lr.assert_relu_clear(fw)
    _close('logits', fw['logits'], logits.detach())
    if mode == 'given':
        dl = torch.randn(b, O, generator=g).double()
        loss_t = (logits * dl).sum()
    elif mode == 'bce':
        y = (torch.rand(b, O, generator=g) < 0.3).double()
        loss_t = F.binary_cross_entropy_with_logits(logits, y)
        loss, dl = lr.bce_logits(fw['logits'], y)
        _close('bce', loss, loss_t.detach())
    else:
        lab = torch.randint(0, O, (b,), generator=g)
        loss_t = F.cross_entropy(logits, lab)
        loss, dl = lr.cross_entropy(fw['logits'], lab)
        _close('ce', loss, loss_t.detach())
    grads = torch.autograd.grad(loss_t, ns + [W, bias, w, bias_ln])
    bw = lr.head_bwd(fw, w.detach(), W.detach(), dl)
    for q in range(n_src):
        _close(f'dn[{q}]', bw['dn'][q], grads[q], rel=1e-10)
    _close('dW', bw['dW'], grads[n_src], rel=1e-10)
    _close('dbias', bw['dbias'], grads[n_src + 1], rel=1e-10)
    _close('dln_w', bw['dln_w'], grads[n_src + 2].reshape(-1), rel=1e-10)
    _close('dln_b', bw['dln_b'], grads[n_src + 3].reshape(-1), rel=1e-10)
    # A, B are what the backward's two LayerNorm means are made of: m1 = dl . A / D, m2 = dl . B / D
    gw = ((dl @ W.detach()) * fw['mask']) * w.detach().reshape(-1)
    _close('dl . A', (dl * fw['A']).sum(1), gw.sum(1), rel=1e-10)
    _close('dl . B', (dl * fw['B']).sum(1), (gw * fw['xhat']).sum(1), rel=1e-10)


def test_relu_margin_is_enforced():
    g = _gen(7)
    n = torch.randn(2, 16, 4, generator=g).double()
    w, bias_ln = _affine(g, 16, 4)
    fw = lr.head_fwd([n], w, bias_ln, torch.zeros(3, 64).double(), torch.zeros(3).double())
    k = 5
    bias_ln = bias_ln.reshape(-1).clone()
    bias_ln[k] -= fw['arg'][1, k] - 1e-4                          # one argument 1e-4 from zero
    fw = lr.head_fwd([n], w, bias_ln, torch.zeros(3, 64).double(), torch.zeros(3).double())
    with pytest.raises(AssertionError):
        lr.assert_relu_clear(fw)
    fixed = lr.clear_relu_bias(g, [n], w, bias_ln)
    lr.assert_relu_clear(lr.head_fwd([n], w, fixed, torch.zeros(3, 64).double(), torch.zeros(3).double()))


def test_gate_accepts_the_documented_lengths_only():
    """bmnas_lazy_ln_ok is host code: L in {4, 8, 16} and C L <= 4096, as include/bmnas_hip.h says — the backward half
    of the family (bmnas_node_mix_lnp_bwd) takes no other L, so the forward half must not either."""
    from bmnas import lib
    for L in range(0, 21):
        assert lib.lazy_ln_ok(16, L) == (L in (4, 8, 16)), L
    assert lib.lazy_ln_ok(256, 16) and not lib.lazy_ln_ok(260, 16) and not lib.lazy_ln_ok(257, 16)
    assert lib.lazy_ln_ok(1024, 4) and not lib.lazy_ln_ok(1025, 4) and not lib.lazy_ln_ok(0, 4)
    assert [lib.lazy_ln_parts(C, L) for C, L in SHAPES] == [lr.n_parts(C * L) for C, L in SHAPES] == [1, 1, 2, 3, 4]
