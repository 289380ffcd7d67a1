"""CPU self-check of tests/bn_ref.py: the float64 statement tests/test_bn_kernels_gpu.py holds the BatchNorm kernels to
is pinned here against torch in float64 — nn.BatchNorm1d (training: two consecutive steps for the running statistics
and the counters; eval), F.batch_norm under autograd for every gradient, F.glu, F.mish, relu and a given dropout mask.
A GPU mismatch is then the kernel's."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as br

TOL = 1e-12                                                        # float64 against float64, of the tensor's scale


def _close(name, got, want, rel=TOL):
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-300)
    err = float((got - want).abs().max())
    assert err <= rel * scale, f'{name}: {err:.3e} of scale {scale:.3e}'


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _rand(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float64)


def _problem(b, M, L, seed):
    g = _gen(seed + 7 * b + 3 * M + L)
    U = _rand(g, b, M, L) * (0.5 + _rand(g, M).abs())[None, :, None] + 2.0 * _rand(g, M)[None, :, None]
    return g, U, _rand(g, M), 1.0 + 0.3 * _rand(g, M), 0.5 * _rand(g, M), _rand(g, M), 0.5 + _rand(g, M).abs()


def _module(M, bn_w, bn_b, rm, rv, nbt):
    bn = torch.nn.BatchNorm1d(M).double()
    bn.load_state_dict({'weight': bn_w, 'bias': bn_b, 'running_mean': rm, 'running_var': rv,
                        'num_batches_tracked': torch.tensor(nbt)})
    return bn


def _check_step(r, U, bn, M):
    """r: one step of bn_ref; bn: the module before that step (training)"""
    y = bn(U)
    c = r['chan']
    _close('out', br.affine(U, c[2 * M:3 * M], c[3 * M:]), y)
    _close('mean', c[:M], U.mean(dim=(0, 2)))
    _close('rstd', c[M:2 * M], 1.0 / torch.sqrt(U.var(dim=(0, 2), unbiased=False) + 1e-5))
    _close('running_mean', r['rm'], bn.running_mean)
    _close('running_var', r['rv'], bn.running_var)
    assert int(r['nbt'][0]) == int(bn.num_batches_tracked) and int(r['nbt'][1]) == int(bn.num_batches_tracked) + 2 ** 33


SHAPES = [(1, 4, 4), (3, 8, 8), (5, 12, 4), (2, 16, 16), (19, 5, 16), (4, 3, 4)]


@pytest.mark.parametrize('shards', [1, 3, 4])
@pytest.mark.parametrize('bias', [True, False])
@pytest.mark.parametrize('b,M,L', SHAPES)
def test_finalisation_from_sums_is_batchnorm1d_over_two_steps(b, M, L, bias, shards):
    g, U, cb, bn_w, bn_b, rm, rv = _problem(b, M, L, 100 + shards)
    cbv = cb if bias else None
    bn = _module(M, bn_w, bn_b, rm, rv, 7).train()
    nbt = torch.tensor([7, 2 ** 33 + 7])
    r = br.fin_from_sums(br.sums_of(U, cbv, shards), cbv, bn_w, bn_b, rm, rv, nbt, b * L)
    _check_step(r, U, bn, M)
    U2 = U * 0.7 + _rand(g, b, M, L)
    r2 = br.fin_from_sums(br.sums_of(U2, cbv, shards), cbv, bn_w, bn_b, r['rm'], r['rv'], r['nbt'], b * L)
    _check_step(r2, U2, bn, M)
    assert int(r2['nbt'][0]) == 9
    none = br.fin_from_sums(br.sums_of(U, cbv, shards), cbv, bn_w, bn_b, None, None, None, b * L)
    assert none['rm'] is None and none['rv'] is None and none['nbt'] is None
    _close('chan without running statistics', none['chan'], r['chan'])


def test_finalisation_from_sums_clamps_a_negative_variance():
    stat = torch.tensor([[[8.0, 15.9]]], dtype=torch.float64)              # E d^2 - (E d)^2 = 3.975 - 4 < 0
    r = br.fin_from_sums(stat, None, torch.ones(1), torch.zeros(1), None, None, None, 4)
    _close('rstd', r['chan'][1:2], torch.tensor([1e-5], dtype=torch.float64) ** -0.5)


@pytest.mark.parametrize('b,M,L', SHAPES + [(17, 3, 16), (1, 1, 2)])
def test_finalisation_from_partials_is_batchnorm1d_over_two_steps(b, M, L):
    g, U, _, bn_w, bn_b, rm, rv = _problem(b, M, L, 200)
    U = U + 30.0                                                     # Chan's rule: no cancellation to hide behind
    bn = _module(M, bn_w, bn_b, rm, rv, 7).train()
    nbt = torch.tensor([7, 2 ** 33 + 7])
    r = br.fin_from_partials(br.group_partials(U), bn_w, bn_b, rm, rv, nbt, b * L)
    _check_step(r, U, bn, M)
    U2 = U * 0.7 + _rand(g, b, M, L)
    r2 = br.fin_from_partials(br.group_partials(U2), bn_w, bn_b, r['rm'], r['rv'], r['nbt'], b * L)
    _check_step(r2, U2, bn, M)
    assert br.partial_counts(b * L, (b * L + 15) // 16)[-1] == (b * L - 1) % 16 + 1


@pytest.mark.parametrize('how', ['sums', 'partials'])
def test_eval_mode_reads_the_running_statistics_and_changes_nothing(how):
    b, M, L = 3, 8, 8
    g, U, cb, bn_w, bn_b, rm, rv = _problem(b, M, L, 300)
    bn = _module(M, bn_w, bn_b, rm, rv, 7).eval()
    nbt = torch.tensor([7])
    if how == 'sums':
        r = br.fin_from_sums(None, cb, bn_w, bn_b, rm, rv, nbt, b * L, training=False)
    else:
        r = br.fin_from_partials(None, bn_w, bn_b, rm, rv, nbt, b * L, training=False)
    _close('out', br.affine(U, r['chan'][2 * M:3 * M], r['chan'][3 * M:]), bn(U))
    assert torch.equal(r['rm'], rm) and torch.equal(r['rv'], rv) and int(r['nbt'][0]) == 7


def _tail_torch(kind, v, mask):
    if kind == 'glu':
        o = F.glu(v, dim=1)
    else:
        o = torch.relu(v) if kind == 'relu' else F.mish(v)
    return o * mask.reshape(o.shape)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('kind', ['relu', 'mish', 'glu'])
@pytest.mark.parametrize('b,M,L', [(1, 4, 4), (3, 8, 8), (5, 12, 16)])
def test_tails_and_phase_b_are_autograd_of_batch_norm(b, M, L, kind, training):
    g, U, _, bn_w, bn_b, rm, rv = _problem(b, M, L, 400)
    U = U * 6.0                                                      # mish / sigmoid arguments on both sides of +-20
    Mo = M // 2 if kind == 'glu' else M
    mask = (torch.rand(b * Mo * L, generator=g) >= 0.3).double() / 0.7
    gout = _rand(g, b, Mo, L)
    prev = _rand(g, 2 * M)
    Ur, w, bb = U.clone().requires_grad_(True), bn_w.clone().requires_grad_(True), bn_b.clone().requires_grad_(True)
    v = F.batch_norm(Ur, None if training else rm.clone(), None if training else rv.clone(), w, bb, training, 0.1, 1e-5)
    v.retain_grad()
    out = _tail_torch(kind, v, mask)
    (out * gout).sum().backward()
    if training:
        chan = br.fin_from_sums(br.sums_of(U, None, 2), None, bn_w, bn_b, None, None, None, b * L)['chan']
    else:
        chan = br.bn_eval_chan(bn_w, bn_b, rm, rv)
    _close('out', br.tail_fwd(kind, U, chan[2 * M:3 * M], chan[3 * M:], mask), out.detach())
    dV, bn_grad = br.tail_bwd(kind, gout, U, chan, mask, prev)
    _close('dV', dV, v.grad)
    _close('bn_grad: weight', bn_grad[:M] - prev[:M], w.grad)
    _close('bn_grad: bias', bn_grad[M:] - prev[M:], bb.grad)
    _close('dU', br.phase_b(dV, U, chan, bn_grad - prev, training), Ur.grad)
    if training:
        dU, chan2, grad2 = br.bn_input_grad(dV, U, bn_w)
        _close('attention_ref.bn_input_grad: dU', dU, Ur.grad)
        _close('attention_ref.bn_input_grad: chan', chan2[:3 * M], chan[:3 * M])
        _close('attention_ref.bn_input_grad: bn_grad', grad2, bn_grad - prev)
    else:
        nan = torch.full_like(U, float('nan'))
        assert torch.equal(br.phase_b(dV, nan, chan, torch.full((2 * M,), float('nan')), False),
                           br.phase_b(dV, U, chan, bn_grad, False))


def test_relu_gradient_at_zero_is_zero_and_mish_is_exact_far_out():
    U = torch.zeros(1, 4, 4, dtype=torch.float64)
    chan = torch.cat([torch.zeros(4), torch.ones(4), torch.ones(4), torch.zeros(4)]).double()
    dV, bn_grad = br.tail_bwd('relu', torch.ones(1, 4, 4), U, chan)
    assert not dV.any() and not bn_grad.any()
    v = torch.tensor([-700.0, -30.0, -20.0, 0.0, 19.9, 20.1, 30.0, 700.0], dtype=torch.float64)
    _close('mish', br.mish(v), F.mish(v))
    assert torch.isfinite(br.dmish(v)).all() and float(br.dmish(v)[-1]) == 1.0 and abs(float(br.mish(v)[0])) < 1e-290
