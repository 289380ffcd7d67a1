"""tests/adam_ref.py (the float64 restatement the Adam-variant GPU tests are read against) pinned to torch itself on the
CPU in float64: torch.optim.Adam(amsgrad=..., decoupled_weight_decay=...) and torch.optim.AdamW, with and without a
preceding torch.nn.utils.clip_grad_norm_, a tensor joining late, a moving learning rate, and a NaN gradient element."""
import numpy as np
import pytest
import torch

import adam_ref

SHAPES = [(7, 5), (33,), (1,), (4, 3, 2)]
MULT = [10, 10, 1, 0.1, 0.1, 1]                 # the second moment must FALL for the running maximum to differ from it


def _make(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]


def _torch_opt(ps, amsgrad, decoupled, wd, adamw):
    if adamw:
        return torch.optim.AdamW(ps, lr=1e-2, betas=(0.9, 0.9), weight_decay=wd, amsgrad=amsgrad)
    return torch.optim.Adam(ps, lr=1e-2, betas=(0.9, 0.9), weight_decay=wd, amsgrad=amsgrad,
                            decoupled_weight_decay=decoupled)


def _run(amsgrad, decoupled, wd, max_norm, adamw=False, nan_at=None):
    ps = [t.requires_grad_(True) for t in _make(3)]
    opt = _torch_opt(ps, amsgrad, decoupled, wd, adamw)
    ref = adam_ref.Ref([p.detach().numpy() for p in ps], betas=(0.9, 0.9), amsgrad=amsgrad, decoupled=decoupled,
                       max_norm=max_norm)
    for step in range(6):
        grads = _make(10 + step, MULT[step])
        if step < 2:
            grads[1] = None
        if nan_at == step:
            grads[0][2, 3] = float('nan')
        lr = 1e-2 * 0.9 ** step
        for g in opt.param_groups:
            g['lr'] = lr
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(ps, max_norm)
        opt.step()
        ref.step(grads, lr, wd)
    return ps, opt, ref


def _same(a, b, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    assert (np.isnan(a) == np.isnan(b)).all()
    ok = ~np.isnan(a)
    if ok.any():
        assert np.abs(a[ok] - b[ok]).max() <= tol * max(1.0, np.abs(b[ok]).max())


@pytest.mark.parametrize('max_norm', [None, 5.0], ids=['unclipped', 'clipped'])
@pytest.mark.parametrize('amsgrad,decoupled', [(False, False), (True, False), (False, True), (True, True)])
def test_six_steps_equal_torchs(amsgrad, decoupled, max_norm):
    ps, opt, ref = _run(amsgrad, decoupled, 0.1, max_norm)
    assert ref.T == [6, 4, 6, 6]
    for i, p in enumerate(ps):
        st = opt.state[p]
        _same(p.detach().numpy(), ref.P[i])
        _same(st['exp_avg'].numpy(), ref.M[i])
        _same(st['exp_avg_sq'].numpy(), ref.V[i])
        assert ('max_exp_avg_sq' in st) == amsgrad
        if amsgrad:
            _same(st['max_exp_avg_sq'].numpy(), ref.X[i])
    if amsgrad and max_norm is None:
        # the inputs do exercise the maximum: on the largest tensor it lies above the moment nearly everywhere (clipping
        # to a fixed norm takes the multipliers out again: there the maximum differs less often)
        assert float((ref.X[0] > ref.V[0]).mean()) > 0.9


@pytest.mark.parametrize('amsgrad', [False, True])
def test_adamw_is_adam_with_the_decoupled_switch(amsgrad):
    ps, opt, ref = _run(amsgrad, True, 0.1, None, adamw=True)
    assert all(g['decoupled_weight_decay'] is True for g in opt.param_groups)
    for i, p in enumerate(ps):
        _same(p.detach().numpy(), ref.P[i])
    # ... and the switch matters at this weight decay
    other = _run(amsgrad, False, 0.1, None)[2]
    assert max(np.abs(a - b).max() for a, b in zip(ref.P, other.P)) > 1e-3


@pytest.mark.parametrize('amsgrad,decoupled', [(False, False), (True, False), (False, True), (True, True)])
def test_a_nan_gradient_element_stays_in_its_element(amsgrad, decoupled):
    """Without clipping one NaN gradient element poisons that element alone — moments, running maximum (torch.maximum
    propagates NaN) and parameter — and it never recovers."""
    ps, opt, ref = _run(amsgrad, decoupled, 0.1, None, nan_at=1)
    for i, p in enumerate(ps):
        st = opt.state[p]
        _same(p.detach().numpy(), ref.P[i])
        _same(st['exp_avg_sq'].numpy(), ref.V[i])
        if amsgrad:
            _same(st['max_exp_avg_sq'].numpy(), ref.X[i])
    bad = np.isnan(ref.P[0])
    assert bad.sum() == 1 and bad[2, 3] and not any(np.isnan(p).any() for p in ref.P[1:])
    assert np.isnan(ref.V[0][2, 3]) and (not amsgrad or np.isnan(ref.X[0][2, 3]))


def test_a_nan_gradient_with_clipping_reaches_every_parameter():
    ps, opt, ref = _run(True, True, 0.1, 5.0, nan_at=1)
    for i, p in enumerate(ps):
        _same(p.detach().numpy(), ref.P[i])
        if ref.T[i] == 6:
            assert np.isnan(ref.P[i]).all() and np.isnan(ref.X[i]).all()


def test_maximum_propagates_nan_unlike_fmax():
    a, b = np.array([1.0, np.nan, 2.0]), np.array([np.nan, 1.0, 3.0])
    got = adam_ref.maximum(a, b)
    assert np.isnan(got[:2]).all() and got[2] == 3.0
    assert torch.isnan(torch.maximum(torch.from_numpy(a), torch.from_numpy(b))[:2]).all()
