"""tests/clip_ref.py (the float64 restatement the GPU clipping tests can be read against) pinned to torch itself:
torch.nn.utils.clip_grad_norm_ followed by torch.optim.Adam on the CPU in float64 — norm, coefficient, the order of
clipping and weight decay, a parameter without a gradient, and the NaN rule."""
import math

import numpy as np
import pytest
import torch

import clip_ref

SHAPES = [(7, 5), (33,), (1,), (4, 3, 2)]


def _make(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return [scale * torch.randn(*s, generator=g, dtype=torch.float64) for s in SHAPES]


@pytest.mark.parametrize('max_norm', [0.5, 5.0, 1e6])
def test_norm_and_clipped_gradients_equal_torchs(max_norm):
    ps = [t.requires_grad_(True) for t in _make(1)]
    grads = _make(2, 3.0)
    grads[2] = None                                          # left out of the norm, as torch leaves it out
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.clone()
    norm_t = torch.nn.utils.clip_grad_norm_(ps, max_norm)
    got, norm = clip_ref.clip(grads, max_norm)
    assert abs(norm - float(norm_t)) <= 1e-14 * norm
    assert got[2] is None and ps[2].grad is None
    for p, g in zip(ps, got):
        if g is not None:
            assert np.abs(g - p.grad.numpy()).max() <= 1e-14 * np.abs(g).max()
    assert (clip_ref.clip_coef(norm, max_norm) < 1.0) == (max_norm < norm)


def test_coefficient_rules():
    assert clip_ref.clip_coef(0.0, 5.0) == 1.0                # all-zero gradients: 5 / 1e-6 clamps to 1
    assert clip_ref.clip_coef(10.0, 5.0) == 5.0 / (10.0 + 1e-6)
    assert clip_ref.clip_coef(float('inf'), 5.0) == 0.0
    assert math.isnan(clip_ref.clip_coef(float('nan'), 5.0))
    # ... which is what torch.clamp does, and not what a min() would do
    assert math.isnan(float(torch.clamp(torch.tensor(float('nan')), max=1.0)))


@pytest.mark.parametrize('wd', [1e-2, 0.0])
def test_clipped_adam_steps_equal_torchs(wd):
    """Six steps, one tensor joining at step 2 (its own step count), a moving learning rate; weight decay large enough
    that clipping AFTER the wd * p term would show at 1e-3."""
    ps = [t.requires_grad_(True) for t in _make(3)]
    opt = torch.optim.Adam(ps, lr=1e-2, betas=(0.5, 0.999), weight_decay=wd)
    P = [p.detach().numpy().copy() for p in ps]
    M = [np.zeros_like(p) for p in P]
    V = [np.zeros_like(p) for p in P]
    T = [0] * len(P)
    for step in range(6):
        grads = _make(10 + step, 4.0)
        if step < 2:
            grads[1] = None
        lr = 1e-2 * 0.9 ** step
        for g in opt.param_groups:
            g['lr'] = lr
        for p, g in zip(ps, grads):
            p.grad = None if g is None else g.clone()
        norm_t = torch.nn.utils.clip_grad_norm_(ps, 5.0)
        opt.step()
        P, M, V, T, norm = clip_ref.clipped_adam_step(P, grads, M, V, T, lr, 5.0, betas=(0.5, 0.999), wds=wd)
        assert abs(norm - float(norm_t)) <= 1e-14 * norm and norm > 5.0
    assert T == [6, 4, 6, 6]
    for p, want, m, v in zip(ps, P, M, V):
        st = opt.state[p]
        assert np.abs(p.detach().numpy() - want).max() <= 1e-12
        assert np.abs(st['exp_avg'].numpy() - m).max() <= 1e-12 * max(1.0, np.abs(m).max())
        assert np.abs(st['exp_avg_sq'].numpy() - v).max() <= 1e-12 * max(1.0, np.abs(v).max())
    if wd:
        # the order matters at this weight decay: scaling (grad + wd * p) instead leaves other moments (the first
        # update itself is lr * sign(g) either way)
        p0 = _make(3)[0].numpy()
        g0 = _make(10, 4.0)
        g0[1] = None
        c = clip_ref.clip_coef(clip_ref.grad_norm(g0), 5.0)
        _, wrong, _ = clip_ref.adam_step(p0, c * (g0[0].numpy() + wd * p0), 0 * p0, 0 * p0, 1, 1e-2, (0.5, 0.999))
        _, right, _ = clip_ref.adam_step(p0, c * g0[0].numpy(), 0 * p0, 0 * p0, 1, 1e-2, (0.5, 0.999), wd=wd)
        assert np.abs(wrong - right).max() > 1e-3


def test_a_nan_gradient_makes_every_parameter_nan_as_with_torch():
    ps = [t.requires_grad_(True) for t in _make(4)]
    grads = _make(5)
    grads[3][1, 2, 0] = float('nan')
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    opt = torch.optim.Adam(ps, lr=1e-2)
    norm_t = torch.nn.utils.clip_grad_norm_(ps, 5.0)
    opt.step()
    P, _, _, _, norm = clip_ref.clipped_adam_step([p.detach().numpy() for p in _make(4)], grads,
                                                  [0 * g.numpy() for g in grads], [0 * g.numpy() for g in grads], 0,
                                                  1e-2, 5.0)
    assert math.isnan(norm) and math.isnan(float(norm_t))
    for p, want in zip(ps, P):
        assert bool(torch.isnan(p.detach()).all()) and np.isnan(want).all()
