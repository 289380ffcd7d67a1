"""CPU: tests/crit_ref.py (the float64 formulas the weighted criterion kernels are tested against)
equals torch.nn.functional with autograd in float64, over the full option grid."""
import itertools

import pytest
import torch
import torch.nn.functional as F

import crit_ref

TOL = 1e-9          # float64 against float64: two evaluation orders of the same formula


def _close(name, got, want):
    if torch.isnan(want).any():
        assert torch.equal(torch.isnan(got), torch.isnan(want)), name
        got, want = torch.nan_to_num(got), torch.nan_to_num(want)
    scale = max(1.0, float(want.abs().max()))
    assert float((got - want).abs().max()) <= TOL * scale, (name, float((got - want).abs().max()))


@pytest.mark.parametrize('use_w,use_p,reduction', list(itertools.product((False, True), (False, True), ('mean', 'sum'))))
def test_bce_formulas_equal_torch(use_w, use_p, reduction):
    g = torch.Generator().manual_seed(5)
    b, O = 7, 23
    z = (4 * torch.randn(b, O, generator=g, dtype=torch.float64)).requires_grad_(True)
    y = (torch.rand(b, O, generator=g) < 0.3).double()
    w = (0.25 + 2 * torch.rand(O, generator=g, dtype=torch.float64)) if use_w else None
    p = (0.25 + 4 * torch.rand(O, generator=g, dtype=torch.float64)) if use_p else None
    want = F.binary_cross_entropy_with_logits(z, y, weight=w, pos_weight=p, reduction=reduction)
    (dwant,) = torch.autograd.grad(want, z)
    loss, dz = crit_ref.bce(z, y, w, p, reduction)
    _close('loss', loss, want.detach())
    _close('dz', dz, dwant)


def test_bce_extreme_logits_are_finite():
    """the worked example of the design note: fp32 z = (80, -80, 0), y = (0, 1, 1), pos_weight = (2, 3, .5)"""
    z = torch.tensor([[80.0, -80.0, 0.0]])
    y = torch.tensor([[0.0, 1.0, 1.0]])
    p = torch.tensor([2.0, 3.0, 0.5])
    loss, dz = crit_ref.bce(z, y, None, p, 'sum')
    want = F.binary_cross_entropy_with_logits(z.double(), y.double(), pos_weight=p.double(), reduction='none')
    assert torch.isfinite(dz).all()
    _close('terms', want, torch.tensor([[80.0, 240.0, 0.5 * 0.6931471805599453]], dtype=torch.float64))
    _close('loss', loss, want.sum())


@pytest.mark.parametrize('use_w,reduction,eps,ignored', list(itertools.product(
    (False, True), ('mean', 'sum'), (0.0, 0.1), ('none', 'some', 'all'))))
def test_ce_formulas_equal_torch(use_w, reduction, eps, ignored):
    g = torch.Generator().manual_seed(9)
    b, O, ign = 9, 11, 4
    z = (3 * torch.randn(b, O, generator=g, dtype=torch.float64)).requires_grad_(True)
    y = torch.randint(0, O, (b,), generator=g)
    y[y == ign] = ign + 1
    if ignored == 'some':
        y[[1, 5, 8]] = ign
    elif ignored == 'all':
        y[:] = ign
    w = (0.25 + 2 * torch.rand(O, generator=g, dtype=torch.float64)) if use_w else None
    want = F.cross_entropy(z, y, weight=w, ignore_index=ign, reduction=reduction, label_smoothing=eps)
    (dwant,) = torch.autograd.grad(want, z)
    loss, dz = crit_ref.ce(z, y, w, eps, ign, reduction)
    _close('loss', loss, want.detach())
    _close('dz', dz, torch.nan_to_num(dwant) if ignored == 'all' else dwant)
    if ignored != 'none':
        assert float(dz[y == ign].abs().max()) == 0.0
    if ignored == 'all' and reduction == 'mean':
        assert torch.isnan(loss) and float(dz.abs().max()) == 0.0


def test_ce_negative_ignore_index_is_never_an_index():
    z = torch.randn(4, 5, dtype=torch.float64)
    y = torch.tensor([0, -100, 3, -100])
    loss, dz = crit_ref.ce(z, y, None, 0.1, -100, 'mean')
    want = F.cross_entropy(z, y, label_smoothing=0.1)
    _close('loss', loss, want)
    assert float(dz[1].abs().max()) == 0.0 and float(dz[3].abs().max()) == 0.0
