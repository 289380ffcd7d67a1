"""The eager weighted / smoothed criterion kernels (csrc/linear.hip: bmnas_bce_logits_crit,
bmnas_cross_entropy_crit) through the C ABI against the float64 formulas of tests/crit_ref.py
(pinned against torch on the CPU by tests/test_crit_ref.py).  Bounds: assert_close_scaled's
defaults.  Every output starts as NaN: an element a kernel never writes fails its comparison.

Shapes: BCE (rows, O) from one element to more elements than the workgroup's 1024 threads, O = 128
the widest class count; CE (b, O) with O < 64 (idle lanes), O > 64 (a second lane stride), b = 256 /
257 the boundary between the one-launch and the two-launch form, and (300, 120)."""
import ctypes

import pytest
import torch

import crit_ref
from gpu_util import assert_close_scaled, dev

pytestmark = pytest.mark.gpu

BCE_SHAPES = [(1, 1), (5, 23), (37, 23), (3, 128), (128, 23)]
CE_SHAPES = [(1, 2), (6, 83), (7, 60), (256, 60), (257, 60), (300, 120)]
BCE_OPTS = [  # weight, pos_weight, reduction
    (False, True, 'mean'), (True, False, 'mean'), (True, True, 'sum'), (False, False, 'sum'), (False, False, 'mean')]
CE_OPTS = [   # weight, label_smoothing, ignore ('none' | 'some' | 'neg'), reduction
    (True, 0.0, 'none', 'mean'), (False, 0.1, 'none', 'mean'), (True, 0.1, 'some', 'mean'), (True, 0.1, 'some', 'sum'),
    (False, 0.0, 'neg', 'mean'), (True, 0.0, 'neg', 'sum'), (False, 0.0, 'none', 'sum')]


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _nan(*shape):
    return torch.full(shape, float('nan'), device=dev())


def _weights(g, O, on):
    return (0.25 + 2.0 * torch.rand(O, generator=g)) if on else None


def _to(t):
    return None if t is None else t.to(dev())


def _run_bce(z, y, w, p, reduction, want_dz=True):
    from bmnas import lib
    keep = (_to(z), _to(y), _to(w), _to(p))
    crit = lib.Criterion('bce', weight=keep[2], pos_weight=keep[3], reduction=reduction)
    loss, dz = _nan(1), (_nan(*z.shape) if want_dz else None)
    lib.bce_logits_crit(keep[0], keep[1], crit, loss, dz, z.numel() // z.shape[-1], z.shape[-1])
    torch.cuda.synchronize()
    return loss, dz


def _run_ce(z, y, w, eps, ignore_index, reduction, want_dz=True):
    from bmnas import lib
    keep = (_to(z), _to(y), _to(w))
    crit = lib.Criterion('ce', weight=keep[2], label_smoothing=eps, ignore_index=ignore_index, reduction=reduction)
    b, O = z.shape
    loss, dz, rows = _nan(1), (_nan(b, O) if want_dz else None), _nan(b)
    lib.cross_entropy_crit(keep[0], keep[1], crit, loss, dz, rows, b, O)
    torch.cuda.synchronize()
    return loss, dz


@pytest.mark.parametrize('rows,O', BCE_SHAPES)
def test_bce_every_option(rows, O):
    g = _gen(100 + rows + O)
    z = 3.0 * torch.randn(rows, O, generator=g)
    y = (torch.rand(rows, O, generator=g) < 0.3).float()
    for use_w, use_p, reduction in BCE_OPTS:
        w, p = _weights(g, O, use_w), _weights(g, O, use_p)
        want, dwant = crit_ref.bce(z, y, w, p, reduction)
        name = f'w={use_w} p={use_p} {reduction}'
        loss, dz = _run_bce(z, y, w, p, reduction)
        assert_close_scaled('loss ' + name, loss, want.reshape(1))
        assert_close_scaled('dz ' + name, dz, dwant)
        loss2, _ = _run_bce(z, y, w, p, reduction, want_dz=False)         # dz == NULL: the loss alone
        assert torch.equal(loss, loss2)


def test_bce_leading_dimensions_and_extreme_logits():
    """(…, O): the class is the last index; logits of +-80 leave everything finite (the design note's example)."""
    g = _gen(7)
    z = 3.0 * torch.randn(2, 3, 23, generator=g)
    y = (torch.rand(2, 3, 23, generator=g) < 0.3).float()
    w, p = _weights(g, 23, True), _weights(g, 23, True)
    loss, dz = _run_bce(z, y, w, p, 'mean')
    want, dwant = crit_ref.bce(z, y, w, p, 'mean')
    assert_close_scaled('loss', loss, want.reshape(1))
    assert_close_scaled('dz', dz, dwant)
    z = torch.tensor([[80.0, -80.0, 0.0], [-80.0, 80.0, 0.0]])
    y = torch.tensor([[0.0, 1.0, 1.0], [0.0, 1.0, 0.0]])
    p = torch.tensor([2.0, 3.0, 0.5])
    loss, dz = _run_bce(z, y, None, p, 'sum')
    want, dwant = crit_ref.bce(z, y, None, p, 'sum')
    assert torch.isfinite(loss).all() and torch.isfinite(dz).all()
    assert_close_scaled('loss', loss, want.reshape(1))
    assert_close_scaled('dz', dz, dwant)
    assert abs(float(want) - (80.0 + 240.0 + 0.5 * 0.6931471805599453 + 0.6931471805599453)) < 1e-9


def _labels(g, b, O, ignore):
    """-> labels, ignore_index.  'some': a valid class id marks the ignored rows (and row 0 too); 'neg': -1."""
    y = torch.randint(0, O, (b,), generator=g)
    if ignore == 'none':
        return y, -100
    ign = O - 1 if ignore == 'some' else -1
    if ignore == 'some':
        y[y == ign] = 0
    y[::3] = ign
    return y, ign


@pytest.mark.parametrize('b,O', CE_SHAPES)
def test_ce_every_option(b, O):
    g = _gen(200 + b + O)
    z = 3.0 * torch.randn(b, O, generator=g)
    for use_w, eps, ignore, reduction in CE_OPTS:
        w = _weights(g, O, use_w)
        y, ign = _labels(g, b, O, ignore)
        if b == 1 and ignore != 'none':
            y[0] = 0                                                      # (all-ignored has its own test)
        want, dwant = crit_ref.ce(z, y, w, eps, ign, reduction)
        name = f'w={use_w} eps={eps} ignore={ignore} {reduction}'
        loss, dz = _run_ce(z, y, w, eps, ign, reduction)
        assert_close_scaled('loss ' + name, loss, want.reshape(1))
        assert_close_scaled('dz ' + name, dz, dwant)
        if ignore != 'none':
            assert float(dz[(y == ign).to(dev())].abs().sum()) == 0.0, name     # exactly zero, not small
        loss2, _ = _run_ce(z, y, w, eps, ign, reduction, want_dz=False)
        assert_close_scaled('loss, dz == NULL ' + name, loss2, want.reshape(1))


@pytest.mark.parametrize('b,O', [(7, 60), (257, 60)])
def test_ce_all_rows_ignored(b, O):
    g = _gen(300 + b)
    z = torch.randn(b, O, generator=g)
    y = torch.full((b,), -1, dtype=torch.int64)
    w = _weights(g, O, True)
    loss, dz = _run_ce(z, y, w, 0.1, -1, 'mean')
    assert torch.isnan(loss).all() and float(dz.abs().sum()) == 0.0       # as torch: NaN loss, zero gradient
    loss, dz = _run_ce(z, y, w, 0.1, -1, 'sum')
    assert float(loss) == 0.0 and float(dz.abs().sum()) == 0.0


@pytest.mark.parametrize('b,O', [(6, 83), (257, 60)])
def test_ce_extreme_logits_are_finite(b, O):
    g = _gen(400 + b)
    z = torch.randn(b, O, generator=g)
    z[:, 0], z[:, 1] = 80.0, -80.0
    z[1, 0], z[1, 1] = -80.0, 80.0
    y = torch.randint(0, O, (b,), generator=g)
    y[0], y[1], y[2] = 1, 1, 0
    w = _weights(g, O, True)
    loss, dz = _run_ce(z, y, w, 0.1, -100, 'mean')
    want, dwant = crit_ref.ce(z, y, w, 0.1, -100, 'mean')
    assert torch.isfinite(loss).all() and torch.isfinite(dz).all()
    assert_close_scaled('loss', loss, want.reshape(1))
    assert_close_scaled('dz', dz, dwant)


def test_refusals():
    """BMNAS_E_ARG for options outside the descriptor's domain, ahead of every other rule"""
    from bmnas import lib
    so, d = lib.load(), dev()
    z, y, lab = torch.zeros(4, 5, device=d), torch.zeros(4, 5, device=d), torch.zeros(4, dtype=torch.int64, device=d)
    w, loss, dz, rows = torch.ones(5, device=d), torch.zeros(1, device=d), torch.zeros(4, 5, device=d), torch.zeros(4, device=d)
    P = lambda t: ctypes.c_void_p(t.data_ptr())

    def desc(weight=None, pos_weight=None, eps=0.0, reduction=0):
        return lib.CriterionDesc(None if weight is None else weight.data_ptr(),
                                 None if pos_weight is None else pos_weight.data_ptr(), eps, -100, reduction)

    bce = lambda c, n=4, O=5: so.bmnas_bce_logits_crit(P(z), P(y), c, P(loss), P(dz), n, O, None)
    ce = lambda c, b=4, O=5: so.bmnas_cross_entropy_crit(P(z), P(lab), c, P(loss), P(dz), P(rows), b, O, None)
    E_ARG = -1
    for c in (desc(eps=1.0), desc(eps=-0.1), desc(eps=float('nan')), desc(reduction=2), desc(reduction=-1)):
        assert bce(c) == E_ARG and ce(c) == E_ARG
    assert bce(desc(eps=0.1)) == E_ARG                                    # label smoothing is CE's
    assert ce(desc(pos_weight=w)) == E_ARG                                # pos_weight is BCE's
    assert bce(desc(), n=0) == E_ARG and bce(desc(), O=0) == E_ARG and ce(desc(), b=0) == E_ARG
    assert so.bmnas_bce_logits_crit(None, P(y), desc(), P(loss), P(dz), 4, 5, None) == E_ARG
    assert so.bmnas_cross_entropy_crit(P(z), P(lab), desc(), P(loss), P(dz), None, 4, 5, None) == E_ARG
    assert bce(desc(weight=w, pos_weight=w, reduction=1)) == 0 and ce(desc(weight=w, eps=0.5, reduction=1)) == 0
    torch.cuda.synchronize()
