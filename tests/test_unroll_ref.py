"""CPU: tests/unroll_ref.py against DARTS' own statements of the unrolled step (cnn/architect.py of Liu et al. 2019),
written with torch CPU ops:

    moment = momentum_buffer.mul(momentum);  dtheta = grad + weight_decay * theta
    theta.sub(moment + dtheta, alpha=eta)                                  (theta.sub(eta, moment + dtheta))
    p.data.add_(v, alpha=R)  /  p.data.sub_(v, alpha=R)                    (w+ / w- about the unperturbed w)
    ig = (x - y).div_(2 * R);  g.sub_(ig, alpha=eta)                       (g.data.sub_(eta, ig.data))

float64: tight (a few ulp of the largest operand).  fp32: bit for bit wherever torch rounds each operation once — the
products by a scalar, the sums of two tensors, the difference and the division.  torch's CPU kernel for `add / sub(other,
alpha=s)` FUSES: its vectorised loop is one fmadd(other, s, self), a single rounding where the reference (and the gfx950
kernel, which contracts nothing) rounds the product and then the sum.  Those three statements — `theta.sub(.., alpha=eta)`,
`p.add_ / p.sub_(v, alpha=R)` and `g.sub_(ig, alpha=eta)` — are compared at 1 ulp, U = the spacing at the largest of
|self|, |s * other| and |result|: the two exact sums differ by the product's own rounding error, at most U / 2, and two
reals that close round to grid points at most U apart (the grid at the result is no coarser than U)."""
import numpy as np
import pytest
import torch

import unroll_ref as ur

N = 4099
ETA, MU, WD, R = 1e-2, 0.9, 3e-4, 3.7e-3


def _t(seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, generator=g) * scale


def _inputs(dtype):
    return [t.to(dtype) for t in (_t(1), _t(2, 0.3), _t(3, 0.1))]


def _ulp_of_largest(*operands):
    """spacing of the dtype at the elementwise largest magnitude of the operands and the result"""
    m = np.maximum.reduce([np.abs(o) for o in operands])
    return np.spacing(m)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int32 if a.dtype == np.float32 else np.int64)


@pytest.mark.parametrize('momentum', [False, True])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_virtual_step_is_darts_theta_sub(dtype, momentum):
    nd = np.float64 if dtype == torch.float64 else np.float32
    theta, grad, buf = _inputs(dtype)
    dtheta = grad + WD * theta
    moment = buf.mul(MU) if momentum else torch.zeros_like(theta)
    # the unfused parts, bit for bit (one rounding per torch op)
    d_ref = (grad.numpy() + nd(WD) * theta.numpy())
    assert np.array_equal(_bits(dtheta.numpy()), _bits(d_ref))
    if momentum:
        d_ref = buf.numpy() * nd(MU) + d_ref
        assert np.array_equal(_bits((moment + dtheta).numpy()), _bits(d_ref))
    want = theta.sub(moment + dtheta, alpha=ETA).numpy()
    got, bak = ur.virtual_step(theta, grad, buf if momentum else None, ETA, MU, WD, dtype=nd)
    assert np.array_equal(_bits(bak), _bits(theta.numpy()))
    # `theta.sub(.., alpha=eta)`: FUSED by torch's CPU kernel -> 1 ulp of the largest operand
    tol = _ulp_of_largest(theta.numpy(), nd(ETA) * d_ref, want)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol).all()
    assert not np.array_equal(got, theta.numpy())


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_zero_decay_and_zero_momentum_are_the_sequence_without_them(dtype):
    nd = np.float64 if dtype == torch.float64 else np.float32
    theta, grad, buf = _inputs(dtype)
    plain, _ = ur.virtual_step(theta, grad, None, ETA, dtype=nd)
    assert np.array_equal(_bits(plain), _bits(theta.numpy() + nd(-ETA) * grad.numpy()))
    zero_mu, _ = ur.virtual_step(theta, grad, buf, ETA, 0.0, 0.0, dtype=nd)
    assert np.array_equal(_bits(zero_mu), _bits(plain))                      # buf * 0 + g == g for finite buf, g != -0
    skipped, _ = ur.virtual_step(theta, grad, buf, ETA, 0.0, 0.0, dtype=nd, plain_terms=True)
    assert np.array_equal(_bits(skipped), _bits(plain))


@pytest.mark.parametrize('sign', [1, -1])
@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_perturb_is_darts_add_and_sub_about_the_backup(dtype, sign):
    nd = np.float64 if dtype == torch.float64 else np.float32
    w, _, v = _inputs(dtype)
    want = w.clone()
    (want.add_ if sign > 0 else want.sub_)(v, alpha=float(nd(R)))          # FUSED by torch's CPU kernel
    got = ur.perturb(w, v, nd(R), sign, dtype=nd)
    tol = _ulp_of_largest(w.numpy(), nd(R) * v.numpy(), want.numpy())
    assert (np.abs(got.astype(np.float64) - want.numpy().astype(np.float64)) <= tol).all()
    assert np.array_equal(_bits(ur.restore(w, dtype=nd)), _bits(w.numpy()))


def test_R_is_r_over_the_norm_of_the_concatenation():
    vs = [_t(5, 0.01).double(), _t(6, 0.02).double()[:1000]]
    want = 1e-2 / float(torch.cat([x.view(-1) for x in vs]).norm())
    assert abs(ur.R_of(vs, 1e-2) - want) <= 1e-14 * want


@pytest.mark.parametrize('dtype', [torch.float64, torch.float32])
def test_combine_is_darts_difference_quotient_and_sub(dtype):
    nd = np.float64 if dtype == torch.float64 else np.float32
    da, x, y = _inputs(dtype)
    y = x + 1e-3 * y                                                        # g+ and g- are close, as in the step
    Rt = torch.tensor(R, dtype=dtype)
    ig = (x - y).div_(2 * Rt)
    # the difference and the division: one rounding each in torch, bit for bit
    ig_ref = (x.numpy() - y.numpy()) / (nd(2) * nd(R))
    assert np.array_equal(_bits(ig.numpy()), _bits(ig_ref))
    want = da.clone().sub_(ig, alpha=ETA).numpy()                           # FUSED by torch's CPU kernel
    got = ur.combine(da, x, y, nd(R), ETA, dtype=nd)
    tol = _ulp_of_largest(da.numpy(), nd(ETA) * ig_ref, want)
    assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= tol).all()
    assert not np.array_equal(got, da.numpy())
