"""Reference arithmetic of the unrolled architecture step's four kernels (csrc/unroll.hip), as numpy sequences with ONE
rounding per operation: dtype=np.float32 is the kernels' bit-for-bit reference (they contract nothing into a fused
multiply-add), dtype=np.float64 the same formulas in double.  tests/test_unroll_ref.py pins both against DARTS' own
statements written with torch CPU ops.

    virtual step   bak = p;  d = g;  wd != 0: d = g + wd * p;  momentum: d = buf * mu + d;  p = p + (-eta) * d
    perturb        p = bak + (sign * R) * v
    restore        p = bak
    combine        d = gp - gn;  ig = d / (2 * R);  out = da - eta * ig
"""
import numpy as np


def _a(x, dtype):
    if hasattr(x, 'detach'):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=dtype)


def virtual_step(p, g, buf, eta, mu=0.0, wd=0.0, dtype=np.float64, plain_terms=False):
    """-> (new p, bak).  buf None: no momentum term (the launch without BMNAS_UNROLL_MOMENTUM, or a NULL buffer).
    plain_terms: the sequence in which a term whose scalar is zero does not exist at all (wd == 0 is such a sequence in
    the kernel already: a branch; mu == 0 is a product by zero there)."""
    p, g = _a(p, dtype), _a(g, dtype)
    neg_eta, mu_, wd_ = dtype(-eta), dtype(mu), dtype(wd)
    d = g
    if wd != 0:
        d = g + wd_ * p
    if buf is not None and not (plain_terms and mu == 0):
        d = _a(buf, dtype) * mu_ + d
    out = p + neg_eta * d
    assert out.dtype == dtype
    return out, p.copy()


def R_of(vs, r):
    """r / ||v|| over a list of tensors, in float64."""
    sq = sum(float((_a(v, np.float64) ** 2).sum()) for v in vs)
    return float(r) / np.sqrt(sq)


def perturb(bak, v, R, sign, dtype=np.float64):
    """bak + fl(sign * R) * v.  R: for dtype=np.float32 pass the fp32 value the launch wrote to R_out."""
    s = dtype(sign) * dtype(R)
    out = _a(bak, dtype) + s * _a(v, dtype)
    assert out.dtype == dtype
    return out


def restore(bak, dtype=np.float64):
    return _a(bak, dtype).copy()


def combine(da, gp, gn, R, eta, dtype=np.float64):
    d = _a(gp, dtype) - _a(gn, dtype)
    ig = d / (dtype(2) * dtype(R))
    out = _a(da, dtype) - dtype(eta) * ig
    assert out.dtype == dtype
    return out
