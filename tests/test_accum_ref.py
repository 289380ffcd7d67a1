"""CPU: tests/accum_ref.py — the reference the combine kernel is held to bit for bit — against torch on the CPU, operation
by operation: acc = torch.mul(g0, w0), then acc = torch.add(acc, torch.mul(gi, wi)).  Weights include 1/3 and 1/7 (no
powers of two: every product rounds)."""
import numpy as np
import torch

import accum_ref

WEIGHTS = [1.0, 1.0 / 3.0, 0.5, 1.0 / 7.0, 0.25, 3.0 / 8.0, 1.0 / 3.0, 1.0 / 7.0]


def _parts(m, n, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) * (1.0 + i) for i in range(m)]


def _torch_combine(parts, weights):
    acc = None
    for g, w in zip(parts, weights):
        if g is None:
            continue
        t = torch.mul(g, float(np.float32(w)))
        acc = t if acc is None else torch.add(acc, t)
    return acc


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.int32), np.asarray(b).view(np.int32))


def test_combine_is_torch_mul_add_bit_for_bit():
    for m in (1, 2, 3, 8):
        parts = _parts(m, 4099, 7 + m)
        ws = WEIGHTS[:m] if m > 1 else [1.0 / 3.0]
        got = accum_ref.combine([p.numpy() for p in parts], ws)
        assert got.dtype == np.float32
        assert _same_bits(got, _torch_combine(parts, ws).numpy()), m


def test_none_parts_are_left_out_and_weight_one_keeps_the_bits():
    parts = _parts(3, 1027, 3)
    ws = [1.0 / 3.0, 1.0, 1.0 / 7.0]
    mid = [parts[0], None, parts[2]]
    got = accum_ref.combine([None if p is None else p.numpy() for p in mid], ws)
    assert _same_bits(got, _torch_combine(mid, ws).numpy())
    first = [None, parts[1], parts[2]]
    got = accum_ref.combine([None if p is None else p.numpy() for p in first], ws)
    assert _same_bits(got, _torch_combine(first, ws).numpy())
    # the first term is the product itself, not 0 + product: -0 survives
    neg0 = np.array([-0.0, 1.0], dtype=np.float32)
    assert _same_bits(accum_ref.combine([None, neg0], [0.5, 1.0]), neg0)
    # m = 1, w = 1: a bit copy, denormals included
    odd = np.array([1e-42, -3e-39, 2.5, -0.0], dtype=np.float32)
    assert _same_bits(accum_ref.combine([odd], [1.0]), odd)
    assert _same_bits(accum_ref.combine([None, None], [0.5, 0.5], shape=(3,)), np.zeros(3, dtype=np.float32))


def test_nan_propagates_and_the_sum_rounds_twice():
    a = np.array([1.0, np.nan, 3.0], dtype=np.float32)
    b = np.array([np.nan, 1.0, 1.0], dtype=np.float32)
    got = accum_ref.combine([a, b], [0.5, 1.0 / 3.0])
    assert np.isnan(got[0]) and np.isnan(got[1]) and not np.isnan(got[2])
    # a value where fma(w, g, acc) and round(acc + round(w * g)) differ: the reference is the latter
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(20000, generator=g).numpy(), torch.randn(20000, generator=g).numpy()
    w = np.float32(1.0 / 3.0)
    two = accum_ref.combine([x, y], [1.0, w])
    fused = (x.astype(np.float64) + np.float64(w) * y.astype(np.float64)).astype(np.float32)
    assert not _same_bits(two, fused)                  # some element rounds differently ...
    assert np.allclose(two, fused, rtol=1e-6, atol=1e-7)   # ... by an ulp
