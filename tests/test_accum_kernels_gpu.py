"""-m gpu: bmnas_grad_combine_multi (csrc/accum.hip) through the C ABI, on a hand-built bmnas_adam_tensor_t table,
bit-equal to tests/accum_ref.py (numpy, one fp32 rounding per operation: the kernel contracts nothing).

ONE launch holds destinations of 1, 3, 4, 1023, 1024, 1025 and 2049 elements (one lane, a ragged float4, a whole float4,
one element short of a chunk, a whole chunk, one past it, two chunks and one) and a 1031-element view one float off the
16-byte alignment (the scalar path), NaN guards round every destination, a tensor with a NULL part in the middle, one
whose first part is NULL, one part that alone is one float off alignment, and a NaN and a denormal inside a part.
m in {1, 2, 3, 8}; weights {1, 1/3, 0.5, 1/7} (cycled for m = 8).  The parts and the guards must not change."""
import ctypes as C

import numpy as np
import pytest
import torch

import accum_ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 1023, 1024, 1025, 2049]
OFF_SIZE = 1031
WEIGHTS = [1.0, 1.0 / 3.0, 0.5, 1.0 / 7.0]
PAD = 4


def _rand(seed, n, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(n, generator=g) * scale


def _guarded(t, off=0):
    """t inside a NaN-filled store, PAD + off elements from its 16-byte aligned start -> (view, store)"""
    store = torch.full((t.numel() + 2 * PAD + 1,), float('nan'), device=dev())
    view = store[PAD + off:PAD + off + t.numel()]
    view.copy_(t)
    return view, store


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _weights(m):
    return [1.0] if m == 1 else [WEIGHTS[(i + 1) % len(WEIGHTS)] for i in range(m)]


def _launch(lib, dsts, parts, m, weights):
    """dsts: device views; parts[t][i]: device view or None."""
    from bmnas.optim import _DESC
    tab = np.zeros(len(dsts), dtype=_DESC)
    tab['grad'] = [d.data_ptr() for d in dsts]
    tab['numel'] = [d.numel() for d in dsts]
    ptrs = np.array([[0 if p is None else p.data_ptr() for p in row] for row in parts], dtype='<u8').reshape(-1)
    E = lib.adam_chunk_elems()
    chunks = [(i, c) for i, d in enumerate(dsts) for c in range((d.numel() + E - 1) // E)]
    d_tab = torch.from_numpy(tab.view(np.uint8)).to(dev())
    d_ptrs = torch.from_numpy(ptrs.view(np.uint8)).to(dev())
    d_chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev())
    torch.cuda.synchronize()
    lib.grad_combine_multi(d_tab, d_chunks, len(chunks), d_ptrs, m, weights)
    torch.cuda.synchronize()
    return len(chunks)


@pytest.mark.parametrize('m', [1, 2, 3, 8])
def test_grad_combine_multi_is_accum_ref_bit_for_bit(m):
    from bmnas import lib
    assert lib.accum_max() == 8
    sizes = SIZES + [OFF_SIZE]
    last = len(sizes) - 1
    weights = _weights(m)
    host, dsts, parts = [], [], []
    for t, n in enumerate(sizes):
        off = 1 if t == last else 0
        dsts.append(_guarded(torch.full((n,), 7.0), off))              # stale values: every element must be overwritten
        row_h, row_d = [], []
        for i in range(m):
            h = _rand(100 * t + i, n, 1.0 + i)
            if n >= 4 and i == 0:
                h[1] = float('nan')                                    # NaN propagates
                h[2] = 1e-42                                           # a denormal (kept: fp32 denormals are on)
            p_off = off
            if t == 4 and i == m - 1 and m > 1:
                p_off = 1                                              # ONE part off alignment: the whole tensor goes scalar
            row_h.append(h.numpy())
            row_d.append(_guarded(h, p_off))
        if m >= 3:
            if t == 3:
                row_h[1], row_d[1] = None, None                        # a NULL part in the middle
            if t == 5:
                row_h[0], row_d[0] = None, None                        # the first part is NULL
        if m == 2 and t == 5:
            row_h[0], row_d[0] = None, None
        host.append(row_h)
        parts.append(row_d)
        assert dsts[-1][0].data_ptr() % 16 == 4 * off
    part_before = [[None if p is None else _bits(p[1]) for p in row] for row in parts]
    guard_before = [_bits(s) for _, s in dsts]

    n_chunks = _launch(lib, [v for v, _ in dsts], [[None if p is None else p[0] for p in row] for row in parts], m,
                       weights)
    assert n_chunks == 1 + 1 + 1 + 1 + 1 + 2 + 3 + 2

    for t, n in enumerate(sizes):
        want = accum_ref.combine(host[t], weights)
        got = dsts[t][0].cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (n, m)
        if n >= 4 and host[t][0] is not None:
            assert np.isnan(got[1])
        lo = PAD + (1 if t == last else 0)
        after = _bits(dsts[t][1])
        assert torch.equal(after[:lo], guard_before[t][:lo]) and torch.equal(after[lo + n:], guard_before[t][lo + n:])
        for p, before in zip(parts[t], part_before[t]):
            if p is not None:
                assert torch.equal(_bits(p[1]), before)
    if m == 1:
        # w = 1 leaves the bits of the part: a copy, the NaN and the denormal included
        for t in range(len(sizes)):
            assert np.array_equal(dsts[t][0].cpu().numpy().view(np.int32), host[t][0].view(np.int32))
        assert dsts[3][0].cpu().numpy()[2] == np.float32(1e-42) != 0.0


def test_grad_combine_multi_all_null_stores_plus_zero():
    from bmnas import lib
    d0, s0 = _guarded(torch.full((1025,), 7.0))
    d1, s1 = _guarded(torch.full((5,), 7.0), 1)
    p = _rand(1, 5).to(dev())
    _launch(lib, [d0, d1], [[None, None], [None, p]], 2, [0.5, 1.0])
    assert torch.equal(_bits(d0), torch.zeros(1025, dtype=torch.int32))                # +0, not -0
    assert torch.equal(_bits(d1), _bits(p))
    assert bool(torch.isnan(s0[:PAD]).all()) and bool(torch.isnan(s0[PAD + 1025:]).all())


def test_grad_combine_multi_refuses_bad_arguments():
    from bmnas import lib
    fn = lib.load().bmnas_grad_combine_multi
    one = torch.zeros(64, dtype=torch.uint8, device=dev())
    p = one.data_ptr()
    w = (C.c_float * 9)(*([1.0] * 9))
    assert fn(None, p, 1, p, 1, w, None) == -1 and fn(p, None, 1, p, 1, w, None) == -1
    assert fn(p, p, 1, None, 1, w, None) == -1 and fn(p, p, 1, p, 1, None, None) == -1
    assert fn(p, p, 1, p, 0, w, None) == -1 and fn(p, p, 1, p, 9, w, None) == -1
    assert fn(p, p, -1, p, 1, w, None) == -1
    assert fn(p, p, 0, p, 1, w, None) == 0                      # nothing to do: no launch
    with pytest.raises(lib.BmnasError, match='weights'):
        lib.grad_combine_multi(one, one, 0, one, 2, [1.0])
