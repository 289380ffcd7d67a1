"""-m gpu: bmnas_avg_multi (csrc/average.hip) through the C ABI, on a hand-built bmnas_adam_tensor_t table, bit-equal to
tests/avg_ref.py (numpy, one fp32 rounding per operation: the kernel contracts nothing).

ONE launch holds: averaged tensors of 1, 3, 4, 1023, 1024, 1025 and 2049 elements (one lane, a ragged float4, a whole
float4, one element short of a chunk, a whole chunk, one past it, two chunks and one), one view one float off the 16-byte
alignment (the scalar path), an int64 tensor that is 8-byte aligned only and a float tensor of arbitrary bit patterns (NaN
payloads, denormals) on RAW rows — and rows with w = 1, 0.75, 0.5, 0.25 and 0 side by side, so both branches of the
lerp rule, its boundary, the copy of a first update and the identity run in the same grid.  Two assignments of rows to
tensors, so every tensor size meets both branches.  NaN guards around every buffer; the live tensors must not change.
The count store: every row carries a count of its own, n_averaged receives that of tensor 0's row."""
import numpy as np
import pytest
import torch

import avg_ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

SIZES = [1, 3, 4, 1023, 1024, 1025, 2049]
OFF_SIZE = 1031                       # the view one float off alignment
WEIGHTS = [1.0, 0.75, 0.5, 0.25, 0.0]
RAW_I64, RAW_F32 = len(WEIGHTS), len(WEIGHTS) + 1      # two RAW rows: the int64 tensor's and the float tensor's
PAD = 4                               # guard elements on each side of a buffer (keeps 16-byte alignment)
N_I64, N_RAWF = 5, 1027


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


@pytest.mark.parametrize('shift', [0, 2])
def test_avg_multi_is_avg_ref_bit_for_bit(shift):
    from bmnas import lib
    from bmnas.optim import _AVG_ROW, _DESC
    sizes = SIZES + [OFF_SIZE]
    host_a = [_rand(10 + i, n) for i, n in enumerate(sizes)]
    host_p = [_rand(50 + i, n, 2.0) for i, n in enumerate(sizes)]
    host_p[4][:8] = host_a[4][:8]                                       # p == a somewhere: d = 0
    avg, live = [], []
    for i, (a, p) in enumerate(zip(host_a, host_p)):
        off = 1 if i == len(sizes) - 1 else 0
        avg.append(_guarded(a, off))
        live.append(_guarded(p, off))
        assert avg[-1][0].data_ptr() % 16 == 4 * off and live[-1][0].data_ptr() % 16 == 4 * off
    # RAW: an int64 tensor 8 bytes off the 16-byte alignment, and floats of arbitrary bits
    g = torch.Generator().manual_seed(99)
    i64_src = torch.randint(-2 ** 62, 2 ** 62, (N_I64 + 3,), generator=g, dtype=torch.int64).to(dev())
    i64_dst = torch.full((N_I64 + 3,), -7, dtype=torch.int64, device=dev())
    assert i64_src[1:].data_ptr() % 16 == 8 and i64_dst[1:].data_ptr() % 16 == 8
    rawf_bits = torch.randint(-2 ** 31, 2 ** 31 - 1, (N_RAWF,), generator=g, dtype=torch.int64).to(torch.int32)
    rawf_src = rawf_bits.to(dev()).view(torch.float32)
    rawf_dst, rawf_store = _guarded(torch.zeros(N_RAWF))

    row_of = [(i + shift) % len(WEIGHTS) for i in range(len(sizes))]
    rows = np.zeros(len(WEIGHTS) + 2, dtype=_AVG_ROW)
    for r, w in enumerate(WEIGHTS):
        rows[r] = (np.float32(w), np.float32(1.0 - w), 0, 0, 100 + r, 0)
    for r in (RAW_I64, RAW_F32):
        rows[r] = (0.3, 0.7, lib.AVG_RAW, 0, 100 + r, 0)              # (the weights of a RAW row are not read)
    tab = np.zeros(len(sizes) + 2, dtype=_DESC)
    tab['param'] = [v.data_ptr() for v, _ in avg] + [i64_dst[1:1 + N_I64].data_ptr(), rawf_dst.data_ptr()]
    tab['grad'] = [v.data_ptr() for v, _ in live] + [i64_src[1:1 + N_I64].data_ptr(), rawf_src.data_ptr()]
    tab['numel'] = sizes + [2 * N_I64, N_RAWF]                          # RAW: 32-bit words
    tab['hyp_row'] = row_of + [RAW_I64, RAW_F32]
    E = lib.adam_chunk_elems()
    chunks = [(i, c) for i, n in enumerate(tab['numel'].tolist()) for c in range((n + E - 1) // E)]
    assert len(chunks) == 1 + 1 + 1 + 1 + 1 + 2 + 3 + 2 + 1 + 2
    d_tab = torch.from_numpy(tab.view(np.uint8)).to(dev())
    d_rows = torch.from_numpy(rows.view(np.uint8)).to(dev())
    d_chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev())
    n_averaged = torch.full((3,), -1, dtype=torch.int64, device=dev())
    torch.cuda.synchronize()
    live_before = [_bits(s) for _, s in live]
    guard_before = [_bits(s) for _, s in avg]

    lib.avg_multi(d_tab, d_chunks, len(chunks), d_rows, n_averaged[1:2])
    torch.cuda.synchronize()

    for i, (a, p) in enumerate(zip(host_a, host_p)):
        want = avg_ref.lerp(a.numpy(), p.numpy(), WEIGHTS[row_of[i]])
        got = avg[i][0].cpu().numpy()
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (sizes[i], WEIGHTS[row_of[i]])
        if WEIGHTS[row_of[i]] == 1.0:
            assert np.array_equal(got.view(np.int32), p.numpy().view(np.int32))          # the first update: a copy
        if WEIGHTS[row_of[i]] == 0.0:
            assert np.array_equal(got.view(np.int32), a.numpy().view(np.int32))
        # nothing outside the tensor was written, and the live tensor was not touched
        lo = PAD + (1 if i == len(sizes) - 1 else 0)
        after = _bits(avg[i][1])
        assert torch.equal(after[:lo], guard_before[i][:lo]) and torch.equal(after[lo + sizes[i]:],
                                                                             guard_before[i][lo + sizes[i]:])
        assert torch.equal(_bits(live[i][1]), live_before[i])
    assert torch.equal(i64_dst[1:1 + N_I64], i64_src[1:1 + N_I64])
    assert int(i64_dst[0]) == -7 and bool((i64_dst[1 + N_I64:] == -7).all())
    assert torch.equal(rawf_dst.view(torch.int32).cpu(), rawf_bits)                      # bits, NaN payloads included
    store_bits = _bits(rawf_store)
    assert bool((store_bits[:PAD] == store_bits[0]).all()) and bool((store_bits[PAD + N_RAWF:] == store_bits[0]).all())
    assert n_averaged.tolist() == [-1, 100 + row_of[0], -1]                              # tensor 0's row, one store


def test_avg_multi_refuses_null_arguments():
    from bmnas import lib
    fn = lib.load().bmnas_avg_multi
    one = torch.zeros(64, dtype=torch.uint8, device=dev())
    p = one.data_ptr()
    assert fn(None, p, 1, p, p, None) == -1 and fn(p, None, 1, p, p, None) == -1
    assert fn(p, p, 1, None, p, None) == -1 and fn(p, p, 1, p, None, None) == -1
    assert fn(p, p, 0, p, p, None) == -1
    with pytest.raises(lib.BmnasError, match='int64'):
        lib.avg_multi(one, one, 1, one, torch.zeros(1, device=dev()))
