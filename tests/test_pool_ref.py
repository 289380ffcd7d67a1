"""CPU: tests/pool_ref.py — the statement of the pooling rule the half-precision GPU tests compare with — is pinned to
F.adaptive_max_pool2d(..., return_indices=True) on the CPU, for fp32, bf16 and fp16: windows, first maximum, NaN, the
argmax, and the backward as an fp32 sum rounded once to the element type."""
import pytest
import torch
import torch.nn.functional as F

import pool_ref

DTYPES = [torch.float32, torch.bfloat16, torch.float16]
CASES = [((2, 3, 8, 40), (4, 1)), ((2, 3, 5, 7), (4, 1)), ((2, 3, 2, 7), (4, 1)), ((2, 3, 13, 9), (8, 1)),
         ((3, 48, 1, 1), (8, 1)), ((2, 3, 20, 32), (4, 4)), ((2, 3, 5, 8), (4, 4)), ((2, 3, 3, 3), (4, 4)),
         ((2, 3, 6, 6), (4, 4)), ((2, 16, 1, 1), (4, 4))]


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape,out', CASES)
def test_forward_is_atens_cpu_pool(shape, out, dtype):
    """values (as the exact fp32 widening) and indices; inputs with ties everywhere, +0 / -0, an all-equal and an
    all -inf window, and at most one NaN per plane"""
    x = pool_ref.make_input(shape, *out, dtype, seed=5, several_nans=False)
    assert x.isnan().any() and (x == 0).any()
    v, i = F.adaptive_max_pool2d(x, out, return_indices=True)
    assert v.dtype == dtype
    got_v, got_i = pool_ref.pool_fwd(x, *out)
    want_v = v.float().reshape(got_v.shape)
    assert got_v.dtype == torch.float32 and got_i.dtype == torch.int32
    assert torch.equal(got_v.isnan(), want_v.isnan())
    assert torch.equal(got_v.nan_to_num(nan=7.0).view(torch.int32), want_v.nan_to_num(nan=7.0).view(torch.int32))  # (-0 too)
    # the same op on the widened input: the element type changes nothing
    v32, i32 = F.adaptive_max_pool2d(x.float(), out, return_indices=True)
    assert torch.equal(v32.isnan(), v.isnan()) and torch.equal(v32.nan_to_num(nan=7.0), v.float().nan_to_num(nan=7.0))
    assert torch.equal(got_i.long(), i32.reshape(got_i.shape))
    # aten's reduced-precision CPU loop carries the index in the element type: it is exact only while the plane's flat
    # indices are (bf16: < 2^8, fp16: < 2^11) — there the half op itself gives the same indices
    if shape[2] * shape[3] <= {torch.float32: 1 << 24, torch.bfloat16: 1 << 8, torch.float16: 1 << 11}[dtype]:
        assert torch.equal(i, i32)


def test_several_nans_in_a_window_the_first_is_kept():
    """The one known difference: aten's CPU loop keeps the LAST NaN of a window, the kernels (and pool_ref) the first.
    The value is a NaN either way."""
    x = torch.arange(16.).view(1, 1, 4, 4).clone()
    x[0, 0, 0, 1] = float('nan')
    x[0, 0, 1, 0] = float('nan')
    v, i = pool_ref.pool_fwd(x, 2, 2)
    assert v[0, 0].isnan().tolist() == [True, False, False, False]
    assert i[0, 0].tolist() == [1, 7, 13, 15]
    tv, ti = F.adaptive_max_pool2d(x, (2, 2), return_indices=True)
    assert torch.equal(tv.isnan().view(-1), v.isnan().view(-1)) and ti.view(-1).tolist()[1:] == [7, 13, 15]
    assert ti.view(-1)[0].item() in (1, 4)                       # (4 with the aten loop as it stands)


@pytest.mark.parametrize('dtype', DTYPES, ids=str)
@pytest.mark.parametrize('shape,out', CASES)
def test_backward_is_the_fp32_scatter_rounded_once(shape, out, dtype):
    """gradients that are multiples of 2^-6 in [-4, 4]: every window sum is exact in fp32, so autograd's scatter on the
    widened input gives THE fp32 sum, whatever its order; the expected dx is that sum narrowed once"""
    x = pool_ref.make_input(shape, *out, dtype, seed=6, several_nans=False)
    g = pool_ref.make_grad((shape[0], shape[1], out[0] * out[1]), seed=7)
    _, idx = pool_ref.pool_fwd(x, *out)
    got = pool_ref.pool_bwd(g, idx, shape[2], shape[3], dtype)
    x32 = x.float().requires_grad_(True)
    F.adaptive_max_pool2d(x32, out).backward(g.view(shape[0], shape[1], *out))
    assert got.dtype == dtype and torch.equal(got, x32.grad.to(dtype))
    if dtype == torch.float32:
        assert torch.equal(got, x32.grad)


def test_narrowing_to_bf16_really_rounds():
    """sums of the test gradients need more than bf16's 8 significant bits, and ties go to even"""
    s = torch.tensor([5.0 + 2.0 ** -6, 9.0 + 3 * 2.0 ** -6, 1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8])
    n = s.to(torch.bfloat16).float()
    assert not torch.equal(n[:2], s[:2])
    assert n[2].item() == 1.0 and n[3].item() == 1.0 + 2.0 ** -6        # ties to even, both ways
    g = pool_ref.make_grad((2, 3, 16), 7)
    assert not torch.equal((g[..., :8] + g[..., 8:]).to(torch.bfloat16).float(), g[..., :8] + g[..., 8:])
