"""tests/bn_momentum_ref.py against torch.nn.BatchNorm1d(momentum=m).double() on the CPU: three consecutive training-mode
batches of different sizes, from fresh buffers and from random buffers with the counter at 5."""
import pytest
import torch

import bn_momentum_ref as mr

M, L = 6, 4
BATCHES = (3, 7, 2)


@pytest.mark.parametrize('start', ['fresh', 'random buffers, counter 5'])
@pytest.mark.parametrize('momentum', [0.0, 0.05, 0.1, 0.5, 1.0, None])
def test_sequence_matches_torch_batchnorm(momentum, start):
    g = torch.Generator().manual_seed(11)
    bn = torch.nn.BatchNorm1d(M, momentum=momentum).double()
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.3 * torch.randn(M, generator=g, dtype=torch.float64))
        bn.bias.copy_(0.5 * torch.randn(M, generator=g, dtype=torch.float64))
        if start != 'fresh':
            bn.running_mean.copy_(torch.randn(M, generator=g, dtype=torch.float64))
            bn.running_var.copy_(0.5 + torch.randn(M, generator=g, dtype=torch.float64).abs())
            bn.num_batches_tracked.fill_(5)
    xs = [2.0 * torch.randn(b, M, L, generator=g, dtype=torch.float64) + 1.0 for b in BATCHES]
    rm0, rv0, n0 = bn.running_mean.clone(), bn.running_var.clone(), int(bn.num_batches_tracked)
    outs, rm, rv, nbt = mr.bn_sequence(xs, bn.weight.detach(), bn.bias.detach(), rm0, rv0, n0, momentum)
    bn.train()
    for x, want in zip(xs, outs):
        torch.testing.assert_close(bn(x).detach(), want, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bn.running_mean, rm, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(bn.running_var, rv, rtol=1e-12, atol=1e-12)
    assert int(bn.num_batches_tracked) == nbt == n0 + len(BATCHES)
    if momentum == 0.0:
        assert torch.equal(rm, rm0) and torch.equal(rv, rv0)
    if momentum == 1.0:
        mean, _, unbiased = mr.batch_stats(xs[-1])
        torch.testing.assert_close(rm, mean, rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(rv, unbiased, rtol=1e-12, atol=1e-12)


def test_cumulative_from_zero_is_the_plain_mean():
    g = torch.Generator().manual_seed(12)
    xs = [torch.randn(b, M, L, generator=g, dtype=torch.float64) for b in BATCHES]
    rm0, rv0 = torch.randn(M, generator=g, dtype=torch.float64), torch.rand(M, generator=g, dtype=torch.float64) + 0.5
    _, rm, rv, nbt = mr.bn_sequence(xs, torch.ones(M), torch.zeros(M), rm0, rv0, 0, None)
    stats = [mr.batch_stats(x) for x in xs]
    torch.testing.assert_close(rm, sum(s[0] for s in stats) / 3, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(rv, sum(s[2] for s in stats) / 3, rtol=1e-12, atol=1e-12)
    assert nbt == 3 and mr.factor(None, 5) == 1.0 / 6 and mr.factor(0.25, 5) == 0.25
