"""CPU: tests/avg_ref.py — the bits the GPU tests of bmnas_avg_multi compare with — pinned to
torch.optim.swa_utils.AveragedModel itself, for EMA (get_ema_multi_avg_fn(decay)) and SWA, over n = 20 updates.

Three statements per recipe:
  * torch's class run in float64 equals avg_ref's float64 recurrence to float64 rounding: the definition is torch's;
  * avg_ref's fp32 sequence stays within the DERIVED bound of the float64 recurrence: an update has three roundings of
    values no larger than 2 M (M: the largest magnitude in the data) plus the rounding of w, and the earlier error
    enters with a factor (1 - w) <= 1, so |error| <= 5 * n * 2^-24 * M (avg_ref.bound);
  * torch's own fp32 result meets the same bound — or the bound would be wrong."""
import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import swa_utils

import avg_ref

N = 20
SHAPES = [(33, 7), (1,), (129,), (4, 3, 5)]
RECIPES = [None, 0.999, 0.9, 0.5, 0.3]          # SWA; EMA with w = 0.001, 0.1, 0.5 (the boundary), 0.7 (second branch)


class Net(nn.Module):
    def __init__(self, dtype):
        super().__init__()
        self.ps = nn.ParameterList([nn.Parameter(torch.zeros(s, dtype=dtype)) for s in SHAPES])


def snapshots():
    g = torch.Generator().manual_seed(7)
    return [[(3.0 * torch.randn(*s, generator=g)).numpy() for s in SHAPES] for _ in range(N)]


def torch_run(snaps, decay, dtype):
    net = Net(dtype)
    fn = swa_utils.get_ema_multi_avg_fn(decay) if decay is not None else None
    avg = swa_utils.AveragedModel(net, multi_avg_fn=fn)
    for snap in snaps:
        with torch.no_grad():
            for p, x in zip(net.ps, snap):
                p.copy_(torch.from_numpy(x))
        avg.update_parameters(net)
    assert int(avg.n_averaged) == N
    return [p.detach().numpy() for p in avg.module.ps]


@pytest.mark.parametrize('decay', RECIPES, ids=lambda d: 'swa' if d is None else f'ema{d}')
def test_avg_ref_is_torchs_averaged_model(decay):
    snaps = snapshots()
    M = max(float(np.abs(x).max()) for snap in snaps for x in snap)
    bound = avg_ref.bound(N, M)
    exact = avg_ref.run(snaps, decay, np.float64)
    ours = avg_ref.run(snaps, decay, np.float32)
    t64 = torch_run(snaps, decay, torch.float64)
    t32 = torch_run(snaps, decay, torch.float32)
    worst = dict(definition=0.0, ours=0.0, torch=0.0)
    for e, o, a, b in zip(exact, ours, t64, t32):
        assert o.dtype == np.float32 and b.dtype == np.float32
        worst['definition'] = max(worst['definition'], float(np.abs(a - e).max()))
        worst['ours'] = max(worst['ours'], float(np.abs(o.astype(np.float64) - e).max()))
        worst['torch'] = max(worst['torch'], float(np.abs(b.astype(np.float64) - e).max()))
    print(f'decay {decay}: M {M:.3f} bound {bound:.3e} worst {worst}')
    assert worst['definition'] <= 64 * N * 2.0 ** -53 * M        # float64 against float64: rounding only
    assert worst['ours'] <= bound
    assert worst['torch'] <= bound
    assert any(np.abs(o.astype(np.float64) - e).max() > 0 for o, e in zip(ours, exact))     # fp32 really is rounded


def test_first_update_copies_and_both_branches_are_taken():
    a = np.array([1.5, -2.25, 1e-3, 7.0], dtype=np.float32)
    p = np.array([0.1, 3.0, -5e-4, 7.0], dtype=np.float32)
    assert np.array_equal(avg_ref.lerp(a, p, 1.0), p)                                # w = 1: p - d * 0
    assert np.array_equal(avg_ref.lerp(a, p, 0.0), a)                                # w = 0: a + 0 * d
    # at exactly 0.5 the SECOND branch runs (|w| < 0.5 is false): p - d * 0.5, which is not a + 0.5 * d in fp32
    rng = np.random.default_rng(3)
    x, y = rng.standard_normal(1000).astype(np.float32), rng.standard_normal(1000).astype(np.float32)
    d = y - x
    assert np.array_equal(avg_ref.lerp(x, y, 0.5), y - d * np.float32(0.5))
    assert not np.array_equal(y - d * np.float32(0.5), x + np.float32(0.5) * d)
    lo = np.nextafter(np.float32(0.5), np.float32(0))
    assert np.array_equal(avg_ref.lerp(x, y, float(lo)), x + lo * d)


def test_integer_arrays_are_copied():
    out = avg_ref.update([np.zeros(3, np.int64), np.zeros(2, np.float32)],
                         [np.array([5, -1, 2 ** 40], np.int64), np.array([1.0, 2.0], np.float32)], 3, 0.9)
    assert out[0].dtype == np.int64 and np.array_equal(out[0], [5, -1, 2 ** 40])
    assert np.array_equal(out[1], np.float32(0.1) * np.array([1.0, 2.0], np.float32))
