"""CPU: bmnas.metrics.PhaseStats on CPU tensors — wholly through its torch restatement of the tally (`_update_torch`) —
gives what the loop's AccuracyMeter / F1Meter and its float64 loss sum give on the same batches; from_meter, the refusals
and the counters."""
import types

import numpy as np
import pytest
import torch

import stats_ref as R


def _loop():
    import models.search.train_searchable._loop as loop
    return loop


def _f1_batches(O, th, seed):
    g = torch.Generator().manual_seed(seed)
    thr = R.logit_threshold(th)
    out = []
    for n in (5, 1, 9):                               # three updates of different n
        x = torch.from_numpy(R.off_band((torch.randn(n, O, generator=g) * 2).numpy(), thr))
        y = (torch.rand(n, O, generator=g) > 0.6).float()
        y[:, 1] = 0                                   # an absent class
        out.append((torch.rand((), generator=g), x, y))
    assert all(R.band_empty(x.numpy(), thr) for _, x, _ in out)
    return out


@pytest.mark.parametrize('f1_type', ['weighted', 'macro', 'micro'])
def test_f1_on_the_cpu_is_the_meters(f1_type):
    from bmnas.metrics import PhaseStats
    loop = _loop()
    meter = loop.F1Meter(f1_type, 0.3)
    stats = PhaseStats.from_meter(meter)
    assert (stats.kind, stats.f1_type, stats.threshold, stats.name) == ('f1', f1_type, 0.3, meter.name)
    assert stats.logit_threshold == R.logit_threshold(0.3)
    for phase in range(2):                            # a second phase: reset() empties the same accumulator
        meter.reset('cpu')
        stats.reset('cpu')
        loss_sum = torch.zeros((), dtype=torch.float64)
        acc = R.empty(6)
        seen = 0
        for loss, x, y in _f1_batches(6, 0.3, 10 + phase):
            loss_sum += loss.detach().double() * y.size(0)
            meter.update(x, y)
            stats.update(loss, x, y)
            R.tally_f1(acc, x.numpy(), y.numpy(), float(loss), stats.logit_threshold)
            seen += y.size(0)
        assert stats.acc.numpy().tobytes() == acc.tobytes()
        assert stats.loss_sum() == float(loss_sum) and stats.samples() == seen == 15 and stats.tallies() == 3
        assert stats.compute(seen) == meter.compute(seen)
    assert stats.fallbacks == 6 and stats.launches == 0


def test_accuracy_on_the_cpu_is_the_meters():
    from bmnas.metrics import PhaseStats
    loop = _loop()
    meter = loop.AccuracyMeter()
    stats = PhaseStats.from_meter(meter)
    assert (stats.kind, stats.f1_type, stats.name) == ('acc', None, 'Acc')
    meter.reset('cpu')
    stats.reset('cpu')
    g = torch.Generator().manual_seed(4)
    loss_sum = torch.zeros((), dtype=torch.float64)
    acc = R.empty(5)
    for n in (4, 7, 2):
        x = torch.randn(n, 5, generator=g)
        x[0, 1] = x[0, 3] = 8.0                       # a tie: the first wins
        y = torch.randint(0, 5, (n,), generator=g)
        y[-1] = -100                                  # never equal
        loss = torch.rand((), generator=g)
        loss_sum += loss.detach().double() * n
        meter.update(x, y)
        stats.update(loss, x, y)
        R.tally_acc(acc, x.numpy(), y.numpy(), float(loss))
    assert stats.acc.numpy().tobytes() == acc.tobytes()
    assert stats.compute(13) == meter.compute(13)
    assert stats.loss_sum() == float(loss_sum) and stats.samples() == 13
    assert (stats.launches, stats.fallbacks) == (0, 3)
    # other dtypes take the same route: fp64 logits, int32 labels, no loss
    stats.reset('cpu')
    stats.update(None, torch.eye(5, dtype=torch.float64), torch.arange(5, dtype=torch.int32))
    assert stats.compute(5) == 1.0 and stats.loss_sum() == 0.0 and stats.fallbacks == 4


def test_from_meter_knows_the_loops_own_meters_only():
    from bmnas.metrics import PhaseStats
    loop = _loop()

    class Mine(loop.AccuracyMeter):
        def update(self, output, labels):
            pass

    assert PhaseStats.from_meter(Mine()) is None
    assert PhaseStats.from_meter(object()) is None
    assert PhaseStats.from_meter(loop.F1Meter('macro', 0.5)).f1_type == 'macro'


def test_refusals():
    from bmnas.lib import BmnasError
    from bmnas.metrics import PhaseStats
    loop = _loop()
    with pytest.raises(BmnasError, match='samples'):
        PhaseStats('f1', 'samples', 0.3)
    with pytest.raises(BmnasError, match='samples'):
        PhaseStats.from_meter(loop.F1Meter('samples', 0.3))
    with pytest.raises(BmnasError):
        PhaseStats('auc')
    with pytest.raises(BmnasError):
        PhaseStats('f1', 'weighted', 1.0)
    stats = PhaseStats('f1', 'weighted', 0.3)
    stats.reset('cpu')
    with pytest.raises(BmnasError, match='O >= 2'):
        stats.update(None, torch.zeros(3, 1), torch.zeros(3, 1))
    assert stats.acc is None and stats.fallbacks == 0
    one = PhaseStats('acc')                           # (a one-class accuracy is what it is)
    one.reset('cpu')
    one.update(None, torch.zeros(3, 1), torch.zeros(3, dtype=torch.int64))
    assert one.compute(3) == 1.0
    with pytest.raises(BmnasError):                   # another class count into the same accumulator
        one.update(None, torch.zeros(3, 2), torch.zeros(3, dtype=torch.int64))


def test_the_option_is_read_beside_the_other_optional_arguments():
    from models.search._common import device_stats_option
    loop = _loop()
    meter = loop.AccuracyMeter()
    assert device_stats_option(types.SimpleNamespace(), meter) is None
    assert device_stats_option(types.SimpleNamespace(device_stats=False), meter) is None
    on = types.SimpleNamespace(device_stats=True)
    stats = device_stats_option(on, meter)
    assert stats is not None and device_stats_option(on, meter) is stats          # kept on the meter
    assert device_stats_option(on, object()) is None                               # a foreign meter: today's path
    f1 = loop.F1Meter('weighted', 0.3)
    first = device_stats_option(on, f1)
    f1.th = 0.5                                       # the meter changed: a new object, with the new threshold
    assert device_stats_option(on, f1) is not first and device_stats_option(on, f1).threshold == 0.5


def test_words_and_wide_heads():
    from bmnas.metrics import PhaseStats, stats_words
    assert stats_words(23) == 4 + 69 == R.words(23)
    stats = PhaseStats('f1', 'macro', 0.5)            # O > 128 has no launch: the torch restatement, also on the CPU
    stats.reset('cpu')
    x = torch.randn(4, 130)
    x[x.abs() < 1e-3] = 1.0
    y = (torch.randn(4, 130) > 0).float()
    stats.update(None, x, y)
    acc = R.tally_f1(R.empty(130), x.numpy(), y.numpy(), None, 0.0)
    assert stats.acc.numpy().tobytes() == acc.tobytes() and stats.compute(4) == R.f1(acc, 'macro')
    assert np.isfinite(stats.compute(4))
