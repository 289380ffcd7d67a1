"""-m gpu: the trainer loop with `args.device_stats` — phase loss, accuracy and F1 from bmnas.metrics.PhaseStats, one
tally per batch: inside the replay of a captured gradient-free forward, one launch behind every other batch.

`_loop.run`, status 'eval', two epochs, a ragged last batch in every phase, over the stock-torch MLP of
tests/test_accum_loop_gpu.py (CrossEntropyLoss + AccuracyMeter, BCEWithLogitsLoss + F1Meter('weighted', 0.3)) and over
the small hypernet of tests/avg_util.py.  An observer clones every batch's loss, output and labels; per phase the logged
loss is the float64 sum of those losses exactly, the accuracy is theirs exactly, the F1 is sklearn's f1_score of those
outputs within 1e-12 (host float64 on both sides; tests/test_stats_ref.py shows bit equality under this sklearn, the
margin covers another build's summation order) — after asserting that no observed logit lies within 1e-4 of logit(0.3),
where `sigmoid(x) > 0.3` in fp32 and `x > logit(0.3)` may disagree.  The classifiers' last layers are scaled up so that
the logits spread over tens of units and that band stays empty."""
import logging
import os
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, Dataset

import avg_util as au
import stats_ref as R
from gpu_util import dev
from test_accum_loop_gpu import MLP, _Feats, _NoPlot

pytestmark = pytest.mark.gpu

BATCH = 16
EPOCHS = 2


class _Pairs(Dataset):
    def __init__(self, n, seed, kind):
        g = torch.Generator().manual_seed(seed)
        self.a, self.b = torch.randn(n, 24, generator=g), torch.randn(n, 24, generator=g)
        self.y = (torch.randint(0, 5, (n,), generator=g) if kind == 'acc'
                  else (torch.rand(n, 5, generator=g) < 0.4).float())

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return [self.a[i], self.b[i]], self.y[i]


class _Watch:
    """run.observer + the unpack wrapper: every batch's (phase, how, loss, output, labels) and every phase's result"""

    def __init__(self, meter):
        self.meter, self.labels, self.batches, self.phases = meter, [], [], []

    def unpack(self, data, device):
        xs, y = [x.to(device) for x in data[0]], data[1].to(device)
        self.labels.append(y.clone())
        return xs, y

    def __call__(self, event, **info):
        if event == 'batch':
            self.batches.append((info['phase'], info['how'], info['loss'].detach().clone(),
                                 info['output'].detach().clone(), self.labels.pop(0)))
        elif event == 'phase':
            stats = self.meter.__dict__.get('_bmnas_phase_stats')
            self.phases.append((info['phase'], info['loss'], info['metric'], self.batches,
                                None if stats is None else stats.samples()))
            self.batches = []


def _run(monkeypatch, tmp_path, model, crit, opt, args, loaders, meter):
    import models.auxiliary.scheduler as sc
    import models.search.train_searchable._loop as loop
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    args.save = str(tmp_path / 'exp')
    os.makedirs(os.path.join(args.save, 'best'))
    sizes = {key: len(v.dataset) for key, v in loaders.items()}
    sched = sc.LRCosineAnnealingScheduler(1e-3, 1e-6, 1, 2, sizes['train'] / loaders['train'].batch_size)
    watch = _Watch(meter)
    monkeypatch.setattr(loop.run, 'observer', watch, raising=False)
    loop.run(model, None, crit, opt, sched, loaders, sizes, dev(), EPOCHS, logging.getLogger('bmnas-test'), _NoPlot(),
             args, 'eval', watch.unpack, meter, eval_phases=['train', 'test'], better=lambda new, old: new > old)
    torch.cuda.synchronize()
    assert watch.labels == [] and watch.batches == []
    return loop, watch, sizes


def _check_phases(watch, sizes, kind, with_samples=True):
    """-> batches seen.  Every phase's logged loss and metric against the observed batches."""
    from sklearn.metrics import f1_score
    thr = R.logit_threshold(0.3)
    total = 0
    assert [p[0] for p in watch.phases] == ['train', 'test'] * EPOCHS
    for phase, loss, metric, batches, samples in watch.phases:
        n = sizes[phase]
        assert sum(b[4].shape[0] for b in batches) == n and batches[-1][4].shape[0] < batches[0][4].shape[0]
        loss_sum = torch.zeros((), device=dev(), dtype=torch.float64)
        for _, _, l, _, y in batches:
            loss_sum += l.double() * y.size(0)
        assert loss == float(loss_sum) / n, (phase, loss, float(loss_sum) / n)
        out, lab = torch.cat([b[3] for b in batches]), torch.cat([b[4] for b in batches])
        if kind == 'acc':
            want = float((out.argmax(1) == lab).sum().double()) / n
            print(phase, 'loss', loss, 'acc', metric, want)
            assert metric == want
        else:
            assert R.band_empty(out.cpu().numpy(), thr), 'an observed logit lies within 1e-4 of logit(0.3)'
            want = float(f1_score(lab.cpu().numpy(), (torch.sigmoid(out) > 0.3).cpu().numpy(), average='weighted',
                                  zero_division=1))
            print(phase, 'loss', loss, 'F1', metric, want, abs(metric - want))
            assert abs(metric - want) <= 1e-12
        if with_samples:
            assert samples == n
        total += len(batches)
    return total


def _mlp(kind):
    from bmnas.optim import Adam
    torch.manual_seed(11)
    model = MLP().to(dev())
    with torch.no_grad():
        model.d.weight.mul_(40.0)                     # logits over tens of units: the threshold band stays empty
    opt = Adam([{'params': list(model.parameters())}], lr=1e-3, weight_decay=1e-4)
    loaders = {key: DataLoader(_Pairs(n, s, kind), batch_size=BATCH, shuffle=False)
               for key, n, s in (('train', 53, 1), ('test', 37, 2))}
    return model, opt, loaders


@pytest.mark.parametrize('kind', ['acc', 'f1'])
def test_mlp_phases_are_tallied_on_the_device(kind, tmp_path, monkeypatch):
    model, opt, loaders = _mlp(kind)
    import models.search.train_searchable._loop as loop_mod
    crit, meter = ((nn.CrossEntropyLoss(), loop_mod.AccuracyMeter()) if kind == 'acc'
                   else (nn.BCEWithLogitsLoss(), loop_mod.F1Meter('weighted', 0.3)))
    args = types.SimpleNamespace(hip_graph=True, device_stats=True)
    loop, watch, sizes = _run(monkeypatch, tmp_path, model, crit, opt, args, loaders, meter)
    stats = loop.run.stats
    batches = _check_phases(watch, sizes, kind)
    assert batches == EPOCHS * (4 + 3)
    assert stats['stat_launches'] + stats['stat_in_replay'] == batches, stats
    assert stats['stat_fallbacks'] == 0, stats
    # the test phase does not learn: its batches are replays of captured forwards (one graph per batch shape, the ragged
    # one included) that tally themselves; every learning batch — replayed or eager — takes the one launch behind it
    assert stats['stat_in_replay'] == stats['forward_replays'] == EPOCHS * 3, stats
    assert stats['graph_replays'] == EPOCHS * 3 and stats['eager_steps'] == EPOCHS, stats
    assert stats['stat_launches'] == stats['graph_replays'] + stats['eager_steps'], stats
    ps = meter._bmnas_phase_stats
    assert ps.fallbacks == 0 and ps.launches == stats['stat_launches']
    # the meter itself kept nothing
    assert not getattr(meter, 'preds', None) and float(getattr(meter, 'correct', torch.zeros(()))) == 0.0


def test_hypernet_phases_are_tallied_on_the_device(tmp_path, monkeypatch):
    import models.search.train_searchable._loop as loop_mod
    model, crit, opt, args = au.build(eta_max=1e-3, hip_graph=True, device_stats=True)
    with torch.no_grad():
        model.central_classifier.weight.mul_(40.0)
    loaders = {key: DataLoader(_Feats(n, s), batch_size=8, shuffle=False)
               for key, n, s in (('train', 20, 1), ('test', 28, 3))}
    meter = loop_mod.F1Meter('weighted', 0.3)
    loop, watch, sizes = _run(monkeypatch, tmp_path, model, crit, opt, args, loaders, meter)
    stats = loop.run.stats
    batches = _check_phases(watch, sizes, 'f1')
    assert batches == EPOCHS * (3 + 4)
    assert stats['stat_launches'] + stats['stat_in_replay'] == batches and stats['stat_fallbacks'] == 0, stats
    assert stats['stat_in_replay'] == stats['forward_replays'] == EPOCHS * 4, stats
    assert stats['stat_launches'] == stats['graph_replays'] + stats['eager_steps'] == EPOCHS * 3, stats


def test_without_the_option_the_loop_uses_its_meter(tmp_path, monkeypatch):
    import models.search.train_searchable._loop as loop_mod
    model, opt, loaders = _mlp('acc')
    meter = loop_mod.AccuracyMeter()
    updates = []
    inner = meter.update
    meter.update = lambda output, labels: (updates.append(labels.shape[0]), inner(output, labels))[1]
    args = types.SimpleNamespace(hip_graph=True)
    loop, watch, sizes = _run(monkeypatch, tmp_path, model, nn.CrossEntropyLoss(), opt, args, loaders, meter)
    stats = loop.run.stats
    assert [stats.get(k, 0) for k in ('stat_launches', 'stat_in_replay', 'stat_fallbacks')] == [0, 0, 0]
    assert '_bmnas_phase_stats' not in meter.__dict__
    assert _check_phases(watch, sizes, 'acc', with_samples=False) == len(updates) == EPOCHS * (4 + 3)
    assert float(meter.correct) / sizes['test'] == watch.phases[-1][2]
    # a foreign meter with the option set: the same
    args = types.SimpleNamespace(hip_graph=True, device_stats=True)

    class Mine(loop_mod.AccuracyMeter):
        pass

    mine = Mine()
    loop, watch, sizes = _run(monkeypatch, tmp_path / 'b', model, nn.CrossEntropyLoss(), opt, args, loaders, mine)
    assert loop.run.stats.get('stat_launches', 0) == 0 and '_bmnas_phase_stats' not in mine.__dict__
    assert float(mine.correct) / sizes['test'] == watch.phases[-1][2]


def test_building_a_graph_mid_phase_leaves_the_tally():
    from bmnas.graph import GraphedForward
    from bmnas.metrics import PhaseStats
    model, _, loaders = _mlp('f1')
    model.train()                                     # BatchNorm updates in the warm-ups: the state path is taken too
    crit = nn.BCEWithLogitsLoss()
    data = [([x.to(dev()) for x in d[0]], d[1].to(dev())) for d in loaders['test']]
    (xs0, y0), (xs1, y1) = data[0], data[1]
    stats, twin = PhaseStats('f1', 'weighted', 0.3), PhaseStats('f1', 'weighted', 0.3)
    for s in (stats, twin):
        s.reset(dev())
    with torch.no_grad():
        out0 = model(xs0)
        stats.update(crit(out0, y0), out0, y0)
        twin.update(crit(out0, y0), out0, y0)
    before = stats.acc.clone()
    assert int(before[2]) == BATCH and stats.launches == 1
    fwd = GraphedForward.try_build(model, crit, xs1, y1, stats=stats)
    assert fwd and fwd.stats is stats
    torch.cuda.synchronize()
    assert torch.equal(stats.acc, before) and stats.launches == 1 and stats.fallbacks == 0
    loss, out = fwd(xs1, y1)                          # the replay tallies its batch: no update() call
    twin.update(loss, out, y1)
    torch.cuda.synchronize()
    assert torch.equal(stats.acc, twin.acc) and int(stats.acc[2]) == 2 * BATCH and stats.launches == 1
    assert stats.samples() == 2 * BATCH and stats.compute(0) == twin.compute(0)
    # an accumulator that does not exist yet is allocated by the build and left empty; int labels under BCE shapes
    # that the launch does not take leave the graph without a tally
    fresh = PhaseStats('f1', 'weighted', 0.3)
    fresh.reset(dev())
    fwd2 = GraphedForward.try_build(model, crit, xs1, y1, stats=fresh)
    assert fwd2 and fwd2.stats is fresh and fresh.acc is not None and int(fresh.acc.abs().sum()) == 0
    assert fresh.launches == 0
    wrong = PhaseStats('acc')
    wrong.reset(dev())
    fwd3 = GraphedForward.try_build(model, crit, xs1, y1, stats=wrong)
    assert fwd3 and fwd3.stats is None and wrong.acc is None
    assert GraphedForward.try_build(model, crit, xs1, y1).stats is None
