"""-m gpu: one search epoch of models.search.train_searchable._loop.run over tiny synthetic loaders
(tests/helpers/loop_stubs.py) with args.unrolled: every dev batch runs DARTS' unrolled architecture step with one training
batch drawn from an iterator over the training loader that restarts when exhausted (3 dev batches, 2 train batches: one
restart); the weights come out of the dev phase bit-identical, alpha moves, and the train phase still replays its graph.
Without args.unrolled the same run is the loop as it always was."""
import logging
import os
import sys
import types

import pytest
import torch
from torch.utils.data import DataLoader

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, 'helpers'))

import loop_stubs as stubs  # noqa: E402


class _Counting:
    """A loader that counts how often it is iterated from the start."""

    def __init__(self, loader):
        self.loader, self.iters = loader, 0

    def __iter__(self):
        self.iters += 1
        return iter(self.loader)

    def __len__(self):
        return len(self.loader)

    def __getattr__(self, name):
        return getattr(self.loader, name)


def _args(save, **extra):
    class Args:
        pass

    a = Args()
    a.C, a.L, a.drpt = 32, 16, 0.1
    a.num_input_nodes, a.num_keep_edges, a.steps, a.multiplier = 6, 2, 2, 2
    a.node_steps, a.node_multiplier, a.num_outputs = 1, 1, 23
    a.batchsize, a.epochs = 8, 1
    a.eta_max, a.eta_min, a.Ti, a.Tm = 2e-3, 1e-5, 1, 2
    a.arch_learning_rate, a.arch_weight_decay, a.weight_decay = 3e-3, 1e-3, 1e-4
    a.f1_type = 'weighted'
    a.use_dataparallel = False
    a.hip_graph = True
    a.save = save
    for k, v in extra.items():
        setattr(a, k, v)
    return a


def _run(tmp_path, monkeypatch, **extra):
    """-> (loop.run.stats, the Architect, per-call records of Architect.step, the counting train loader)"""
    central = types.ModuleType('models.central')
    fake = types.ModuleType('models.central.mmimdb')
    fake.GP_VGG, fake.MaxOut_MLP = stubs.StubVGG, stubs.StubMLP
    central.mmimdb = fake
    monkeypatch.setitem(sys.modules, 'models.central', central)
    monkeypatch.setitem(sys.modules, 'models.central.mmimdb', fake)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    import models.search.mmimdb_darts_searchable as drv
    import models.search.train_searchable._loop as loop
    from models.search.darts.architect import Architect
    from models.search.darts.utils import create_exp_dir

    class Pinned(drv.Searchable_Image_Text_Net):
        def __init__(self, args, criterion):
            super().__init__(args, criterion)
            stubs.fill_state(self, 5)

    monkeypatch.setattr(drv, 'Searchable_Image_Text_Net', Pinned)
    calls, seen = [], {}
    step = Architect.step

    def recording_step(self, *a, **k):
        seen['architect'] = self
        arch = self.model.arch_parameters()
        weights = [p for p in self.model.parameters() if not any(p is t for t in arch)]
        before = ([p.detach().clone() for p in weights], [t.detach().clone() for t in arch])
        out = step(self, *a, **k)
        calls.append(dict(before=before, weights=[p.detach().clone() for p in weights],
                          arch=[t.detach().clone() for t in arch], kwargs=sorted(k), out=out))
        return out

    monkeypatch.setattr(Architect, 'step', recording_step)
    a = _args(str(tmp_path / 'exp'), **extra)
    create_exp_dir(a.save)
    loaders = {k: DataLoader(stubs.MMIMDBData(n, 40 + i), batch_size=8, shuffle=False, drop_last=False)
               for i, (k, n) in enumerate((('train', 16), ('dev', 24), ('test', 8)))}
    loaders['train'] = _Counting(loaders['train'])
    best_f1, genotype = drv.train_darts_model(loaders, a, torch.device('cuda:0'), logging.getLogger('bmnas-test'))
    torch.cuda.synchronize()
    assert 0.0 <= best_f1 <= 1.0 and len(genotype.edges) == 4
    return dict(loop.run.stats), seen['architect'], calls, loaders['train']


def test_unrolled_search_epoch(tmp_path, monkeypatch):
    stats, architect, calls, train = _run(tmp_path, monkeypatch, unrolled=True)
    print(stats)
    assert architect.unrolled and architect.unrolled_steps == 3 and architect.graph_replays == 0
    assert stats['unrolled_steps'] == 3 and len(calls) == 3
    # 3 dev batches over 2 train batches: the iterator over the training loader restarted once
    assert stats['unrolled_train_restarts'] == 1 and train.iters == 3              # the train phase + two passes
    assert all(c['kwargs'] == ['input_train', 'target_train'] and c['out'] is None for c in calls)
    # the weights: bit-identical before and after the dev phase (and after every architecture step)
    start = calls[0]['before'][0]
    assert len(start) > 0
    for c in calls:
        assert all(torch.equal(p, q) for p, q in zip(c['weights'], start))
    # alpha moved, at every step
    for c in calls:
        assert any(not torch.equal(x, y) for x, y in zip(c['arch'], c['before'][1]))
        assert all(bool(torch.isfinite(t).all()) for t in c['arch'])
    # the train phase still replays its graph; the metric forwards of the dev phase replay theirs
    assert stats['graph_replays'] > 0 and stats['forward_replays'] == 3
    assert stats.get('k_step_replays', 0) == 0 and stats.get('merged_metric_replays', 0) == 0


def test_without_unrolled_the_loop_is_untouched(tmp_path, monkeypatch):
    stats, architect, calls, train = _run(tmp_path, monkeypatch)
    print(stats)
    assert not architect.unrolled and architect._unrolled is None and architect.unrolled_steps == 0
    assert 'unrolled_steps' not in stats and 'unrolled_train_restarts' not in stats
    assert architect.graph_replays > 0 and stats['graph_replays'] > 0
    assert train.iters == 1                                                         # the train phase alone
    assert len(calls) == 3 and all(c['kwargs'] == ['metric'] for c in calls)
