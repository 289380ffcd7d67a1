"""-m gpu: gradient accumulation in the trainer loop (`args.accum_steps`).

`_loop.run` with status 'eval' over the small hypernet of tests/avg_util.py — whose weight step the loop captures —, two
epochs, 5 batches in each learning phase and accum_steps = 2: 3 optimizer steps per learning phase (two replays of the
accumulate=2 graph and ONE eager accumulated step over the tail: a shorter last batch in `train`, a single full batch in
`dev`), the scheduler advanced once per batch, the EMA once per optimizer step, the observer once per micro-batch.

And `_loop.run` over a small MLP of stock deterministic torch ops, where a replay and an eager step agree bit for bit:
after two epochs of 4 batches (a full group, then a full batch + a ragged one) the weights and the EMA hold the bits of a
hand-driven eager twin — per-batch cosine rates, each step taken with the rates after its group's last batch, weights
n_i / N."""
import logging
import os
import types

import pytest
import torch
import torch.nn as nn
from torch.utils.data import DataLoader, Dataset

import avg_util as au
from gpu_util import dev

pytestmark = pytest.mark.gpu


class MLP(nn.Module):
    """Stock deterministic torch ops: a replayed step and an eager one agree bit for bit (tests/test_avg_loop_gpu.py)."""

    def __init__(self):
        super().__init__()
        self.a, self.bn, self.b, self.c, self.d = (nn.Linear(24, 40), nn.BatchNorm1d(40), nn.Linear(40, 33),
                                                    nn.Linear(33, 17), nn.Linear(17, 5))
        # what _loop.run reads of a hypernet besides its forward (no parameters in either)
        self.reshape_layers, self.fusion_net = nn.ModuleList(), nn.Identity()

    def genotype(self):
        return 'mlp'

    def forward(self, xs):
        h = torch.relu(self.bn(self.a(xs[0] + xs[1])))
        return self.d(torch.relu(self.c(torch.relu(self.b(h)))))


class _PairData(Dataset):
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.a, self.b, self.y = (torch.randn(n, 24, generator=g), torch.randn(n, 24, generator=g),
                                  torch.randn(n, 5, generator=g))

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return [self.a[i], self.b[i]], self.y[i]


class _Feats(Dataset):
    """The hypernet's input features and multi-hot labels, sample by sample."""

    def __init__(self, n, seed):
        import dp_child as base
        from oracle import synth
        cfg = base.cfg_small()
        self.xs = [x.clone() for x in synth.make_inputs(cfg, n, seed)]
        self.y = synth.make_labels('bce', n, base.NOUT, seed)

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return [x[i] for x in self.xs], self.y[i]


class _NegLoss:
    """The loop's meter interface: minus the summed squared error (larger is better)."""
    name = '-SSE'

    def reset(self, device):
        self.s = torch.zeros((), device=device, dtype=torch.float64)

    def update(self, output, labels):
        self.s -= ((output - labels) ** 2).sum()

    def compute(self, n):
        return float(self.s) / n


class _NoPlot:
    def plot(self, *a, **k):
        pass


def _counting(scheduler):
    calls = [0]
    inner = scheduler.step

    def step():
        calls[0] += 1
        return inner()

    scheduler.step = step
    return calls


def test_found_stage_run_takes_one_step_per_group(tmp_path, monkeypatch):
    import models.auxiliary.scheduler as sc
    import models.search.train_searchable._loop as loop
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    model, crit, opt, args = au.build(eta_max=1e-2, hip_graph=True, accum_steps=2, ema_decay=0.9)
    args.save = str(tmp_path / 'exp')
    os.makedirs(os.path.join(args.save, 'best'))
    # train: 4 full batches + one of 4 samples; dev: 5 full batches; test: one full batch
    loaders = {key: DataLoader(_Feats(n, s), batch_size=8, shuffle=False)
               for key, n, s in (('train', 36, 1), ('dev', 40, 2), ('test', 8, 3))}
    sizes = {key: len(v.dataset) for key, v in loaders.items()}
    sched = sc.LRCosineAnnealingScheduler(1e-2, 1e-6, 1, 2, sizes['train'] / 8)
    calls = _counting(sched)
    unpack = lambda data, device: ([x.to(device) for x in data[0]], data[1].to(device))
    events = []

    def observer(event, **info):
        if event == 'batch':
            events.append((info['phase'], info['learn'], info['how'], int(info['output'].shape[0])))

    monkeypatch.setattr(loop.run, 'observer', observer, raising=False)
    epochs = 2
    before = [p.detach().clone() for g in opt.param_groups for p in g['params']]
    loop.run(model, None, crit, opt, sched, loaders, sizes, dev(), epochs, logging.getLogger('bmnas-test'), _NoPlot(),
             args, 'eval', unpack, loop.F1Meter('weighted', 0.3), eval_phases=['train', 'dev', 'test'],
             better=lambda new, old: new > old)
    stats, avg = loop.run.stats, loop.run.averaged
    torch.cuda.synchronize()
    # 2 epochs x 2 learning phases x ceil(5 / 2) optimizer steps
    assert stats['accum_groups'] == 12 and stats['accum_replays'] == 8, stats
    steps = {float(st['step']) for st in opt.state_dict()['state'].values()}
    assert steps == {12.0}, steps
    assert stats['averaged_updates'] == 12 == int(avg.n_averaged), stats
    assert avg.captures == 1 and avg.launches == 1 + 4            # the captured call, and the four eager tails' updates
    # ... over 20 micro-batches: 16 through replays, 4 eagerly (the tails), none as a single step of its own
    assert stats['graph_replays'] == 16 and stats['eager_steps'] == 4 and stats['k_step_replays'] == 0, stats
    assert calls[0] == 20                                         # the schedule advances once per BATCH
    learn = [e for e in events if e[1]]
    assert len(learn) == 20
    per_epoch = [('train', True, 'graph', 8)] * 4 + [('train', True, 'eager', 4)] + \
                [('dev', True, 'graph', 8)] * 4 + [('dev', True, 'eager', 8)]
    assert learn == per_epoch * epochs
    assert stats['forward_replays'] == epochs                     # the test phase: gradient-free replays, as ever
    after = [p.detach() for g in opt.param_groups for p in g['params']]
    assert sum(int(not torch.equal(a, b)) for a, b in zip(after, before)) > 20
    assert all(bool(torch.isfinite(a).all()) for a in after)


def _mlp_side():
    from bmnas.optim import Adam
    torch.manual_seed(11)
    model = MLP().to(dev())
    opt = Adam([{'params': list(model.parameters())}], lr=1e-2, weight_decay=1e-4)
    return model, opt


def test_loop_with_accumulation_leaves_the_bits_of_an_eager_twin(tmp_path, monkeypatch):
    import models.auxiliary.scheduler as sc
    import models.search.train_searchable._loop as loop
    from bmnas.optim import AveragedModel, GradAccumulator, accum_weights
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    crit = nn.MSELoss()
    model_g, opt_g = _mlp_side()
    model_e, opt_e = _mlp_side()
    avg_e = AveragedModel(model_e, decay=0.75, use_buffers=True, skip_frozen=True)
    args = types.SimpleNamespace(save=str(tmp_path / 'exp'), hip_graph=True, accum_steps=2, ema_decay=0.75)
    os.makedirs(os.path.join(args.save, 'best'))
    loaders = {key: DataLoader(_PairData(n, s), batch_size=16, shuffle=False)
               for key, n, s in (('train', 53, 1), ('test', 16, 2))}
    sizes = {key: len(v.dataset) for key, v in loaders.items()}
    unpack = lambda data, device: ([x.to(device) for x in data[0]], data[1].to(device))
    mk_sched = lambda: sc.LRCosineAnnealingScheduler(1e-2, 1e-6, 1, 2, sizes['train'] / 16)
    epochs = 2
    loop.run(model_g, None, crit, opt_g, mk_sched(), loaders, sizes, dev(), epochs, logging.getLogger('bmnas-test'),
             _NoPlot(), args, 'eval', unpack, _NegLoss(), eval_phases=['train', 'test'], better=lambda new, old: new > old)
    stats, avg_g = loop.run.stats, loop.run.averaged
    # per epoch: (16, 16) one replay, (16, 5) one eager accumulated step
    assert stats['accum_groups'] == 2 * epochs and stats['accum_replays'] == epochs, stats
    assert stats['graph_replays'] == 2 * epochs and stats['eager_steps'] == 2 * epochs, stats
    assert stats['averaged_updates'] == 2 * epochs == int(avg_g.n_averaged)
    # the twin: everything eager
    sched = mk_sched()
    acc = GradAccumulator(opt_e)
    model_e.train()
    for _ in range(epochs):
        batches = [unpack(data, dev()) for data in loaders['train']]
        for group in (batches[:2], batches[2:]):
            ws = accum_weights([y.size(0) for _, y in group], 'mean')
            assert ws == ([0.5, 0.5] if group[1][1].size(0) == 16 else [16 / 21, 5 / 21])
            for (xs, y), w in zip(group, ws):
                sched.step()
                sched.update_optimizer(opt_e)
                acc.add([g.contiguous() for g in torch.autograd.grad(crit(model_e(xs), y), acc.tensors)], w)
            acc.combine()
            opt_e.step()                                          # with the rates after the group's last batch
            avg_e.update_parameters(model_e)
    assert au.same_bits(au.tensors(model_g), au.tensors(model_e)) == [], 'the weight steps differ'
    assert au.same_bits(au.tensors(avg_g.module), au.tensors(avg_e.module)) == []
