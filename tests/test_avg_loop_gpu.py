"""-m gpu: weight averaging inside captured steps and in the found-stage trainer loop.

Captured: bmnas.graph.GraphedTrainStep(..., averaged=avg) at k = 1 and k = 2 — at k = 1 with seven parameter groups,
whose rows no longer fit the by-value blob, so that the copy-node fallback carries them, and at k = 1 with a frozen
layer under skip_frozen (the frozen tensors are copied eagerly in front of the first replay).  Five replays from
n_averaged == 0 must leave the averaged bits of an eager twin: the same steps issued one by one, each followed by an eager
update_parameters().  That asks for weight steps that are bit-equal between a replay and an eager step, so the model is a
small MLP of stock deterministic torch ops (Linear, BatchNorm1d — its running statistics and int64 counter are averaged /
copied too —, ReLU, MSE) under bmnas.optim.Adam: the test first asserts that the WEIGHTS of the two sides are bit-equal,
so a difference in the averages is the averaging's.  Two captured steps (k = 2 and k = 1) that share ONE averager and
one optimizer, replayed in turn, against the same eager twin; and `_loop.run` itself over that MLP with
args.steps_per_replay = 2 and an odd number of full batches per phase — the k-step graph, the one-step graph of the tail
and the eager ragged batch all feed one EMA — against a hand-driven eager twin, bit for bit.

Loop: train_mmimdb_track_f1(status='eval') on the synthetic loaders of tests/test_search_driver_gpu.py with
args.ema_decay: the test phase evaluates the averaged module (the outputs the loop saw in its last test phase are those
of run.averaged.module, not those of the live model), best_test_averaged.pt loads into torch's class, and without the
option run.stats and the saved files are what they were.  The loop does not capture the weight step of a Found_* network
today (with or without averaging), so its updates there are the eager ones; `_loop.run` over the small hypernet of
tests/avg_util.py with status 'eval' — whose step the loop does capture — shows the EMA updated INSIDE the replays, eagerly
on the ragged batches, and SWA snapshots taken at the end of the epochs from args.swa_start on."""
import logging
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import swa_utils
from torch.utils.data import DataLoader, Dataset

import avg_util as au
from gpu_util import assert_close_scaled, dev

pytestmark = pytest.mark.gpu

REPLAYS = 5


class MLP(nn.Module):
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


def _side(groups, frozen=False):
    from bmnas.optim import Adam, AveragedModel
    torch.manual_seed(11)
    model = MLP().to(dev())
    if frozen:
        for p in model.a.parameters():
            p.requires_grad_(False)
    ps = [p for p in model.parameters() if p.requires_grad]
    assert len(ps) == (8 if frozen else 10)
    if groups == 1:
        pg = [{'params': ps}]
    else:
        cuts = [0, 1, 2, 3, 4, 6, 8, 10]
        pg = [{'params': ps[a:b], 'lr': 1e-2 * (1 + i)} for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:]))]
    opt = Adam(pg, lr=1e-2, weight_decay=1e-4)
    avg = AveragedModel(model, decay=0.9, use_buffers=True, skip_frozen=frozen)
    if frozen:                                       # the first update must COPY the frozen tensors: spoil the copies
        with torch.no_grad():
            for p in avg.module.a.parameters():
                p.fill_(123.0)
    return model, opt, avg


def _batches(n):
    g = torch.Generator().manual_seed(5)
    return [([torch.randn(16, 24, generator=g).to(dev()), torch.randn(16, 24, generator=g).to(dev())],
             torch.randn(16, 5, generator=g).to(dev())) for _ in range(n)]


@pytest.mark.parametrize('k,groups,frozen', [(1, 1, False), (2, 1, False), (1, 7, False), (1, 1, True)],
                         ids=['k1', 'k2', 'k1-copy-node', 'k1-skip-frozen'])
def test_captured_updates_leave_the_bits_of_eager_steps_and_updates(k, groups, frozen):
    from bmnas import lib
    from bmnas.graph import GraphedTrainStep
    crit = nn.MSELoss()
    batches = _batches(REPLAYS * k)
    model_g, opt_g, avg_g = _side(groups, frozen)
    model_e, opt_e, avg_e = _side(groups, frozen)
    step = GraphedTrainStep.try_build(model_g, crit, opt_g, *batches[0], k=k, averaged=avg_g)
    assert isinstance(step, GraphedTrainStep) and step.in_graph_step and step.averaged is avg_g
    assert step.avg_plan is not None and avg_g.captures == 1 and avg_g._capturing is None
    assert len(step.avg_plan['order']) == (10 if frozen else 12) + 1      # parameters + running stats, + the counter
    # both kinds of tensors ride: k rows and the shared RAW row (num_batches_tracked), behind the optimizer's rows
    assert step.plan['extra'].nbytes == 32 * (k + 1)
    assert step.plan['hyp_all'].nbytes == k * 32 * groups + 32 * (k + 1)
    assert step.plan['poke'] == (step.plan['hyp_all'].nbytes <= lib.copy_blob_max()) == (groups == 1)
    assert int(avg_g.n_averaged) == 0 and avg_g._n == 0                   # the capture itself averaged nothing
    assert au.same_bits(au.tensors(model_g), au.tensors(model_e)) == []   # ... and moved nothing
    launched = avg_g.launches
    for r in range(REPLAYS):
        if k == 1:
            step(*batches[r])
        else:
            for j in range(k):
                step.stage(j, *batches[r * k + j])
            step.replay_staged()
        for xs, y in batches[r * k:(r + 1) * k]:
            opt_e.zero_grad()
            crit(model_e(xs), y).backward()
            opt_e.step()
            avg_e.update_parameters(model_e)
        assert au.same_bits(au.tensors(model_g), au.tensors(model_e)) == [], f'replay {r}: the weight steps differ'
        bad = au.same_bits(au.tensors(avg_g.module), au.tensors(avg_e.module))
        assert bad == [], f'replay {r}: averaged tensors {bad} differ'
        assert int(avg_g.n_averaged) == (r + 1) * k == avg_g._n
        if frozen:
            assert torch.equal(avg_g.module.a.weight, model_g.a.weight) and torch.equal(avg_g.module.a.bias, model_g.a.bias)
    # no eager launch: the updates were replayed (skip_frozen: the one copy of the frozen layer in front of replay 0)
    assert avg_g.launches == launched + (1 if frozen else 0)
    assert any(not np.array_equal(a, p) for a, p in zip(au.tensors(avg_g.module), au.tensors(model_g)))
    # an eager update in between (a ragged batch) and the next replay continue one count
    xs, y = batches[0]
    for model, opt, avg in ((model_g, opt_g, avg_g), (model_e, opt_e, avg_e)):
        opt.zero_grad()
        crit(model(xs), y).backward()
        opt.step()
        avg.update_parameters(model)
    del xs, y
    if k == 1:
        step(*batches[1])
        opt_e.zero_grad()
        crit(model_e(batches[1][0]), batches[1][1]).backward()
        opt_e.step()
        avg_e.update_parameters(model_e)
        assert au.same_bits(au.tensors(avg_g.module), au.tensors(avg_e.module)) == []
        assert int(avg_g.n_averaged) == REPLAYS + 2 == int(avg_e.n_averaged)


def _eager_step(model, opt, avg, crit, xs, y):
    opt.zero_grad()
    crit(model(xs), y).backward()
    opt.step()
    avg.update_parameters(model)


def test_two_captured_steps_share_one_averager():
    """A two-step graph and a one-step graph over ONE averager and one optimizer (what the trainer loop builds with
    steps_per_replay = 2), replayed in turn with an eager step in between: each writes its rows into its own plan."""
    from bmnas.graph import GraphedTrainStep
    crit = nn.MSELoss()
    batches = _batches(12)
    model_g, opt_g, avg_g = _side(1)
    model_e, opt_e, avg_e = _side(1)
    two = GraphedTrainStep.try_build(model_g, crit, opt_g, *batches[0], k=2, averaged=avg_g)
    one = GraphedTrainStep.try_build(model_g, crit, opt_g, *batches[0], averaged=avg_g)
    assert isinstance(two, GraphedTrainStep) and isinstance(one, GraphedTrainStep) and avg_g.captures == 2
    assert two.avg_plan is not one.avg_plan and two.avg_plan['slots'] == 2 and one.avg_plan['slots'] == 1
    i = 0
    for r in range(3):
        for j in range(2):
            two.stage(j, *batches[i + j])
        two.replay_staged()
        one(*batches[i + 2])
        _eager_step(model_g, opt_g, avg_g, crit, *batches[i + 3])         # (a ragged batch's eager step and update)
        for xs, y in batches[i:i + 4]:
            _eager_step(model_e, opt_e, avg_e, crit, xs, y)
        i += 4
        assert au.same_bits(au.tensors(model_g), au.tensors(model_e)) == [], f'round {r}: the weight steps differ'
        bad = au.same_bits(au.tensors(avg_g.module), au.tensors(avg_e.module))
        assert bad == [], f'round {r}: averaged tensors {bad} differ'
        assert int(avg_g.n_averaged) == i == avg_g._n
    # the shared RAW row of each plan is still one
    from bmnas import lib
    assert two.avg_plan['rows'][2]['flags'] == lib.AVG_RAW and one.avg_plan['rows'][1]['flags'] == lib.AVG_RAW
    with pytest.raises(lib.BmnasError, match='captured_plan'):
        avg_g.prepare_replay(None)


class _PairData(Dataset):
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.a, self.b, self.y = (torch.randn(n, 24, generator=g), torch.randn(n, 24, generator=g),
                                  torch.randn(n, 5, generator=g))

    def __len__(self):
        return len(self.y)

    def __getitem__(self, i):
        return [self.a[i], self.b[i]], self.y[i]


class _NegLoss:
    """The loop's meter interface: minus the summed squared error (larger is better)."""
    name = '-SSE'

    def reset(self, device):
        self.s = torch.zeros((), device=device, dtype=torch.float64)

    def update(self, output, labels):
        self.s -= ((output - labels) ** 2).sum()

    def compute(self, n):
        return float(self.s) / n


def test_loop_with_two_steps_per_replay_and_an_odd_number_of_full_batches(tmp_path, monkeypatch):
    """53 training samples in batches of 16: two full batches go through the two-step graph, the third through the
    one-step graph `one_batch` builds for the tail, the ragged fourth through an eager step — all into one EMA.  The
    averaged bits after two epochs are those of a hand-driven eager twin (same batches, same per-batch cosine rates)."""
    import models.auxiliary.scheduler as sc
    import models.search.train_searchable._loop as loop
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    from bmnas.optim import AveragedModel
    crit = nn.MSELoss()
    model_g, opt_g, _ = _side(1)
    model_e, opt_e, _ = _side(1)
    avg_e = AveragedModel(model_e, decay=0.75, use_buffers=True, skip_frozen=True)
    args = types.SimpleNamespace(save=str(tmp_path / 'exp'), hip_graph=True, steps_per_replay=2, ema_decay=0.75)
    os.makedirs(os.path.join(args.save, 'best'))
    loaders = {key: DataLoader(_PairData(n, s), batch_size=16, shuffle=False) for key, n, s in (('train', 53, 1), ('test', 16, 2))}
    sizes = {key: len(v.dataset) for key, v in loaders.items()}
    unpack = lambda data, device: ([x.to(device) for x in data[0]], data[1].to(device))
    mk_sched = lambda: sc.LRCosineAnnealingScheduler(1e-2, 1e-6, 1, 2, sizes['train'] / 16)
    epochs = 2
    loop.run(model_g, None, crit, opt_g, mk_sched(), loaders, sizes, dev(), epochs, logging.getLogger('bmnas-test'),
             _NoPlot(), args, 'eval', unpack, _NegLoss(), eval_phases=['train', 'test'], better=lambda new, old: new > old)
    stats, avg_g = loop.run.stats, loop.run.averaged
    assert stats['k_step_replays'] == epochs and stats['graph_replays'] == 3 * epochs, stats
    assert stats['averaged_updates'] == 4 * epochs == int(avg_g.n_averaged) and avg_g.captures == 2
    assert avg_g.launches == 2 + 1 + epochs           # captured calls of the two graphs, and the ragged batches' eager updates
    sched = mk_sched()
    model_e.train()
    for _ in range(epochs):
        for data in loaders['train']:
            xs, y = unpack(data, dev())
            sched.step()
            sched.update_optimizer(opt_e)
            _eager_step(model_e, opt_e, avg_e, crit, xs, y)
    assert au.same_bits(au.tensors(model_g), au.tensors(model_e)) == [], 'the weight steps differ'
    assert au.same_bits(au.tensors(avg_g.module), au.tensors(avg_e.module)) == []
    assert any(not np.array_equal(a, p) for a, p in zip(au.tensors(avg_g.module), au.tensors(model_g)))


# ---------------------------------------------------------------------------------------------------- the trainer loop
class _VGG(nn.Module):
    """Stand-in image backbone without host synchronisation, as in tests/test_search_driver_gpu.py; FROZEN here, as the
    real backbones of a found-stage run are."""

    def __init__(self, args):
        super().__init__()
        self.proj = nn.Linear(3 * 16 * 16, 512)
        for p in self.parameters():
            p.requires_grad_(False)

    def forward(self, image):
        f = self.proj(image.flatten(1)).relu()
        mk = lambda h, w: f[:, :, None, None].expand(-1, -1, h, w) * torch.linspace(
            0.5, 1.5, h * w, device=f.device).view(1, 1, h, w)
        return [mk(20, 32), mk(20, 32), mk(10, 16), mk(5, 8), f[:, :23]]


class _MLPText(nn.Module):
    def __init__(self, args):
        super().__init__()

    def forward(self, text):
        return [text[:, :64].relu(), text[:, :128].relu(), text[:, :23]]


class _DS(Dataset):
    def __init__(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        self.img = torch.randn(n, 3, 16, 16, generator=g)
        self.txt = torch.randn(n, 300, generator=g)
        self.lab = (torch.rand(n, 23, generator=g) < 0.2).float()

    def __len__(self):
        return len(self.lab)

    def __getitem__(self, i):
        return {'image': self.img[i], 'text': self.txt[i], 'label': self.lab[i]}


def _found_setup(tmp_path, monkeypatch, **options):
    central = types.ModuleType('models.central')
    fake = types.ModuleType('models.central.mmimdb')
    fake.GP_VGG, fake.MaxOut_MLP = _VGG, _MLPText
    central.mmimdb = fake
    monkeypatch.setitem(sys.modules, 'models.central', central)
    monkeypatch.setitem(sys.modules, 'models.central.mmimdb', fake)
    import models.auxiliary.scheduler as sc
    import models.search.mmimdb_darts_searchable as drv
    from bmnas import nn as bnn
    from bmnas.optim import Adam
    from models.search.darts.genotypes import Genotype, StepGenotype
    from models.search.darts.utils import create_exp_dir

    a = types.SimpleNamespace()
    a.C, a.L, a.drpt = 32, 16, 0.1
    a.num_input_nodes, a.num_keep_edges, a.steps, a.multiplier = 6, 2, 2, 2
    a.node_steps, a.node_multiplier, a.num_outputs = 2, 2, 23
    a.batchsize, a.epochs = 8, 2
    a.eta_max, a.eta_min, a.Ti, a.Tm = 1e-2, 1e-6, 1, 2
    a.f1_type = 'weighted'
    a.use_dataparallel = False
    a.save = str(tmp_path / 'exp')
    for key, v in options.items():
        setattr(a, key, v)
    create_exp_dir(a.save)
    genotype = Genotype(
        edges=[('skip', 1), ('skip', 4), ('skip', 0), ('skip', 5)],
        steps=[StepGenotype(inner_edges=[('skip', 0), ('skip', 1), ('skip', 2), ('skip', 0)],
                            inner_steps=['ScaleDotAttn', 'LinearGLU'], inner_concat=[2, 3]),
               StepGenotype(inner_edges=[('skip', 1), ('skip', 0), ('skip', 1), ('skip', 2)],
                            inner_steps=['ConcatFC', 'Sum'], inner_concat=[2, 3])],
        concat=[6, 7])
    torch.manual_seed(5)
    criterion = bnn.BCEWithLogitsLoss()
    model = drv.Found_Image_Text_Net(a, criterion, genotype)
    loaders = {key: DataLoader(_DS(n, s), batch_size=a.batchsize, shuffle=False, drop_last=False)
               for key, n, s in (('train', 20, 1), ('dev', 12, 2), ('test', 11, 3))}
    sizes = {key: len(v.dataset) for key, v in loaders.items()}
    model.to(dev())
    frozen = [p for p in model.parameters() if not p.requires_grad]
    assert len(frozen) == 2                                               # the image backbone's projection
    optimizer = Adam([p for p in model.parameters() if p.requires_grad], lr=a.eta_max, weight_decay=1e-4)
    scheduler = sc.LRCosineAnnealingScheduler(a.eta_max, a.eta_min, a.Ti, a.Tm, sizes['train'] / a.batchsize)
    return a, model, criterion, optimizer, scheduler, loaders, sizes, genotype, drv, frozen


def _train(setup):
    import models.search.train_searchable.mmimdb as tr
    from models.search.plot_genotype import Plotter
    a, model, criterion, optimizer, scheduler, loaders, sizes, genotype, _, _ = setup
    return tr.train_mmimdb_track_f1(model, None, criterion, optimizer, scheduler, loaders, sizes, dev(), a.epochs, False,
                                    logging.getLogger('bmnas-test'), Plotter(a), a, a.f1_type, 0.0, 0.3, 'eval')


def test_found_stage_loop_evaluates_and_saves_the_ema(tmp_path, monkeypatch):
    import models.search.train_searchable._loop as loop
    from bmnas.optim import AveragedModel
    setup = _found_setup(tmp_path, monkeypatch, ema_decay=0.5, hip_graph=True)
    a, model, criterion, _, _, loaders, _, genotype, drv, frozen = setup
    seen = []

    def observer(event, **info):
        if event == 'batch' and info['phase'] == 'test' and info['epoch'] == a.epochs - 1:
            seen.append(info['output'].detach().clone())

    monkeypatch.setattr(loop.run, 'observer', observer, raising=False)
    test_f1, _ = _train(setup)
    stats, avg = loop.run.stats, loop.run.averaged
    assert 0.0 <= test_f1 <= 1.0 and isinstance(avg, AveragedModel) and avg.use_buffers and avg.skip_frozen
    # every weight step of both learning phases was averaged: 2 epochs x (3 + 2) batches (eager updates: the loop does
    # not capture a Found_* weight step today)
    assert stats['averaged_updates'] == 10 == int(avg.n_averaged)
    assert stats['graph_replays'] + stats['eager_steps'] >= 10, stats
    # the frozen backbone was copied once and is in no later launch
    assert len(avg._main(model)) == len(avg.members(model, with_frozen=True)) - len(frozen)
    plans = [pl for key_, pl in avg._eager.items() if key_[1] == 'all']
    assert (plans or avg.captures) and all(len(pl['order']) == len([1 for t, _, _ in avg._main(model) if t.numel()])
                                           for pl in plans)
    assert stats['averaged_forwards'] == 2 * 2                            # the test phase: 2 epochs x (1 full + 1 ragged)
    # the outputs the loop's last test phase saw are the averaged module's, not the live model's
    avg.module.eval()
    model.eval()
    apart = 0.0
    with torch.no_grad():
        for out, d in zip(seen, loaders['test']):
            x = (d['text'].to(dev()), d['image'].to(dev()))
            assert_close_scaled('test phase output', out, avg.module(x), rel=1e-5)
            apart = max(apart, float((out - model(x)).abs().max() / out.abs().max()))
    assert len(seen) == 2 and apart > 1e-4, apart                         # (10 x the tolerance of the comparison above)
    # best_test_averaged.pt next to best_test_model.pt, in torch's format
    best = os.path.join(a.save, 'best')
    assert sorted(os.listdir(best)) == ['best_test_averaged.pt', 'best_test_genotype.pkl', 'best_test_model.pt']
    theirs = swa_utils.AveragedModel(drv.Found_Image_Text_Net(a, criterion, genotype), use_buffers=True)
    missing = theirs.load_state_dict(torch.load(os.path.join(best, 'best_test_averaged.pt')))
    assert not missing.missing_keys and not missing.unexpected_keys and int(theirs.n_averaged) > 0
    live = torch.load(os.path.join(best, 'best_test_model.pt'))
    assert any(not torch.equal(v.cpu(), theirs.module.state_dict()[key_].cpu()) for key_, v in live.items()
               if v.is_floating_point())


def test_deepcopy_of_a_found_network_computes_its_forward(tmp_path, monkeypatch):
    """copy.deepcopy(Found_Image_Text_Net): the copy's forward is the original's, eagerly and through GraphedForward (two
    passes of one model agree to fp32 round-off — the split-K atomics —, the 1e-5 of tests/test_graph_forward_gpu.py)."""
    import copy
    from bmnas.graph import GraphedForward
    _, model, criterion, _, _, loaders, _, _, _, _ = _found_setup(tmp_path, monkeypatch)
    twin = copy.deepcopy(model)
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(twin.parameters(), model.parameters()))
    model.eval()
    twin.eval()
    d = next(iter(loaders['test']))
    xs, y = [d['text'].to(dev()), d['image'].to(dev())], d['label'].to(dev())
    with torch.no_grad():
        want, got = model(xs), twin(xs)
    assert_close_scaled('eager forward of the copy', got, want, rel=1e-5)
    fwd = GraphedForward.try_build(twin, twin.criterion, xs, y)
    assert isinstance(fwd, GraphedForward)
    loss_t, out_t = fwd(xs, y)
    assert_close_scaled('replayed forward of the copy', out_t, want, rel=1e-5)
    assert_close_scaled('replayed loss of the copy', loss_t.reshape(1), criterion(want, y).reshape(1), rel=1e-5)
    with torch.no_grad():
        model.central_classifier.bias.add_(1.0)                         # the copy is a model of its own
    assert_close_scaled('the copy after the original moved', fwd(xs, y)[1], want, rel=1e-5)


def test_found_stage_loop_without_the_options_is_what_it_was(tmp_path, monkeypatch):
    import models.search.train_searchable._loop as loop
    setup = _found_setup(tmp_path, monkeypatch, hip_graph=True)
    a = setup[0]
    test_f1, _ = _train(setup)
    assert 0.0 <= test_f1 <= 1.0
    assert loop.run.averaged is None
    assert set(loop.run.stats) == {'graph_replays', 'eager_steps', 'forward_replays', 'k_step_replays'}
    assert sorted(os.listdir(os.path.join(a.save, 'best'))) == ['best_test_genotype.pkl', 'best_test_model.pt']


def test_the_options_are_refused_in_a_search(tmp_path, monkeypatch):
    import models.search.train_searchable.mmimdb as tr
    from models.search.plot_genotype import Plotter
    setup = _found_setup(tmp_path, monkeypatch, ema_decay=0.9)
    a, model, criterion, optimizer, scheduler, loaders, sizes, _, _, _ = setup
    with pytest.raises(ValueError, match='would not belong to the current alphas'):
        tr.train_mmimdb_track_f1(model, None, criterion, optimizer, scheduler, loaders, sizes, dev(), 1, False,
                                 logging.getLogger('bmnas-test'), Plotter(a), a, a.f1_type, 0.0, 0.3, 'search')


# ------------------------------------------------------------------------- the loop over a model whose step it captures
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


class _NoPlot:
    def plot(self, *a, **k):
        pass


def _run_hypernet(tmp_path, **options):
    import models.auxiliary.scheduler as sc
    import models.search.train_searchable._loop as loop
    model, crit, opt, args = au.build(eta_max=1e-2, hip_graph=True, **options)
    args.save = str(tmp_path / 'exp')
    os.makedirs(os.path.join(args.save, 'best'))
    loaders = {key: DataLoader(_Feats(n, s), batch_size=8, shuffle=False) for key, n, s in (('train', 20, 1), ('test', 8, 2))}
    sizes = {key: len(v.dataset) for key, v in loaders.items()}
    sched = sc.LRCosineAnnealingScheduler(1e-2, 1e-6, 1, 2, sizes['train'] / 8)
    unpack = lambda data, device: ([x.to(device) for x in data[0]], data[1].to(device))
    best = loop.run(model, None, crit, opt, sched, loaders, sizes, dev(), 3, logging.getLogger('bmnas-test'), _NoPlot(),
                    args, 'eval', unpack, loop.F1Meter('weighted', 0.3), eval_phases=['train', 'test'],
                    better=lambda new, old: new > old)
    return model, best, loop.run.stats, loop.run.averaged, args


def test_loop_updates_the_ema_inside_the_replays(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    model, best, stats, avg, args = _run_hypernet(tmp_path, ema_decay=0.9)
    # 3 epochs x (2 full batches: replays, 1 ragged batch: an eager step)
    assert stats['graph_replays'] == 6 and stats['averaged_updates'] == 9 == int(avg.n_averaged), stats
    assert avg.captures == 1
    assert avg.launches == 1 + 3                      # the captured call, and the three ragged batches' eager updates
    assert stats['averaged_forwards'] == 3 and best['best_test'] is not None
    assert os.path.exists(os.path.join(args.save, 'best', 'best_test_averaged.pt'))
    assert any(not torch.equal(a, p) for a, p in zip(avg.module.parameters(), model.parameters()))


def test_loop_takes_swa_snapshots_from_swa_start_on(tmp_path, monkeypatch):
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    model, best, stats, avg, args = _run_hypernet(tmp_path, swa_start=1)
    assert stats['graph_replays'] == 6 and stats['averaged_updates'] == 2 == int(avg.n_averaged), stats
    assert avg.decay is None and avg.captures == 0 and avg.launches == 2           # eager, one per epoch from epoch 1 on
    assert stats['averaged_forwards'] == 2            # epoch 0's test phase had no snapshot yet: the live model
