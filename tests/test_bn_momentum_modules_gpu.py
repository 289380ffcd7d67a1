"""-m gpu: nn.BatchNorm1d.momentum through the modules — the search cell, an NTU-shaped cell (out_conv BatchNorm), a found
network (stand-alone conv + BatchNorm tails, ConvBnReluLnFn), the grouped reshape layers — then bmnas.optim.update_bn and
the trainer option args.swa_update_bn.

Where the expectation comes from.  NOT from the new code path: a twin model with momentum 0.1 and fresh buffers
(r0: mean 0, variance 1) sees the same batch through the unchanged default path, which the parity suite pins to the
oracle; its batch statistics follow in float64 as s = (r - 0.9 r0) / 0.1, and a model with momentum m must hold
(1 - m) r0 + m s in every BatchNorm buffer — gpu_util's forward bound, 1e-4 of the element + 1e-4 of the scale (the
division by 0.1 amplifies the twin's fp32 round-off ten times, to about 1e-6).  Cumulative momentum (None) over three
batches: the mean of the three s of three fresh twins, counters 3; update_bn over a loader of those batches (the last one
ragged), graphed and eager: the same means.

Logits and gradients of the twin and of the model under test: momentum reaches nothing but the running buffers, so they
are the same computation.  Bit for bit where a step is reproducible at all — the MM-IMDB hypernet in deterministic mode
(bmnas.cell.DETERMINISTIC, which also sends its BatchNorms through bmnas_bn_finalize_ex; tests/test_deterministic_gpu.py
pins that two runs are bit-identical there).  In the default mode two runs of ONE model already differ in the last bits
(the order of fp32 atomic additions — split-K outputs, reductions —: tests/test_deterministic_gpu.py
test_the_default_mode_is_not_bit_reproducible; measured here on an MI355X: twin and model under test differ in the last
digit of the logits at 16 columns per channel, for all three networks), so there the comparison takes the bound the
suite already uses for two passes of one model, 1e-5 of scale for the logits (tests/test_graph_forward_gpu.py), and ten
times that for the gradients, which pass through the network once more.  The launch-level statement — `out` and `chan`
bit-identical in every mode — is tests/test_bn_momentum_gpu.py's.  Dropout is an identity (gpu_util.set_mode
'train_nodrop')."""
import logging

import pytest
import torch
import torch.nn as nn

from gpu_util import assert_close_scaled, build_found_net, build_search_net, dev
from oracle import fusion_oracle as fo
from oracle import synth

pytestmark = pytest.mark.gpu

SEED, NOUT, M_TEST = 6, 23, 0.01
KINDS = ['mmimdb', 'ntu', 'found']


def _cfg(kind):
    if kind == 'mmimdb':                                  # the small MM-IMDB hypernet of tests/helpers/dp_child.py
        return fo.Cfg({**fo.CONFIGS['mmimdb'], 'C': 32, 'drpt': 0.0})
    return fo.make_cfg(N=3, C=32, L=8, S=2, M=2, ns=2, nm=2, drpt=0.0)


class _Net(nn.Module):
    def __init__(self, kind):
        super().__init__()
        from bmnas import nn as bnn
        cfg = _cfg(kind)
        if kind == 'found':
            self.fusion_net = build_found_net(cfg, fo.network_genotype(synth.make_arch(cfg, SEED), cfg), SEED,
                                              'train_nodrop')
        else:
            self.fusion_net = build_search_net(cfg, SEED, 'train_nodrop')
        self.central_classifier = bnn.Linear(cfg.M * cfg.C * cfg.L, NOUT).to(dev())
        cw, cb = synth.make_classifier(cfg, NOUT, SEED)
        self.central_classifier.weight.data.copy_(cw)
        self.central_classifier.bias.data.copy_(cb)
        self.cfg = cfg

    def forward(self, xs):
        return self.fusion_net.forward_classified(list(xs), self.central_classifier)


def _bns(model):
    return {n: m for n, m in model.named_modules() if isinstance(m, nn.BatchNorm1d)}


def _make(kind, momentum=0.1):
    net = _Net(kind)
    for bn in _bns(net).values():
        bn.reset_running_stats()                          # fresh buffers r0: mean 0, variance 1, counter 0
        bn.momentum = momentum
    return net


def _batch(cfg, b, seed):
    xs = [x[:b].contiguous().to(dev()) for x in synth.make_inputs(cfg, 8, seed)]
    return xs, synth.make_labels('bce', 8, NOUT, seed)[:b].contiguous().to(dev())


def _step(model, xs, y):
    from bmnas import nn as bnn
    model.zero_grad(set_to_none=True)
    logits = model(xs)
    bnn.BCEWithLogitsLoss()(logits, y).backward()
    torch.cuda.synchronize()
    return logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


def _batch_stats(twin):
    """s = (r - 0.9 r0) / 0.1 in float64 from a twin that saw ONE batch from fresh buffers"""
    out = {}
    for n, bn in _bns(twin).items():
        assert int(bn.num_batches_tracked) == 1 and bn.momentum == 0.1
        out[n] = (bn.running_mean.double().cpu() / 0.1, (bn.running_var.double().cpu() - 0.9) / 0.1)
    return out


def _twin_stats(kind, xs, y):
    twin = _make(kind)
    out = _step(twin, xs, y)
    return _batch_stats(twin), out


def _check_buffers(model, want, counter):
    bns = _bns(model)
    assert bns and set(bns) == set(want)
    for n, bn in bns.items():
        assert_close_scaled(n + '.running_mean', bn.running_mean, want[n][0])
        assert_close_scaled(n + '.running_var', bn.running_var, want[n][1])
        assert int(bn.num_batches_tracked) == counter, (n, int(bn.num_batches_tracked))


@pytest.mark.parametrize('kind', KINDS)
def test_momentum_reaches_the_running_buffers_and_nothing_else(kind):
    cfg = _cfg(kind)
    xs, y = _batch(cfg, 16 // cfg.L, 1)
    s, (logits0, grads0) = _twin_stats(kind, xs, y)
    model = _make(kind, M_TEST)
    logits, grads = _step(model, xs, y)
    assert_close_scaled('logits', logits, logits0, rel=1e-5)
    assert set(grads) == set(grads0) and len(grads) > 10
    for n in grads:
        assert_close_scaled(n + '.grad', grads[n], grads0[n], rel=1e-4)
    _check_buffers(model, {n: (M_TEST * m, (1.0 - M_TEST) + M_TEST * v) for n, (m, v) in s.items()}, 1)


@pytest.fixture
def deterministic():
    from bmnas import cell as K
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0 (switch matrix): the deterministic mode covers the fused-head path only')
    prev = K.DETERMINISTIC
    K.DETERMINISTIC = True
    K.apply_deterministic()
    yield K
    K.DETERMINISTIC = prev
    K.apply_deterministic()


def _fused_step(model, xs, y):
    """the step the way Searchable_*.forward issues it: the criterion evaluated by the head's backward launch"""
    from bmnas import nn as bnn
    model.zero_grad(set_to_none=True)
    with bnn.fused_criterion():
        logits = model(xs)
        loss = bnn.BCEWithLogitsLoss()(logits, y)
    loss.backward()
    torch.cuda.synchronize()
    return logits.detach(), {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize('momentum', [M_TEST, None])
def test_deterministic_mode_is_bit_identical_whatever_the_momentum(deterministic, momentum):
    """the MM-IMDB hypernet through bmnas_bn_finalize_ex: logits and every gradient bit for bit, the buffers by the rule"""
    cfg = _cfg('mmimdb')
    xs, y = _batch(cfg, 6, 2)
    twin = _make('mmimdb')
    logits0, grads0 = _fused_step(twin, xs, y)
    s = _batch_stats(twin)
    model = _make('mmimdb', momentum)
    logits, grads = _fused_step(model, xs, y)
    assert torch.equal(logits, logits0)
    assert set(grads) == set(grads0) and len(grads) > 10
    differ = [n for n in grads if not torch.equal(grads[n], grads0[n])]
    assert not differ, differ[:6]
    m = 1.0 if momentum is None else momentum                 # (None from a fresh counter: 1 / 1)
    _check_buffers(model, {n: (m * mean, (1.0 - m) + m * var) for n, (mean, var) in s.items()}, 1)


def _three_batches(cfg):
    return [_batch(cfg, b, 10 + i) for i, b in enumerate((3, 3, 2))]


def _mean_stats(kind, batches):
    per = [_twin_stats(kind, xs, y)[0] for xs, y in batches]
    return {n: (sum(p[n][0] for p in per) / len(per), sum(p[n][1] for p in per) / len(per)) for n in per[0]}


@pytest.mark.parametrize('kind', KINDS)
def test_cumulative_momentum_over_three_forwards(kind):
    batches = _three_batches(_cfg(kind))
    want = _mean_stats(kind, batches)
    model = _make(kind, None)
    with torch.no_grad():
        for bn in _bns(model).values():                   # the plain mean does not depend on what the buffers held
            bn.running_mean.fill_(3.0)
            bn.running_var.fill_(7.0)
        for xs, _ in batches:
            model(xs)
    _check_buffers(model, want, 3)


@pytest.mark.parametrize('graph', [True, False])
@pytest.mark.parametrize('kind', KINDS)
def test_update_bn(kind, graph):
    from bmnas import nn as bnn
    from bmnas.optim import update_bn
    batches = _three_batches(_cfg(kind))
    want = _mean_stats(kind, batches)
    model = _make(kind, M_TEST)
    xs, y = batches[0]
    _step(model, xs, y)                                   # some history in the buffers, which the pass must forget
    model.eval()
    report = update_bn(batches, model, dev(), unpack=lambda batch, device: batch, criterion=bnn.BCEWithLogitsLoss(),
                       graph=graph)
    torch.cuda.synchronize()
    _check_buffers(model, want, 3)
    assert report['batches'] == 3 and report['replays'] + report['eager'] == 3
    if graph:
        assert report['replays'] >= 1 and report['eager'] >= 1, report        # two replays, the ragged batch eagerly
    else:
        assert report['replays'] == 0
    assert not model.training and all(bn.momentum == M_TEST and not bn.training for bn in _bns(model).values())


def test_stacked_batchnorms_must_agree_on_momentum():
    from bmnas import lib
    from models.search.darts.node_operations import NodeMixedOp
    model = _make('mmimdb')
    op = next(m for m in model.modules() if isinstance(m, NodeMixedOp))
    op._kind('LinearGLU').bn.momentum = 0.01
    xs, y = _batch(model.cfg, 2, 1)
    with pytest.raises(lib.BmnasError, match=r'LinearGLU\.bn has momentum=0\.01 and ConcatFC\.bn has momentum=0\.1'):
        model(xs)
    torch.cuda.synchronize()
    for n, bn in _bns(model).items():                     # before any launch: nothing was counted
        assert int(bn.num_batches_tracked) == 0, n


def test_grouped_reshape_layers_take_a_momentum_each():
    from models.auxiliary.aux_models import ReshapeInputLayer_MMIMDB, reshape_tails
    import types
    args = types.SimpleNamespace(drpt=0.0)
    C, L, b = 32, 16, 4
    c_ins = (64, 128, 32)
    g = torch.Generator().manual_seed(3)
    pooled = [torch.randn(b, c, L, generator=g).to(dev()) for c in c_ins]

    def layers(momenta):
        torch.manual_seed(4)
        ls = [ReshapeInputLayer_MMIMDB(c, C, L, args).to(dev()).train() for c in c_ins]
        for layer, m in zip(ls, momenta):
            layer.bn.momentum = m
        return ls

    twins = layers((0.1, 0.1, 0.1))
    outs0 = reshape_tails(twins, [p.clone().requires_grad_(True) for p in pooled])
    under = layers((M_TEST, None, 0.1))
    ins = [p.clone().requires_grad_(True) for p in pooled]
    outs = reshape_tails(under, ins)
    assert all(type(o.grad_fn).__name__ == 'ReshapeGroupFnBackward' for o in outs + outs0)
    sum(o.square().sum() for o in outs).backward()
    torch.cuda.synchronize()
    for i, (layer, twin, m) in enumerate(zip(under, twins, (M_TEST, 1.0, 0.1))):      # None from a fresh counter: 1 / 1
        assert torch.equal(outs[i], outs0[i]) and ins[i].grad is not None
        s_mean, s_var = twin.bn.running_mean.double() / 0.1, (twin.bn.running_var.double() - 0.9) / 0.1
        assert_close_scaled(f'layer {i} running_mean', layer.bn.running_mean, m * s_mean)
        assert_close_scaled(f'layer {i} running_var', layer.bn.running_var, (1.0 - m) + m * s_var)
        assert int(layer.bn.num_batches_tracked) == 1


# ------------------------------------------------------------------------------------------------------- trainer loop
def test_loop_recomputes_the_averaged_statistics(tmp_path, monkeypatch):
    import models.search.train_searchable._loop as loop
    from test_avg_loop_gpu import _found_setup, _train
    setup = _found_setup(tmp_path, monkeypatch, swa_start=0, swa_update_bn=True)
    a, model, _, _, _, loaders, _, _, _, _ = setup
    test_f1, _ = _train(setup)
    stats, avg = loop.run.stats, loop.run.averaged
    assert 0.0 <= test_f1 <= 1.0 and not avg.use_buffers
    assert stats['update_bn_passes'] >= 1 and stats['averaged_updates'] == a.epochs, stats
    counters = {n: int(bn.num_batches_tracked) for n, bn in _bns(avg.module).items()}
    assert counters and set(counters.values()) == {len(loaders['train'])}, counters
    momenta = {bn.momentum for bn in _bns(avg.module).values()}
    assert momenta == {0.1} and not avg.module.training


def test_loop_without_the_option_is_what_it_was(tmp_path, monkeypatch):
    import models.search.train_searchable._loop as loop
    from test_avg_loop_gpu import _found_setup, _train
    setup = _found_setup(tmp_path, monkeypatch, swa_start=0)
    _train(setup)
    assert sorted(loop.run.stats) == ['averaged_forwards', 'averaged_updates', 'eager_steps', 'forward_replays',
                                      'graph_replays', 'k_step_replays'], loop.run.stats
    assert loop.run.averaged.use_buffers
    logging.getLogger('bmnas-test').info('stats %s', loop.run.stats)
