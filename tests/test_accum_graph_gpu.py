"""-m gpu: bmnas.graph.GraphedTrainStep(accumulate=m): m static micro-batches, ONE combine launch, ONE optimizer step in
one replay — on the small configuration and the global batch tests/helpers/dp_child.py uses (cfg_small(), BCE, 8
samples), split two ways evenly (4 + 4) and unevenly (5 + 3).

Parity rule (as tests/test_dp_gpu.py applies it): the combined gradient equals the float64 oracle
gradients computed micro-batch by micro-batch with shared weights (per-micro-batch BatchNorm statistics) and summed with
weights n_i / N — `assert_close_scaled(rel=5e-4)`, that test's tolerance."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

import accum_ref
from gpu_util import assert_close_scaled, dev, set_mode
from oracle import fusion_oracle as fo
from oracle import synth

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))
import dp_child as ch  # noqa: E402

pytestmark = pytest.mark.gpu
REL = 5e-4                     # tests/test_dp_gpu.py's


def _setup(drpt=0.0, mode='train_nodrop', lr=0.0):
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase, search_setup
    cfg = fo.Cfg({**fo.CONFIGS['mmimdb'], 'C': 32, 'drpt': drpt}) if drpt else ch.cfg_small()
    args = ch.make_args(cfg)
    args.use_dataparallel = False

    class Net(HyperNetBase):
        def __init__(self, criterion):
            super().__init__()
            self._build_head(args, criterion, nn.ModuleList([nn.Identity() for _ in range(cfg.N)]), cfg.N, 2)

        def forward(self, feats):
            return self.fuse(feats)

    crit = bnn.BCEWithLogitsLoss()
    model = Net(crit)
    model.fusion_net.load_state_dict(synth.make_params(cfg, ch.SEED))
    for dst, src in zip(model.arch_parameters(), synth.make_arch(cfg, ch.SEED, 0.5)):
        dst.data.copy_(src)
    cw, cb = synth.make_classifier(cfg, ch.NOUT, ch.SEED)
    model.central_classifier.weight.data.copy_(cw)
    model.central_classifier.bias.data.copy_(cb)
    optimizer, _, _, _ = search_setup(model, args, crit, dev(), 1.0, args.weight_decay)
    set_mode(model, mode)
    for g in optimizer.param_groups:
        g['lr'] = lr
    X = [x.to(dev()) for x in synth.make_inputs(cfg, ch.GLOBAL_BATCH, ch.SEED)]
    Y = synth.make_labels('bce', ch.GLOBAL_BATCH, ch.NOUT, ch.SEED).to(dev())
    return cfg, model, crit, optimizer, X, Y


def _micro(X, Y, cuts):
    return [([x[lo:hi].contiguous() for x in X], Y[lo:hi].contiguous()) for lo, hi in cuts]


def _names(model):
    return {id(p): n for grp in ('reshape_layers', 'fusion_net', 'central_classifier')
            for n, p in getattr(model, grp).named_parameters(prefix=grp)}


def _run_group(step, batches):
    for i, (xs, y) in enumerate(batches):
        step.stage(i, xs, y)
    return step.replay_staged()


@pytest.mark.parametrize('cuts', [((0, 4), (4, 8)), ((0, 5), (5, 8))], ids=['even', 'uneven'])
def test_combined_gradient_is_the_oracle_micro_batch_by_micro_batch(cuts):
    from bmnas.graph import GraphedTrainStep
    cfg, model, crit, optimizer, X, Y = _setup()
    batches = _micro(X, Y, cuts)
    step = GraphedTrainStep(model, crit, optimizer, [b[0] for b in batches], [b[1] for b in batches], accumulate=2)
    n = ch.GLOBAL_BATCH
    assert step.accum_weights == [(hi - lo) / n for lo, hi in cuts]
    assert step.matches_group(batches) and not step.matches_group(batches[:1])
    assert step.matches_group(batches[::-1]) == (cuts[0][1] - cuts[0][0] == cuts[1][1] - cuts[1][0])
    before = [p.detach().clone() for p in step.targets]
    launches = step.accumulator.launches
    out = _run_group(step, batches)
    torch.cuda.synchronize()
    assert len(out) == 2 and out[0][1].shape[0] == cuts[0][1] - cuts[0][0] and out[1][1].shape[0] == cuts[1][1] - cuts[1][0]
    assert step.accumulator.launches == launches                      # the combine is IN the graph: no Python launch
    for p, b in zip(step.targets, before):
        assert torch.equal(p.detach(), b)                             # lr = 0: the update is disarmed
    # (a) the float64 oracle, micro-batch by micro-batch, summed with n_i / N
    Xc, Yc = [x.cpu() for x in X], Y.cpu()
    cw, cb = synth.make_classifier(cfg, ch.NOUT, ch.SEED)
    want = None
    for lo, hi in cuts:
        _, _, g = fo.search_step([x[lo:hi] for x in Xc], Yc[lo:hi], synth.make_arch(cfg, ch.SEED, 0.5),
                                 synth.make_params(cfg, ch.SEED), cw, cb, cfg, 'bce', training=True, attn_drop=0.0)
        w = (hi - lo) / n
        g = {k: v for k, v in g.items() if not k.startswith('input.')}
        want = {k: w * v for k, v in g.items()} if want is None else {k: want[k] + w * v for k, v in g.items()}
    names = _names(model)
    checked = 0
    for p in step.targets:
        name = names[id(p)]
        key = name[len('fusion_net.'):] if name.startswith('fusion_net.') else name
        assert p.grad is step.accumulator.accumulation_tensor(p)
        if key.endswith('conv.bias') or key.endswith('out_conv.bias'):
            assert float(p.grad.abs().max()) < 1e-4                   # zero in exact arithmetic (bias in front of BN)
        else:
            assert_close_scaled(name, p.grad, want[key], rel=REL)
        checked += 1
    assert checked > 20
    # (b) bit-equal to the reference combine of the graph's OWN static parts
    parts = step.accum_plan['parts']
    assert [w for _, w in parts] == step.accum_weights
    for j, p in enumerate(step.targets):
        col = [None if gs[j] is None else gs[j].cpu().numpy() for gs, _ in parts]
        ref = accum_ref.combine(col, step.accum_weights)
        assert np.array_equal(p.grad.cpu().numpy().view(np.int32).reshape(-1), ref.view(np.int32).reshape(-1)), names[id(p)]


def test_two_replays_match_the_eager_accumulated_sequence():
    from bmnas import optim
    from bmnas.graph import GraphedTrainStep
    cuts = ((0, 5), (5, 8))
    _, model, crit, optimizer, X, Y = _setup(lr=1e-3)
    batches = _micro(X, Y, cuts)
    step = GraphedTrainStep(model, crit, optimizer, [b[0] for b in batches], [b[1] for b in batches], accumulate=2)
    for _ in range(2):
        _run_group(step, batches)
    torch.cuda.synchronize()
    got = [p.detach().clone() for p in step.targets]
    del step
    # the same two steps eagerly: autograd.grad per micro-batch, GradAccumulator, one optimizer step
    _, model2, crit2, optimizer2, _, _ = _setup(lr=1e-3)
    acc = optim.GradAccumulator(optimizer2)
    initial = [p.detach().clone() for p in acc.tensors]
    ws = optim.accum_weights([hi - lo for lo, hi in cuts], 'mean')
    for _ in range(2):
        for (xs, y), w in zip(batches, ws):
            acc.add(torch.autograd.grad(crit2(model2(xs), y), acc.tensors, allow_unused=True), w)
        acc.combine()
        optimizer2.step()
    torch.cuda.synchronize()
    assert acc.launches == 2
    names = _names(model2)
    moved = 0
    for a, b, p0 in zip(got, acc.tensors, initial):
        assert_close_scaled(names[id(b)], a, b.detach(), rel=REL)
        moved += int(not torch.equal(b.detach(), p0))
    assert moved > 20                                                 # real steps: the parameters moved


def test_micro_batches_of_one_replay_draw_different_dropout_masks():
    from bmnas.graph import GraphedTrainStep
    out = {}
    for label, drpt, mode in (('nodrop', 0.0, 'train_nodrop'), ('drop', 0.1, 'train')):
        _, model, crit, optimizer, X, Y = _setup(drpt=drpt, mode=mode)
        xs, y = _micro(X, Y, ((0, 4),))[0]
        step = GraphedTrainStep(model, crit, optimizer, xs, y, accumulate=2)      # one batch stands for two of its shape
        assert step.accum_weights == [0.5, 0.5]
        (l0, z0), (l1, z1) = _run_group(step, [(xs, y), (xs, y)])                # the SAME samples in both passes
        torch.cuda.synchronize()
        out[label] = float((z0 - z1).abs().max()), float(z0.abs().max())
        del step
    # without dropout the two passes agree to rounding (atomics); with it every pass has masks of its own
    assert out['nodrop'][0] <= 1e-4 * out['nodrop'][1], out
    assert out['drop'][0] > 1e-2 * out['drop'][1], out


def test_accumulate_one_builds_no_accumulator_and_refusals():
    from bmnas import lib
    from bmnas.graph import GraphedTrainStep
    _, model, crit, optimizer, X, Y = _setup()
    xs, y = _micro(X, Y, ((0, 4),))[0]
    # (f) refused before anything is run
    with pytest.raises(RuntimeError, match='k > 1'):
        GraphedTrainStep(model, crit, optimizer, xs, y, k=2, accumulate=2)
    with pytest.raises(RuntimeError, match='metric_forward'):
        GraphedTrainStep(model, crit, optimizer, xs, y, metric_forward=True, accumulate=2)
    with pytest.raises(RuntimeError, match='accum_max'):
        GraphedTrainStep(model, crit, optimizer, xs, y, accumulate=lib.accum_max() + 1)
    with pytest.raises(RuntimeError, match='micro-batches'):
        GraphedTrainStep(model, crit, optimizer, [xs], [y], accumulate=2)

    class _Reducer:
        world, selftest = 2, False
    optimizer._bmnas_reducer = _Reducer()
    try:
        with pytest.raises(RuntimeError, match='data parallelism'):
            GraphedTrainStep(model, crit, optimizer, xs, y, accumulate=2)
    finally:
        del optimizer._bmnas_reducer
    with pytest.raises(ValueError):
        GraphedTrainStep(model, crit, optimizer, xs, y, accumulate=0)
    # (e) accumulate=1: today's step
    step = GraphedTrainStep(model, crit, optimizer, xs, y, accumulate=1)
    assert step.accumulator is None and step.accum_plan is None and step.accumulate == 1
    loss, logits = step(xs, y)
    torch.cuda.synchronize()
    assert logits.shape[0] == 4 and bool(torch.isfinite(loss))
    with pytest.raises(RuntimeError, match='stage'):
        two = GraphedTrainStep(model, crit, optimizer, xs, y, accumulate=2)
        two(xs, y)
