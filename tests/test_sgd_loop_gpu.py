"""-m gpu: the DARTS recipe through the drivers — models.search._common.search_setup with args.optimizer = 'sgd',
args.momentum = 0.9 and args.grad_clip = 5 on the small MM-IMDB hypernet of tests/helpers/dp_child.py (fusion cell +
classifier, C = 32, batch 8) — captured by bmnas.graph.GraphedTrainStep: a graph is built (no fall-back to eager), and three
replayed weight steps match three eager steps of the same optimizer and three of torch.optim.SGD behind
torch.nn.utils.clip_grad_norm_.

At this configuration the gradient norm is about 1.2, below the recipe's max_grad_norm of 5: the norm launch and the
clipped instantiation run and report the norm, the coefficient is 1 (a clip that bites: tests/test_sgd_gpu.py).

Parameters are compared at the gradient tolerance of tests/gpu_util.py (2e-4 of |want| + scale, as
tests/test_grad_clip_network_gpu.py does): the sides' gradients agree to that (fp32 atomics accumulate them in a
run-dependent order) and the update is bounded by lr * (1 + momentum + momentum^2) * |g| per step.  lr is 1e-2, ten times the
drivers' eta_max, so that three steps move the parameters well past that tolerance; the test ends by showing that a
plain-SGD run of the same steps is >= 10 x the tolerance away."""
import os
import sys

import pytest
import torch
import torch.nn as nn

from gpu_util import assert_close_scaled, dev, set_mode

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))

GRAD_REL = 2e-4
STEPS = 3


def _build(**extra):
    """dp_child.run_grads' hypernet through search_setup, single process -> model, criterion, optimizer, args"""
    import dp_child as base
    from oracle import synth
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase, search_setup
    cfg = base.cfg_small()
    args = base.make_args(cfg)
    args.use_dataparallel = False
    for k, v in extra.items():
        setattr(args, k, v)

    class Net(HyperNetBase):
        def __init__(self, criterion):
            super().__init__()
            self._build_head(args, criterion, nn.ModuleList([nn.Identity() for _ in range(cfg.N)]), cfg.N, 2)

        def forward(self, feats):
            return self.fuse(feats)

    crit = bnn.BCEWithLogitsLoss()
    model = Net(crit)
    model.fusion_net.load_state_dict(synth.make_params(cfg, base.SEED))
    for dst, src in zip(model.arch_parameters(), synth.make_arch(cfg, base.SEED, 0.5)):
        dst.data.copy_(src)
    cw, cb = synth.make_classifier(cfg, base.NOUT, base.SEED)
    model.central_classifier.weight.data.copy_(cw)
    model.central_classifier.bias.data.copy_(cb)
    optimizer, _, _, _ = search_setup(model, args, crit, dev(), 1.0, args.weight_decay)
    set_mode(model, 'train_nodrop')
    return model, crit, optimizer, args


def _batch():
    import dp_child as base
    from oracle import synth
    cfg = base.cfg_small()
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, base.GLOBAL_BATCH, base.SEED)]
    return xs, synth.make_labels('bce', base.GLOBAL_BATCH, base.NOUT, base.SEED).to(dev())


def _same_params(label, got, want):
    for (k, a), (_, b) in zip(got.named_parameters(), want.named_parameters()):
        assert_close_scaled(f'{label} {k}', a, b, rel=GRAD_REL)


def test_sgd_weight_step_is_captured_and_follows_its_eager_twins(monkeypatch):
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import SGD
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    # eta_max 1e-2: at the drivers' 1e-3 only 2 of the 28 parameter tensors move by more than the tolerance in three steps
    sgd = dict(optimizer='sgd', momentum=0.9, grad_clip=5, eta_max=1e-2)
    xs, y = _batch()
    model_g, crit_g, opt_g, args = _build(**sgd)
    model_e, crit_e, opt_e, _ = _build(**sgd)
    model_t, crit_t, _, _ = _build(**sgd)
    model_p, crit_p, opt_p, _ = _build(**dict(sgd, momentum=0.0))                  # plain SGD: what momentum must differ from
    assert type(opt_g) is SGD and opt_g.max_grad_norm == 5 and opt_g.param_groups[0]['momentum'] == 0.9
    opt_t = torch.optim.SGD(model_t.central_params(), lr=args.eta_max, momentum=0.9, weight_decay=args.weight_decay)
    params_t = [p for g in opt_t.param_groups for p in g['params']]
    start = [p.detach().clone() for p in model_g.parameters()]

    step = GraphedTrainStep.try_build(model_g, crit_g, opt_g, xs, y)
    assert isinstance(step, GraphedTrainStep) and step.in_graph_step              # a graph, not the eager fall-back
    assert step.plan is opt_g._plan and step.plan['captured'] and step.plan['poke']
    assert step.plan['key'] == (True, True, False) and len(opt_g.state_dict()['state']) == 0

    for r in range(STEPS):
        for opt in (opt_g, opt_e, opt_t, opt_p):                                   # a moving rate, as the scheduler's
            for g in opt.param_groups:
                g['lr'] = args.eta_max * (0.7 ** r)
        step(xs, y)
        norm_g = float(opt_g.last_grad_norm)
        opt_e.zero_grad()
        crit_e(model_e(xs), y).backward()
        opt_e.step()
        norm_e = float(opt_e.last_grad_norm)
        opt_t.zero_grad()
        crit_t(model_t(xs), y).backward()
        norm_t = float(torch.nn.utils.clip_grad_norm_(params_t, 5))
        opt_t.step()
        opt_p.zero_grad()
        crit_p(model_p(xs), y).backward()
        opt_p.step()
        print(f'step {r}: norm replayed {norm_g!r} eager {norm_e!r} torch {norm_t!r} (max_grad_norm 5)')
        assert abs(norm_g - norm_e) <= GRAD_REL * norm_e and abs(norm_g - norm_t) <= GRAD_REL * norm_t
        _same_params(f'replay {r} against the eager step', model_g, model_e)
        _same_params(f'replay {r} against torch.optim.SGD', model_g, model_t)
    assert opt_g._plan is step.plan                                                # still the captured plan
    # the comparisons above cannot pass vacuously: the eager momentum twin must sit >= 10 x their tolerance from a plain-SGD
    # run of the same steps.  (Three steps of momentum 0.9 move a parameter (1 + 1.9 * 0.7 + 2.71 * 0.49) / 2.19 = 1.7 x as
    # far as plain SGD does; a float64 CPU evaluation of this step at a tenth of this lr puts two tensors 8.8 x the
    # tolerance apart, the other 26 within it: at this lr those two are expected near 90 x, and 10 x is asked of two.)
    apart = []
    for (k, a), (_, b) in zip(model_e.named_parameters(), model_p.named_parameters()):
        a, b = a.detach().double(), b.detach().double()
        tol = GRAD_REL * b.abs() + max(1e-6, GRAD_REL * float(b.abs().max()))     # assert_close_scaled's
        apart.append(float(((a - b).abs() / tol).max()))
    far = sum(x >= 10 for x in apart)
    print(f'momentum 0.9 against plain SGD: worst distance / tolerance {max(apart):.1f}; >= 10 on {far} of {len(apart)} tensors')
    assert far >= 2
    assert any(not torch.equal(a, b) for a, b in zip(start, model_g.parameters()))
    # the same tensors have stepped on both sides, and the state is torch's: momentum_buffer and nothing else
    sd_g, sd_t = opt_g.state_dict()['state'], opt_t.state_dict()['state']
    assert set(sd_g) == set(sd_t) and len(sd_g) > 0
    assert all(set(v) == {'momentum_buffer'} for v in sd_g.values())
