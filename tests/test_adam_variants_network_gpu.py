"""-m gpu: bmnas.optim.AdamW(amsgrad=True, max_grad_norm=...) inside captured steps of whole networks — GraphedTrainStep
against an eager twin with the same optimizer, k steps per replay, the launches of the captured step, and the drivers'
arguments.  Small configurations of tests/test_grad_clip_network_gpu.py (SMALL_LAZY search cell, SMALL_PLAIN found
network, batch 17).

Parameters are compared at that file's gradient tolerance (2e-4 of |want| + scale): the two sides' gradients agree to that
(fp32 atomics accumulate them in a run-dependent order) and Adam's update is bounded by lr per step.  The running
maximum's invariant — max_exp_avg_sq = maximum(its value before the step, exp_avg_sq after it) — holds bit for bit.

eps = 1e-6 on both twins.  The conv biases in front of a train-mode BatchNorm have a gradient that is mathematically zero
and arrives as fp32 round-off, <= 1.3e-9 here (seven orders below the real gradients) and different on the two sides.
Adam normalises a gradient: with the default eps = 1e-8 such a bias moves by ~5 % of lr per step, in a run-dependent
direction, and the twins drift apart by 1.3e-4 in three steps (3 x the tolerance) whatever the optimizer does.  An L2 decay
hides this (wd * p ~ 5e-6 swamps the round-off: test_grad_clip_network_gpu.py); a decoupled decay never enters the
gradient.  eps is Adam's own remedy: at 1e-6 a round-off gradient moves its parameter by <= lr * 1.3e-9 / 1e-6 per step,
8e-6 over three steps on two sides, a fifth of the smallest tolerance in these networks (2e-4 x 0.2), while the
parameters with a real gradient (|g| 1e-5 ... 1e-2) keep Adam's normalised update.  Every parameter stays compared."""
import sys

import pytest
import torch

from fc_edges_util import device_kernels
from oracle import fusion_oracle as fo
from test_crit_network_gpu import SMALL_LAZY, SMALL_PLAIN, _batch, _model
from test_grad_clip_network_gpu import BATCH, GRAD_REL, HELPERS, NOUT, _crit, _first_norm, _same_params

pytestmark = pytest.mark.gpu

EPS = 1e-6                 # see the module docstring


def _bits(t):
    return t.detach().view(torch.int32)


def _maxes(opt):
    return {p: st['max_exp_avg_sq'].clone() for p, st in opt.state.items() if 'max_exp_avg_sq' in st}


def _assert_running_max(opt, before, label):
    assert before
    for p, was in before.items():
        st = opt.state[p]
        assert torch.equal(_bits(st['max_exp_avg_sq']), _bits(torch.maximum(was, st['exp_avg_sq']))), label


def _eager(model, opt, crit, xs, y):
    opt.zero_grad()
    crit(model(xs), y).backward()
    opt.step()


@pytest.mark.parametrize('shape,found', [(SMALL_LAZY, False), (SMALL_PLAIN, True)], ids=['search', 'found'])
def test_captured_adamw_amsgrad_step_follows_the_eager_twin(shape, found):
    from bmnas import cell as K
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import AdamW
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg = fo.make_cfg(**shape)
    xs, y = _batch(cfg, BATCH, NOUT, 'bce', None)
    c = _first_norm(shape, found, xs, y) / 2                        # half the first step's norm: it clips
    crit = _crit()
    models = [_model(cfg, NOUT, found) for _ in range(2)]
    opt_g, opt_e = [AdamW(list(m.parameters()), lr=1e-3, eps=EPS, amsgrad=True, max_grad_norm=c) for m in models]
    step = GraphedTrainStep(models[0], crit, opt_g, xs, y)
    assert step.plan['flags'] == 3 and step.plan['clip']
    start = [p.detach().clone() for p in models[0].parameters()]
    for r in range(3):
        before = _maxes(opt_g)
        step(xs, y)
        torch.cuda.synchronize()
        _assert_running_max(opt_g, before, f'replay {r}')
        _eager(models[1], opt_e, crit, xs, y)
        got, want = float(opt_g.last_grad_norm), float(opt_e.last_grad_norm)
        print(f'replay {r}: norm {got!r} twin {want!r} max_grad_norm {c!r}')
        assert abs(got - want) <= GRAD_REL * want
        _same_params(f'replay {r}', models[0], models[1])
    assert any(not torch.equal(a, b) for a, b in zip(start, models[0].parameters()))
    assert any(float(st['max_exp_avg_sq'].max()) > 0 for st in opt_g.state.values())


def test_two_steps_per_replay_equal_two_single_replays():
    """GraphedTrainStep(k=2): each slot's descriptor table carries its own max_exp_avg_sq pointer array behind it."""
    from bmnas import cell as K
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import AdamW
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg = fo.make_cfg(**SMALL_LAZY)
    batches = [_batch(cfg, BATCH, NOUT, 'bce', None, seed=s) for s in (31, 32)]
    c = _first_norm(SMALL_LAZY, False, *batches[0]) / 2
    crit = _crit()
    models = [_model(cfg, NOUT) for _ in range(2)]
    opts = [AdamW(list(m.parameters()), lr=1e-3, eps=EPS, amsgrad=True, max_grad_norm=c) for m in models]
    g2 = GraphedTrainStep(models[0], crit, opts[0], *batches[0], k=2)
    g1 = GraphedTrainStep(models[1], crit, opts[1], *batches[0])
    assert g2.plan['slots'] == 2 and len(g2.plan['dev_maxes']) == 2
    for j, (xs, y) in enumerate(batches):
        g2.stage(j, xs, y)
    g2.replay_staged()
    for xs, y in batches:
        g1(xs, y)
    torch.cuda.synchronize()
    _same_params('k=2', models[0], models[1])
    for st in opts[0].state.values():                                  # both slots wrote the one running maximum
        assert bool((st['max_exp_avg_sq'] >= st['exp_avg_sq']).all())
    assert any(float(st['max_exp_avg_sq'].max()) > 0 for st in opts[0].state.values())
    assert float(opts[0].state_dict()['state'][0]['step']) == 2.0


@pytest.mark.parametrize('shape,found', [(SMALL_LAZY, False), (SMALL_PLAIN, True)], ids=['search', 'found'])
def test_variant_captured_step_adds_no_device_event(shape, found):
    """AMSGrad + decoupled decay ride in the one update launch; clipping adds its norm launch; nothing of aten."""
    from bmnas import cell as K
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam, AdamW
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg = fo.make_cfg(**shape)
    xs, y = _batch(cfg, BATCH, NOUT, 'bce', None)
    names = {}
    for label, make in (('plain', lambda ps: Adam(ps, lr=1e-3)),
                        ('variant', lambda ps: AdamW(ps, lr=1e-3, amsgrad=True)),
                        ('clipped', lambda ps: AdamW(ps, lr=1e-3, amsgrad=True, max_grad_norm=1.0))):
        model = _model(cfg, NOUT, found)
        step = GraphedTrainStep(model, _crit(), make(list(model.parameters())), xs, y)
        step(xs, y)
        torch.cuda.synchronize()
        names[label] = device_kernels(lambda: step(xs, y))
        assert torch.isfinite(step(xs, y)[0]).all()
        del step
    plain, variant, clipped = names['plain'], names['variant'], names['clipped']
    print(f'{len(plain)} device events plain, {len(variant)} AdamW + amsgrad, {len(clipped)} with clipping')
    assert len(variant) == len(plain), (plain, variant)
    assert len(clipped) == len(plain) + 1, (plain, clipped)
    for got in (variant, clipped):
        assert sum('adam_multi_ex_k' in n for n in got) == 1
        assert not [n for n in got if 'at::native' in n]
        assert not [n for n in got if 'adam_multi_k' in n or 'adam_multi_clip_k' in n]
    assert sum('grad_sqnorm_multi_k' in n for n in clipped) == 1 and not [n for n in variant if 'grad_sqnorm' in n]
    assert not [n for n in plain if 'adam_multi_ex_k' in n] and sum('adam_multi_k' in n for n in plain) == 1


def test_search_setup_reads_the_four_switch_arguments(monkeypatch):
    """tests/helpers/clip_dp_child.build with the arguments added to what its make_args returns (build itself passes only
    grad_clip / arch_grad_clip through)."""
    sys.path.insert(0, HELPERS)
    import clip_dp_child as ch
    from bmnas.optim import Adam

    def build(**extra):
        make = ch.base.make_args

        def with_extra(cfg):
            args = make(cfg)
            for k, v in extra.items():
                setattr(args, k, v)
            return args
        monkeypatch.setattr(ch.base, 'make_args', with_extra)
        try:
            return ch.build()
        finally:
            monkeypatch.setattr(ch.base, 'make_args', make)

    _, _, optimizer, architect, _ = build()
    for opt in (optimizer, architect.optimizer):
        assert type(opt) is Adam and opt._variant() == (False, False, False)
    _, _, optimizer, architect, args = build(amsgrad=True, arch_decoupled_weight_decay=True)
    assert optimizer._variant() == (False, True, False) and architect.optimizer._variant() == (False, False, True)
    assert all(g['weight_decay'] == args.arch_weight_decay for g in architect.optimizer.param_groups)
    _, _, optimizer, architect, _ = build(decoupled_weight_decay=True, arch_amsgrad=True, grad_clip=5.0)
    assert optimizer._variant() == (True, False, True) and architect.optimizer._variant() == (False, True, False)
    assert set(optimizer.state_dict()['param_groups'][0]) == set(
        torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))]).state_dict()['param_groups'][0])
