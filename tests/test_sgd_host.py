"""Host logic of bmnas.optim.SGD (no GPU): constructor and torch's `param_groups` keys, nothing of ours in state_dict(),
torch's own refusals, the refusal of `maximize` and of groups that disagree on a kernel switch, and the optimizers
models.search._common.search_setup builds from the optional args.optimizer / momentum / dampening / nesterov arguments."""
import copy

import pytest
import torch
import torch.nn as nn


def _params():
    return [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]


def test_constructor_keeps_torchs_keys_and_refusals():
    from bmnas import lib
    from bmnas.optim import SGD, _OneLaunch
    opt = SGD(_params(), lr=0.1, momentum=0.9, dampening=0.5, weight_decay=3e-4, max_grad_norm=5)
    theirs = torch.optim.SGD(_params(), lr=0.1, momentum=0.9, dampening=0.5, weight_decay=3e-4)
    assert isinstance(opt, torch.optim.SGD) and isinstance(opt, _OneLaunch)
    assert opt.state_dict() == theirs.state_dict()                     # torch's keys and nothing new; no state yet
    theirs.load_state_dict(copy.deepcopy(opt.state_dict()))            # still a torch.optim.SGD checkpoint
    assert opt.max_grad_norm == 5 and opt.last_grad_norm is None and opt.grad_norms is None
    assert opt._variant() == (True, True, False)
    assert SGD(_params())._variant() == (False, False, False) and SGD(_params()).param_groups[0]['lr'] == 1e-3
    assert SGD(_params(), momentum=0.9, nesterov=True)._variant() == (False, True, True)
    for bad in (dict(nesterov=True), dict(nesterov=True, momentum=0.9, dampening=0.1), dict(lr=-1.0),
                dict(momentum=-0.5), dict(weight_decay=-1.0)):
        with pytest.raises(ValueError):                                # torch's own refusals stay
            SGD(_params(), **bad)
    for bad in (0, -1.0, float('nan'), '5', True):
        with pytest.raises(lib.BmnasError, match='bmnas.optim.SGD: max_grad_norm'):
            SGD(_params(), max_grad_norm=bad)


def test_maximize_is_refused_wherever_it_comes_from():
    from bmnas import lib
    from bmnas.optim import SGD
    with pytest.raises(lib.BmnasError, match='maximize'):
        SGD(_params(), maximize=True)
    opt = SGD(_params(), lr=0.1, momentum=0.9)
    before = copy.deepcopy(opt.state_dict())
    with pytest.raises(lib.BmnasError, match='maximize'):
        opt.load_state_dict(torch.optim.SGD(_params(), lr=0.5, maximize=True).state_dict())
    assert opt.state_dict() == before                                  # refused before anything was loaded
    opt.param_groups[0]['maximize'] = True
    for p in opt.param_groups[0]['params']:
        p.grad = torch.ones_like(p)
    with pytest.raises(lib.BmnasError, match='maximize'):
        opt.step()


@pytest.mark.parametrize('edit,name', [(dict(momentum=0.0), 'momentum'), (dict(nesterov=True, dampening=0), 'nesterov')])
def test_groups_that_disagree_on_a_switch_are_refused_at_step(edit, name):
    """CPU parameters: the check precedes the device check (whose message is about the GPU)."""
    from bmnas import lib
    from bmnas.optim import SGD
    ps = _params()
    opt = SGD([{'params': ps[:1]}, {'params': ps[1:], 'lr': 3e-3, 'momentum': 0.5}], lr=1e-3, momentum=0.9)
    for p in ps:
        p.grad = torch.ones_like(p)
    assert opt._variant() == (False, True, False)                      # different non-zero momenta: one kernel
    opt.param_groups[1].update(edit)
    with pytest.raises(lib.BmnasError, match=f"param_groups disagree on '{name}'"):
        opt.step()
    with pytest.raises(lib.BmnasError, match=f"param_groups disagree on '{name}'"):
        opt.capture_safe()
    assert not opt.state and not opt._pending                          # refused before any buffer was created
    opt.param_groups[0].update(edit)                                   # agreeing again
    assert opt._variant() == (False, name == 'nesterov', name == 'nesterov')
    with pytest.raises(lib.BmnasError, match='needs parameters on the GPU'):
        opt.capture_safe()                                             # no CPU path


def test_loading_a_state_forgets_pending_buffers_and_plans():
    from bmnas.optim import SGD
    ps = _params()
    opt = SGD(ps, lr=0.1, momentum=0.9)
    opt._pending[ps[0]] = torch.zeros(3)
    theirs = torch.optim.SGD(_params(), lr=0.2, momentum=0.8, dampening=0.1)
    for p in theirs.param_groups[0]['params']:
        p.grad = torch.ones_like(p)
    theirs.step()
    opt.load_state_dict(copy.deepcopy(theirs.state_dict()))
    assert not opt._pending and opt._plan is None and opt._gen == 1
    assert opt.param_groups[0]['momentum'] == 0.8 and opt.param_groups[0]['dampening'] == 0.1
    assert all(opt._stepped(p) for p in ps)                            # restored buffers count as stepped ones
    assert torch.equal(opt._buffer(ps[0]), torch.ones(3))


# --------------------------------------------------------------------------------------------------------------- drivers
class _A:
    C, L, drpt = 16, 8, 0.1
    num_input_nodes, num_keep_edges, steps, multiplier = 3, 2, 1, 1
    node_steps, node_multiplier, num_outputs = 1, 1, 5
    eta_max, eta_min, Ti, Tm = 1e-3, 1e-6, 1, 2
    arch_learning_rate, arch_weight_decay, weight_decay = 3e-4, 1e-3, 1e-4
    use_dataparallel = False


def _setup(monkeypatch, **extra):
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase, search_setup
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    args = _A()
    for k, v in extra.items():
        setattr(args, k, v)

    class Net(HyperNetBase):
        def __init__(self, criterion):
            super().__init__()
            self._build_head(args, criterion, nn.ModuleList([nn.Identity() for _ in range(3)]), 3, 2)

    crit = bnn.BCEWithLogitsLoss()
    optimizer, scheduler, architect, _ = search_setup(Net(crit), args, crit, torch.device('cpu'), 4, args.weight_decay)
    return optimizer, architect.optimizer, scheduler


def test_search_setup_without_the_new_arguments_builds_the_adam_it_always_built(monkeypatch):
    from bmnas.optim import Adam, AdamW
    w, a, _ = _setup(monkeypatch)
    assert type(w) is Adam and type(a) is Adam
    assert len(w.param_groups) == 3 and len(a.param_groups) == 1
    for g in w.param_groups:
        assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (1e-3, (0.9, 0.999), 1e-8, 1e-4)
        assert g['amsgrad'] is False and g['decoupled_weight_decay'] is False
    g = a.param_groups[0]
    assert (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (3e-4, (0.5, 0.999), 1e-8, 1e-3)
    assert g['amsgrad'] is False and g['decoupled_weight_decay'] is False
    assert w.max_grad_norm is None and a.max_grad_norm is None
    # the earlier optional arguments still reach it, and 'adam' by name is the same thing
    w, a, _ = _setup(monkeypatch, optimizer='adam', arch_optimizer='adam', grad_clip=5.0, arch_amsgrad=True,
                     decoupled_weight_decay=True, momentum=0.5)
    assert type(w) is Adam and w.max_grad_norm == 5.0 and w._variant() == (True, False, True)
    assert type(a) is Adam and a._variant() == (False, True, False) and not isinstance(w, AdamW)


def test_search_setup_builds_the_sgd_its_arguments_describe(monkeypatch):
    from bmnas.optim import SGD, Adam
    w, a, sched = _setup(monkeypatch, optimizer='sgd', grad_clip=5)
    assert type(w) is SGD and type(a) is Adam                          # each optimizer has its own switch
    assert len(w.param_groups) == 3 and w.max_grad_norm == 5
    for g in w.param_groups:
        assert (g['lr'], g['momentum'], g['dampening'], g['weight_decay'], g['nesterov']) == (1e-3, 0.9, 0, 1e-4, False)
    assert sched is not None
    w, a, _ = _setup(monkeypatch, optimizer='sgd', momentum=0.8, dampening=0.25, arch_optimizer='sgd', arch_momentum=0.5,
                     arch_nesterov=True, arch_grad_clip=0.5)
    g = w.param_groups[0]
    assert (g['momentum'], g['dampening'], g['nesterov']) == (0.8, 0.25, False) and w.max_grad_norm is None
    g = a.param_groups[0]
    assert type(a) is SGD and a.max_grad_norm == 0.5
    assert (g['lr'], g['momentum'], g['dampening'], g['weight_decay'], g['nesterov']) == (3e-4, 0.5, 0, 1e-3, True)
    assert _setup(monkeypatch, arch_optimizer='sgd')[1].param_groups[0]['momentum'] == 0.9
    with pytest.raises(ValueError, match="'adam' or 'sgd'"):
        _setup(monkeypatch, optimizer='rmsprop')
