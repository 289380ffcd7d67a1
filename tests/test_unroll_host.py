"""Host logic of the unrolled architecture step (no GPU): an Architect without `args.unrolled` is the first-order one and
never builds a bmnas.optim.UnrolledStep nor touches the network optimizer; what the unrolled step refuses, it refuses
before anything moves; the scalar row of a weight tensor follows DARTS' try / except over `momentum_buffer`; and
models.search._common.search_setup hands the weight optimizer to the Architect."""
import copy

import pytest
import torch
import torch.nn as nn


class _Net(nn.Module):
    """A CPU stand-in with the two things the Architect asks of a model: a forward and arch_parameters()."""

    def __init__(self):
        super().__init__()
        torch.manual_seed(0)
        self.lin = nn.Linear(4, 3)
        self.alpha = [torch.zeros(3, requires_grad=True)]
        self.calls = 0

    def forward(self, x):
        self.calls += 1
        return self.lin(x) * torch.softmax(self.alpha[0], 0)

    def arch_parameters(self):
        return self.alpha


class _Args:
    weight_decay = 1e-4
    hip_graph = False


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(5, 4, generator=g), torch.randn(5, 3, generator=g)


def _architect(network_optimizer='sgd', **extra):
    from models.search.darts.architect import Architect
    args = _Args()
    for k, v in extra.items():
        setattr(args, k, v)
    net = _Net()
    if network_optimizer == 'sgd':
        network_optimizer = torch.optim.SGD(net.parameters(), lr=0.1, momentum=0.9, weight_decay=3e-4)
    arch_opt = torch.optim.Adam(net.arch_parameters(), lr=0.01)
    return Architect(net, args, nn.MSELoss(), arch_opt, network_optimizer=network_optimizer), net


class _Untouchable:
    """a network optimizer whose every attribute access is a failure"""

    def __getattr__(self, name):
        raise AssertionError(f'the first-order step read network_optimizer.{name}')


@pytest.mark.parametrize('extra', [{}, {'unrolled': False}, {'unrolled': 0}], ids=['absent', 'False', 'zero'])
def test_without_unrolled_the_architect_is_first_order_and_builds_no_unrolled_step(monkeypatch, extra):
    import bmnas.optim

    def boom(*a, **k):
        raise AssertionError('UnrolledStep was built')

    monkeypatch.setattr(bmnas.optim, 'UnrolledStep', boom)
    arch, net = _architect(network_optimizer=_Untouchable(), **extra)
    assert arch.unrolled is False and arch.unrolled_r == 1e-2
    x, y = _batch(1)
    w0 = [p.detach().clone() for p in net.parameters()]
    a0 = net.alpha[0].detach().clone()
    # a training batch handed to a first-order Architect is ignored
    assert arch.step(x, y, None, input_train=x, target_train=y) is None
    assert arch.step(x, y, None) is None
    assert arch._unrolled is None and arch.unrolled_steps == 0 and net.calls == 2
    assert not torch.equal(net.alpha[0], a0)
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), w0))
    # ... and it is exactly the reference's zero_grad / backward / step
    twin = _Net()
    opt = torch.optim.Adam(twin.arch_parameters(), lr=0.01)
    for _ in range(2):
        opt.zero_grad()
        nn.MSELoss()(twin(x), y).backward()
        opt.step()
    assert torch.equal(twin.alpha[0], net.alpha[0])


def test_args_reach_the_architect():
    arch, _ = _architect(unrolled=True, unrolled_r=5e-3)
    assert arch.unrolled is True and arch.unrolled_r == 5e-3 and arch._unrolled is None
    arch, _ = _architect(unrolled=1)
    assert arch.unrolled is True and arch.unrolled_r == 1e-2


def _frozen(arch, net):
    return ([p.detach().clone() for p in net.parameters()], net.alpha[0].detach().clone(),
            None if arch.network_optimizer is None else copy.deepcopy(arch.network_optimizer.state_dict()),
            copy.deepcopy(arch.optimizer.state_dict()))


def _assert_nothing_moved(arch, net, frozen):
    w0, a0, sd_w, sd_a = frozen
    assert net.calls == 0                                                 # not even a forward
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), w0)) and torch.equal(net.alpha[0], a0)
    assert all(p.grad is None for p in net.parameters()) and net.alpha[0].grad is None
    if sd_w is not None:
        assert arch.network_optimizer.state_dict() == sd_w
    assert arch.optimizer.state_dict() == sd_a and arch.unrolled_steps == 0


def test_the_unrolled_step_refuses_before_anything_moves(monkeypatch):
    from bmnas import lib
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    x, y = _batch(1)
    xt, yt = _batch(2)
    # no training batch
    arch, net = _architect(unrolled=True)
    fr = _frozen(arch, net)
    for kw in ({}, {'input_train': xt}, {'target_train': yt}):
        with pytest.raises(lib.BmnasError, match='training batch'):
            arch.step(x, y, None, **kw)
    _assert_nothing_moved(arch, net, fr)
    # no network optimizer
    arch, net = _architect(network_optimizer=None, unrolled=True)
    fr = _frozen(arch, net)
    with pytest.raises(lib.BmnasError, match='network optimizer'):
        arch.step(x, y, None, input_train=xt, target_train=yt)
    _assert_nothing_moved(arch, net, fr)
    # groups with different learning rates: DARTS' step has one eta
    arch, net = _architect(network_optimizer=None, unrolled=True)
    arch.network_optimizer = torch.optim.SGD([{'params': [net.lin.weight]}, {'params': [net.lin.bias], 'lr': 0.05}],
                                             lr=0.1, momentum=0.9)
    fr = _frozen(arch, net)
    with pytest.raises(lib.BmnasError, match='different learning rates'):
        arch.step(x, y, None, input_train=xt, target_train=yt)
    _assert_nothing_moved(arch, net, fr)
    # more than one process
    arch, net = _architect(unrolled=True)
    fr = _frozen(arch, net)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(lib.BmnasError, match='world size 2'):
        arch.step(x, y, None, input_train=xt, target_train=yt)
    _assert_nothing_moved(arch, net, fr)
    monkeypatch.delenv('WORLD_SIZE')
    # ... and with everything in place the CPU model is refused by the step itself (HIP kernels, no CPU path) — after
    # the training forward, with the weights untouched
    arch, net = _architect(unrolled=True)
    w0 = [p.detach().clone() for p in net.parameters()]
    with pytest.raises(lib.BmnasError, match='contiguous fp32 on the parameter device|on the GPU'):
        arch.step(x, y, None, input_train=xt, target_train=yt)
    assert all(torch.equal(p, q) for p, q in zip(net.parameters(), w0))


def test_rows_follow_the_momentum_buffers():
    """mu = the group's momentum where state[p] holds a momentum_buffer, else 0 (DARTS' try / except); wd = the group's
    weight_decay."""
    from bmnas import lib
    from bmnas.optim import SGD, Adam, UnrolledStep
    ps = [nn.Parameter(torch.ones(3)), nn.Parameter(torch.ones(2, 2))]
    alpha = [torch.zeros(2, requires_grad=True)]
    with pytest.raises(lib.BmnasError, match='network'):
        UnrolledStep(None, alpha)
    # torch.optim.SGD: stepped tensors have buffers, the others not
    opt = torch.optim.SGD([{'params': ps[:1]}, {'params': ps[1:], 'momentum': 0.5, 'weight_decay': 0.1}], lr=0.1,
                          momentum=0.9, weight_decay=3e-4)
    us = UnrolledStep(opt, alpha, r=2e-2)
    assert us.r == 2e-2 and us.weights == ps and us.arch == alpha and us.eta() == 0.1
    g0, g1 = opt.param_groups
    assert us.row_of(ps[0], g0) == (False, 0.0, 3e-4) and us.row_of(ps[1], g1) == (False, 0.0, 0.1)
    ps[0].grad = torch.ones(3)
    opt.step()                                                           # ps[1] has no gradient: no buffer
    assert us.row_of(ps[0], g0) == (True, 0.9, 3e-4) and us.row_of(ps[1], g1) == (False, 0.0, 0.1)
    ps[1].grad = torch.ones(2, 2)
    opt.step()
    assert us.row_of(ps[1], g1) == (True, 0.5, 0.1)
    # bmnas.optim.SGD that has not stepped: a zero buffer waiting in _pending is no momentum_buffer
    ours = SGD(ps, lr=0.1, momentum=0.9, weight_decay=1e-4)
    ours._pending[ps[0]] = torch.zeros(3)
    us = UnrolledStep(ours, alpha)
    assert us.row_of(ps[0], ours.param_groups[0]) == (False, 0.0, 1e-4)
    # Adam, the BM-NAS default: the plain step, stepped or not
    for adam in (Adam(ps, lr=1e-3, weight_decay=1e-4), torch.optim.Adam(ps, lr=1e-3, weight_decay=1e-4)):
        us = UnrolledStep(adam, alpha)
        assert us.row_of(ps[0], adam.param_groups[0]) == (False, 0.0, 1e-4)
    adam.step()
    assert 'exp_avg' in adam.state[ps[0]] and us.row_of(ps[0], adam.param_groups[0]) == (False, 0.0, 1e-4)
    # the optimizer's state was only read
    assert set(adam.state[ps[0]]) == {'step', 'exp_avg', 'exp_avg_sq'}
    # lists that do not follow the weight tensors are refused
    with pytest.raises(lib.BmnasError, match='1 gradients for 2 weight tensors'):
        us.virtual_step([None])
    with pytest.raises(lib.BmnasError, match='no weight tensor has a gradient'):
        us.virtual_step([None, None])
    with pytest.raises(lib.BmnasError, match='virtual_step'):
        us.perturb([None, None], 1)
    with pytest.raises(lib.BmnasError, match='virtual_step'):
        us.restore()


class _A:
    C, L, drpt = 16, 8, 0.1
    num_input_nodes, num_keep_edges, steps, multiplier = 3, 2, 1, 1
    node_steps, node_multiplier, num_outputs = 1, 1, 5
    eta_max, eta_min, Ti, Tm = 1e-3, 1e-6, 1, 2
    arch_learning_rate, arch_weight_decay, weight_decay = 3e-4, 1e-3, 1e-4
    use_dataparallel = False


@pytest.mark.parametrize('extra', [{}, {'unrolled': True, 'unrolled_r': 5e-3, 'optimizer': 'sgd'}], ids=['default', 'unrolled'])
def test_search_setup_hands_the_weight_optimizer_to_the_architect(monkeypatch, extra):
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
    optimizer, _, architect, _ = search_setup(Net(crit), args, crit, torch.device('cpu'), 4, args.weight_decay)
    assert architect.network_optimizer is optimizer and architect._unrolled is None
    assert architect.unrolled is bool(extra) and architect.unrolled_r == (5e-3 if extra else 1e-2)
