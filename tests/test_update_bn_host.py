"""CPU: bmnas.optim.update_bn on a pure-torch model against torch.optim.swa_utils.update_bn, what it restores (also when
a forward raises), the `unpack` callable, the momentum -> (value, mode) helper of bmnas.lib and the parsing of
args.swa_update_bn.  No GPU: nothing here launches."""
import copy
import math
import types

import pytest
import torch
import torch.nn as nn
from torch.optim import swa_utils

from bmnas import lib
from bmnas.optim import update_bn


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.c1, self.b1 = nn.Conv1d(3, 5, 1), nn.BatchNorm1d(5, momentum=0.01)
        self.c2, self.b2 = nn.Conv1d(5, 4, 1), nn.BatchNorm1d(4)
        self.fail = False

    def forward(self, x):
        if self.fail:
            raise RuntimeError('forward failed')
        return self.b2(self.c2(torch.relu(self.b1(self.c1(x)))))


def _net():
    torch.manual_seed(3)
    net = Net().double()
    with torch.no_grad():
        for bn in (net.b1, net.b2):                      # buffers that a reset must clear
            bn.running_mean.normal_()
            bn.running_var.uniform_(0.5, 2.0)
            bn.num_batches_tracked.fill_(9)
    return net


def _batches():
    g = torch.Generator().manual_seed(4)
    return [torch.randn(b, 3, 4, generator=g, dtype=torch.float64) for b in (4, 4, 3)]      # the last one ragged


def _buffers(net):
    return {k: v.clone() for k, v in net.state_dict().items() if 'running' in k or 'num_batches' in k}


def test_leaves_the_buffers_torch_leaves():
    ours, theirs = _net(), _net()
    ours.eval()
    report = update_bn([(x, None) for x in _batches()], ours)            # torch's convention: batch[0]
    swa_utils.update_bn([(x, None) for x in _batches()], theirs)
    for k, v in _buffers(theirs).items():
        assert torch.equal(_buffers(ours)[k], v), k
    assert int(ours.b1.num_batches_tracked) == 3
    assert report == dict(batches=3, replays=0, eager=3)
    assert ours.b1.momentum == 0.01 and ours.b2.momentum == 0.1 and not ours.training and not ours.b1.training


def test_restores_training_mode_and_momenta_when_the_forward_raises():
    net = _net()
    net.train()
    net.fail = True
    with pytest.raises(RuntimeError, match='forward failed'):
        update_bn(_batches(), net)
    assert net.b1.momentum == 0.01 and net.b2.momentum == 0.1 and net.training and net.b2.training


def test_unpack_is_honoured():
    seen = []

    def unpack(batch, device):
        seen.append(device)
        return batch['modalities'][0], batch['label']

    ours, theirs = _net(), _net()
    data = [{'modalities': [x], 'label': torch.zeros(x.shape[0])} for x in _batches()]
    update_bn(data, ours, 'cpu', unpack=unpack)
    swa_utils.update_bn(_batches(), theirs)
    assert seen == ['cpu'] * 3
    for k, v in _buffers(theirs).items():
        assert torch.equal(_buffers(ours)[k], v), k


def test_a_model_without_batchnorm_is_left_alone():
    net = nn.Linear(3, 2)
    assert update_bn([torch.zeros(1, 3)], net) == dict(batches=0, replays=0, eager=0)


def test_momentum_to_value_and_mode():
    assert (lib.BN_MOM_DEFAULT, lib.BN_MOM_VALUE, lib.BN_MOM_CUMULATIVE) == (0, 1, 2)
    assert lib.bn_momentum(0.1) == (0.0, 0) == lib.bn_momentum(nn.BatchNorm1d(2).momentum)
    assert lib.bn_momentum(0.01) == (0.01, 1) and lib.bn_momentum(0.0) == (0.0, 1) and lib.bn_momentum(1) == (1.0, 1)
    assert lib.bn_momentum(None) == (0.0, 2)
    with pytest.raises(lib.BmnasError):
        lib.bn_momentum(math.nan)
    # the descriptor of the default path is byte for byte what it was: the two new fields are zero
    old = lib.BnFin(1, 2, 3, 4, 5, 6, 7, 4, 1, 1, 1)
    new = lib.make_bn_fin(None, 0, None, None, None, None, None, None, False)
    assert (old.momentum, old.momentum_mode) == (0.0, 0) == (new.momentum, new.momentum_mode)
    assert (lib.NO_FIN.momentum, lib.NO_FIN.momentum_mode) == (0.0, 0)
    fin = lib.make_bn_fin(None, 0, None, None, None, None, None, None, True, momentum=None)
    assert (fin.momentum, fin.momentum_mode) == (0.0, 2)


def test_swa_update_bn_option():
    from models.search._common import averaging_options, make_averager, update_bn_option
    ns = types.SimpleNamespace
    assert update_bn_option(ns(), 'eval') is False and update_bn_option(ns(swa_start=0), 'search') is False
    assert update_bn_option(ns(swa_update_bn=False, ema_decay=0.9), 'eval', world=4) is False
    assert update_bn_option(ns(swa_update_bn=True, swa_start=0), 'eval', world=1) is True
    assert update_bn_option(ns(swa_update_bn=True, ema_decay=0.9), 'eval') is True
    with pytest.raises(ValueError, match='search'):
        update_bn_option(ns(swa_update_bn=True, swa_start=0), 'search')
    with pytest.raises(ValueError, match='shard'):
        update_bn_option(ns(swa_update_bn=True, swa_start=0), 'eval', world=2)
    with pytest.raises(ValueError, match='ema_decay or args.swa_start'):
        update_bn_option(ns(swa_update_bn=True), 'eval')
    # without the option the averager is what it was; with it the buffers are not averaged
    assert averaging_options(ns(swa_start=2), 'eval') == dict(decay=None, swa_start=2, skip_frozen=True)
    avg, opts = make_averager(Net(), ns(swa_start=2), 'eval')
    assert avg.use_buffers and opts['update_bn'] is False
    avg, opts = make_averager(Net(), ns(swa_start=2, swa_update_bn=True), 'eval')
    assert not avg.use_buffers and opts['update_bn'] is True
    net = copy.deepcopy(avg.module)
    assert isinstance(net, Net)
