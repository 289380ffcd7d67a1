"""CPU: the host side of bmnas.optim.AveragedModel — the scalar rows it stages (first update, EMA, SWA, decay 0 and 1, the
|w| < 0.5 boundary), which tensors a skip_frozen launch holds, checkpoints travelling to and from torch's class, and the
refusal of the trainer options in a search.  No GPU: nothing here launches."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn
from torch.optim import swa_utils

import avg_ref
from bmnas import lib
from bmnas.optim import AveragedModel, avg_row, avg_weight, _AVG_ROW


def _rec(row):
    r = np.zeros(1, dtype=_AVG_ROW)
    r[0] = row
    return r[0]


def test_row_layout_is_the_headers():
    assert _AVG_ROW.itemsize == 32
    assert [_AVG_ROW.fields[n][1] for n in ('w', 'omw', 'flags', 'count')] == [0, 4, 8, 16]
    assert lib.AVG_RAW == 1


def test_first_update_is_the_row_w_1():
    for decay in (None, 0.0, 0.5, 0.999, 1.0):
        r = _rec(avg_row(0, decay))
        assert (r['w'], r['omw'], r['flags'], r['count']) == (1.0, 0.0, 0, 1)


@pytest.mark.parametrize('n', [1, 2, 3])
def test_swa_rows(n):
    r = _rec(avg_row(n))
    w = np.float32(1.0) / np.float32(n + 1)                      # torch: 1 / (num_averaged + 1) on a tensor
    assert r['w'] == w and r['count'] == n + 1 and r['flags'] == 0
    assert r['omw'] == np.float32(1.0 - float(w))                # formed in double, rounded once
    assert avg_weight(n) == avg_ref.weight(n) == float(w)


def test_ema_rows():
    r = _rec(avg_row(7, 0.999))
    assert r['w'] == np.float32(1.0 - 0.999) and r['omw'] == np.float32(1.0 - (1.0 - 0.999)) and r['count'] == 8
    r = _rec(avg_row(7, 0.0))                                    # decay 0: the live weights, every time
    assert (r['w'], r['omw']) == (1.0, 0.0)
    r = _rec(avg_row(7, 1.0))                                    # decay 1: the average never moves after the first copy
    assert (r['w'], r['omw']) == (0.0, 1.0)
    assert avg_weight(7, 0.9) == avg_ref.weight(7, 0.9)


def test_boundary_at_one_half_takes_the_second_branch():
    """|w| < 0.5 is false at exactly 0.5 (SWA's second update, EMA with decay 0.5): a = p - d * omw with omw = 0.5."""
    for row in (avg_row(1), avg_row(5, 0.5)):
        r = _rec(row)
        assert r['w'] == 0.5 and r['omw'] == 0.5 and not abs(r['w']) < 0.5
    below = float(np.nextafter(np.float32(0.5), np.float32(0)))
    r = _rec(avg_row(5, 1.0 - below))
    assert abs(r['w']) < 0.5


def test_raw_row_carries_the_count_only():
    r = _rec(avg_row(4, 0.9, raw=True))
    assert (r['w'], r['omw'], r['flags'], r['count']) == (0.0, 0.0, lib.AVG_RAW, 5)


class Net(nn.Module):
    def __init__(self):
        super().__init__()
        self.backbone = nn.Linear(3, 4)
        self.bn = nn.BatchNorm1d(4)
        self.head = nn.Linear(4, 2)
        for p in self.backbone.parameters():
            p.requires_grad_(False)


def _names(avg, trio):
    by_id = {id(t): k for k, t in list(avg.module.named_parameters()) + list(avg.module.named_buffers())}
    return [(by_id[id(a)], kind) for a, _, kind in trio]


def test_skip_frozen_membership():
    net = Net()
    avg = AveragedModel(net, decay=0.9, use_buffers=True, skip_frozen=True)
    every = [('backbone.weight', 'avg'), ('backbone.bias', 'avg'), ('bn.weight', 'avg'), ('bn.bias', 'avg'),
             ('head.weight', 'avg'), ('head.bias', 'avg'), ('bn.running_mean', 'avg'), ('bn.running_var', 'avg'),
             ('bn.num_batches_tracked', 'raw')]                  # an integer buffer is copied, whatever the recipe
    assert _names(avg, avg.members(net, with_frozen=True)) == every
    later = [e for e in every if not e[0].startswith('backbone')]
    assert _names(avg, avg._main(net)) == _names(avg, avg.members(net, with_frozen=False)) == later
    frozen = [k for (k, _), (_, _, _, f) in zip(every, avg.pairs(net)) if f]
    assert frozen == ['backbone.weight', 'backbone.bias']        # parameters with requires_grad=False; never a buffer
    plain = AveragedModel(net, decay=0.9, use_buffers=True)      # the default is torch's: everything, every time
    assert _names(plain, plain._main(net)) == every
    sync = AveragedModel(net, skip_frozen=True)                  # use_buffers=False: buffers are kept in sync by copy
    assert [k for _, k in _names(sync, sync._main(net))] == ['avg'] * 4 + ['raw'] * 3


def test_constructor_refuses_what_it_does_not_take():
    with pytest.raises(ValueError, match='decay'):
        AveragedModel(Net(), decay=1.5)
    with pytest.raises(TypeError):
        AveragedModel(Net(), avg_fn=lambda a, b, n: a)
    with pytest.raises(TypeError):
        AveragedModel(Net(), multi_avg_fn=lambda a, b, n: None)


def test_cpu_models_run_torchs_class_after_a_note():
    net = Net()
    ours = AveragedModel(net, decay=0.9, use_buffers=True)
    ref = swa_utils.AveragedModel(Net(), multi_avg_fn=swa_utils.get_ema_multi_avg_fn(0.9), use_buffers=True)
    ref.module.load_state_dict(net.state_dict())
    assert ours.off_path(net) == 'tensors off the GPU'
    for step in range(3):
        with torch.no_grad():
            for p in net.parameters():
                p.add_(0.1 * (step + 1))
        with pytest.warns(RuntimeWarning, match='AveragedModel') if step == 0 else _nullcontext():
            ours.update_parameters(net)
        ref.update_parameters(net)
    assert int(ours.n_averaged) == 3
    for (k, a), (_, b) in zip(ours.module.state_dict().items(), ref.module.state_dict().items()):
        assert torch.equal(a, b), k


class _nullcontext:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


def test_state_dict_round_trip_with_torchs_class():
    net = Net()
    ours = AveragedModel(net, decay=0.9, use_buffers=True, skip_frozen=True)
    theirs = swa_utils.AveragedModel(Net(), multi_avg_fn=swa_utils.get_ema_multi_avg_fn(0.9), use_buffers=True)
    assert list(ours.state_dict()) == list(theirs.state_dict())              # the same keys, in the same order
    with torch.no_grad():
        for p in theirs.module.parameters():
            p.fill_(0.25)
        theirs.n_averaged.fill_(11)
    ours.load_state_dict(theirs.state_dict())                                # torch's checkpoint into ours
    assert ours._n is None and ours._count() == 11 and ours._n == 11         # the mirror is re-read once
    assert all(bool((p == 0.25).all()) for p in ours.module.parameters())
    back = swa_utils.AveragedModel(Net(), use_buffers=True)
    back.load_state_dict(ours.state_dict())                                  # ... and ours into torch's
    assert int(back.n_averaged) == 11
    for (k, a), (_, b) in zip(back.state_dict().items(), theirs.state_dict().items()):
        assert torch.equal(a, b), k


def test_options_are_read_for_found_stage_runs_and_refused_in_a_search():
    from models.search._common import averaging_options, make_averager
    none = types.SimpleNamespace()
    assert averaging_options(none, 'eval') is None and averaging_options(none, 'search') is None
    assert make_averager(Net(), none, 'eval') == (None, None)
    ema = types.SimpleNamespace(ema_decay=0.99)
    assert averaging_options(ema, 'eval') == dict(decay=0.99, swa_start=None, skip_frozen=True)
    swa = types.SimpleNamespace(swa_start=2, average_skip_frozen=False)
    assert averaging_options(swa, 'eval') == dict(decay=None, swa_start=2, skip_frozen=False)
    for args in (ema, swa):
        with pytest.raises(ValueError, match='would not belong to the current alphas'):
            averaging_options(args, 'search')
    with pytest.raises(ValueError, match='set one of them'):
        averaging_options(types.SimpleNamespace(ema_decay=0.9, swa_start=1), 'eval')
    with pytest.raises(ValueError, match='ema_decay'):
        averaging_options(types.SimpleNamespace(ema_decay=1.2), 'eval')
    avg, opts = make_averager(Net(), ema, 'eval')
    assert isinstance(avg, AveragedModel) and avg.use_buffers and avg.skip_frozen and avg.decay == 0.99
    assert isinstance(avg, swa_utils.AveragedModel) and opts['decay'] == 0.99


def test_rider_rows_leave_the_staging_layout_alone():
    """The rows of a captured averager ride behind the optimizer's: extra_bytes = 0 is today's layout, and a rider only
    moves what lies behind the scalar region."""
    from bmnas.optim import staging_layout
    base = staging_layout(2, 5, slots=2, clip=True)
    assert staging_layout(2, 5, slots=2, clip=True, extra_bytes=0) == base
    assert base.extra_at == 2 * base.hyp_slot == 160
    ride = staging_layout(2, 5, slots=2, clip=True, extra_bytes=96)
    assert (ride.rows_at, ride.clip_at, ride.hyp_slot, ride.extra_at) == (base.rows_at, base.clip_at, base.hyp_slot, 160)
    assert ride.hyp_bytes == 256 and ride.tab_at[0] == 256 and ride.nbytes == base.nbytes + 64
    with pytest.raises(ValueError):
        staging_layout(2, 5, extra_bytes=24)
