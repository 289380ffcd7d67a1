"""Host logic of the Adam variants (no GPU): bmnas.optim.Adam's amsgrad / decoupled_weight_decay arguments, bmnas.optim.AdamW,
torch's `param_groups` keys and nothing else in state_dict(), what load_state_dict() does to the switches, and the refusal
of groups that disagree on one."""
import copy

import pytest
import torch


def _params():
    return [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]


def test_the_two_switches_construct_and_live_in_torchs_keys():
    from bmnas.optim import Adam
    a = Adam(_params(), amsgrad=True)
    assert all(g['amsgrad'] is True and g['decoupled_weight_decay'] is False for g in a.param_groups)
    d = Adam(_params(), weight_decay=0.1, decoupled_weight_decay=True)
    assert all(g['amsgrad'] is False and g['decoupled_weight_decay'] is True for g in d.param_groups)
    plain = Adam(_params())
    assert all(g['amsgrad'] is False and g['decoupled_weight_decay'] is False for g in plain.param_groups)
    assert a._variant() == (False, True, False) and d._variant() == (False, False, True)
    assert Adam(_params(), amsgrad=True, max_grad_norm=5.0)._variant() == (True, True, False)
    # torch's keys and nothing new, in the live groups and in the checkpoint
    for ours, theirs in ((a, torch.optim.Adam(_params(), amsgrad=True)),
                         (d, torch.optim.Adam(_params(), weight_decay=0.1, decoupled_weight_decay=True))):
        assert set(ours.param_groups[0]) == set(theirs.param_groups[0])
        sd, sd_t = ours.state_dict(), theirs.state_dict()
        assert sd['param_groups'] == sd_t['param_groups']
        theirs.load_state_dict(copy.deepcopy(sd))                      # still a torch.optim.Adam checkpoint


def test_adamw_defaults_and_keys():
    from bmnas.optim import Adam, AdamW
    w = AdamW(_params())
    assert isinstance(w, Adam) and w.max_grad_norm is None
    assert all(g['weight_decay'] == 1e-2 and g['decoupled_weight_decay'] is True and g['amsgrad'] is False
               for g in w.param_groups)
    w = AdamW(_params(), lr=3e-3, weight_decay=0.2, amsgrad=True, max_grad_norm=2.0)
    assert w.max_grad_norm == 2.0 and w._variant() == (True, True, True)
    theirs = torch.optim.AdamW(_params(), lr=3e-3, weight_decay=0.2, amsgrad=True)
    assert w.state_dict()['param_groups'] == theirs.state_dict()['param_groups']
    assert 'max_grad_norm' not in w.param_groups[0]


def test_a_torch_adamw_checkpoint_flips_the_flag_of_adam():
    from bmnas.optim import Adam
    opt = Adam(_params(), lr=1e-3)
    assert opt._variant() == (False, False, False)
    opt.load_state_dict(torch.optim.AdamW(_params(), lr=1e-3, weight_decay=0.05).state_dict())
    assert all(g['decoupled_weight_decay'] is True and g['weight_decay'] == 0.05 for g in opt.param_groups)
    assert opt._variant() == (False, False, True)
    opt.load_state_dict(torch.optim.Adam(_params(), amsgrad=True).state_dict())
    assert opt._variant() == (False, True, False)


def test_adamw_stays_decoupled_whatever_it_loads():
    from bmnas.optim import AdamW
    opt = AdamW(_params(), lr=1e-3)
    opt.load_state_dict(torch.optim.Adam(_params(), lr=1e-3, weight_decay=0.05).state_dict())
    assert all(g['decoupled_weight_decay'] is True and g['weight_decay'] == 0.05 for g in opt.param_groups)
    assert opt._variant() == (False, False, True)


@pytest.mark.parametrize('name', ['amsgrad', 'decoupled_weight_decay'])
def test_groups_that_disagree_on_a_switch_are_refused_at_step(name):
    """CPU parameters: the check precedes the device check (whose message is about the GPU)."""
    from bmnas import lib
    from bmnas.optim import Adam
    ps = _params()
    opt = Adam([{'params': ps[:1]}, {'params': ps[1:], 'lr': 3e-3}], lr=1e-3, weight_decay=0.1)
    for p in ps:
        p.grad = torch.ones_like(p)
    opt.param_groups[1][name] = True
    with pytest.raises(lib.BmnasError, match=name):
        opt.step()
    with pytest.raises(lib.BmnasError, match=name):
        opt.capture_safe()
    assert not opt.state                                               # refused before any state was created
    opt.param_groups[0][name] = True                                   # agreeing again
    assert opt._variant() == (False, name == 'amsgrad', name != 'amsgrad')
