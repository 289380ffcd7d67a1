"""Host logic of gradient-norm clipping (no GPU): bmnas.optim.Adam's max_grad_norm argument and what
bmnas.optim.clip_grad_norm_ hands to torch's function."""
import pytest
import torch


def _params():
    return [torch.nn.Parameter(torch.ones(3)), torch.nn.Parameter(torch.ones(2, 2))]


def test_max_grad_norm_is_validated_and_stays_out_of_param_groups():
    from bmnas import lib
    from bmnas.optim import Adam
    for bad in (0, -1.0, float('nan'), '5', True):
        with pytest.raises(lib.BmnasError):
            Adam(_params(), max_grad_norm=bad)
    opt = Adam(_params(), lr=1e-3, max_grad_norm=5)
    assert opt.max_grad_norm == 5 and opt.last_grad_norm is None and opt.grad_norms is None
    assert Adam(_params()).max_grad_norm is None
    sd = opt.state_dict()
    assert all('max_grad_norm' not in g for g in sd['param_groups'])
    torch.optim.Adam(_params(), lr=1e-3).load_state_dict(sd)            # still a torch.optim.Adam checkpoint
    opt.load_state_dict(torch.optim.Adam(_params(), lr=1e-2).state_dict())
    assert opt.max_grad_norm == 5


def test_stand_alone_clip_hands_cpu_tensors_and_other_norms_to_torch():
    from bmnas.optim import clip_grad_norm_
    for kwargs in ({}, {'norm_type': 1.0}, {'norm_type': float('inf')}, {'error_if_nonfinite': True}):
        a, b = _params(), _params()
        for i, (p, q) in enumerate(zip(a, b)):
            p.grad = torch.full_like(p, 2.0 + i)
            q.grad = torch.full_like(q, 2.0 + i)
        got = clip_grad_norm_(a, 1.5, **kwargs)
        want = torch.nn.utils.clip_grad_norm_(b, 1.5, **kwargs)
        assert torch.equal(got, want)
        for p, q in zip(a, b):
            assert torch.equal(p.grad, q.grad)
    p = _params()[0]
    p.grad = torch.tensor([float('nan'), 1.0, 1.0])
    with pytest.raises(RuntimeError):
        clip_grad_norm_(p, 1.0, error_if_nonfinite=True)
    assert float(clip_grad_norm_(_params(), 1.0)) == 0.0               # no gradients at all: torch's answer
