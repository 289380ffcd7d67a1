"""tests/sgd_ref.py (the float64 restatement the SGD GPU tests are read against) pinned to torch.optim.SGD on the CPU in
float64 over the layout of tests/test_sgd_gpu.py: the first-step rule, nesterov, dampening, L2 decay, a preceding
torch.nn.utils.clip_grad_norm_, two groups with different momentum and dampening, and a tensor joining at step 2 (its
first-step rule then runs while the others are past theirs).  Also: the configurations are far enough apart to be told
from each other at the GPU tests' tolerance, and torch's own fp32 run sits well inside it."""
import numpy as np
import pytest
import torch

import sgd_ref

TOL = 2e-6                     # the GPU tests' tolerance (of each tensor's scale)


def _same(a, b, tol=1e-12):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape
    assert np.abs(a - b).max() <= tol * max(1.0, np.abs(b).max())


@pytest.mark.parametrize('name', list(sgd_ref.CASES))
def test_six_steps_equal_torchs(name):
    cfg = sgd_ref.CASES[name]
    cpu, opt = sgd_ref.torch_cached(name)
    P, B, norms = sgd_ref.ref_run(cfg)
    for i, p in enumerate(cpu):
        _same(P[i], p.detach().numpy())
        buf = opt.state.get(p, {}).get('momentum_buffer')
        assert (buf is None) == (B[i] is None)
        if buf is not None:
            _same(B[i], buf.numpy())
    assert all((n is None) == (cfg.get('max_norm') is None) for n in norms)
    if cfg.get('max_norm') is not None:
        assert sum(n > cfg['max_norm'] for n in norms) >= 3          # the clip does bite
    if name == 'plain':
        assert all(b is None for b in B) and len(opt.state_dict()['state']) == 0


@pytest.mark.parametrize('name', list(sgd_ref.NEIGHBOUR))
def test_the_cases_can_be_told_apart_at_the_gpu_tolerance(name):
    apart = sgd_ref.distance(sgd_ref.torch_cached(name)[0], sgd_ref.torch_cached(sgd_ref.NEIGHBOUR[name])[0])
    print(f'{name} against {sgd_ref.NEIGHBOUR[name]}: {apart:.3e} of scale')
    assert apart >= 100 * TOL


def test_a_late_tensor_takes_the_first_step_rule_on_its_own():
    """dampening 0.5: parameter 2's buffer after ITS first step (step 2 of the run) is its gradient, undamped."""
    cfg = sgd_ref.CASES['dampening']
    P, B, _ = sgd_ref.ref_run(cfg, steps=3)
    assert np.array_equal(B[2], sgd_ref.grads_of(2)[2].double().numpy())
    assert not np.array_equal(B[1], sgd_ref.grads_of(2)[1].double().numpy())
    cpu, opt = sgd_ref.torch_run(cfg, steps=3)
    _same(B[2], opt.state[cpu[2]]['momentum_buffer'].numpy())


@pytest.mark.parametrize('name', list(sgd_ref.CASES))
def test_fp32_sequence_is_within_the_gpu_tolerance_of_float64(name):
    """Every operation rounded to fp32 on its own (what the kernel computes) against float64: the tolerance of the GPU
    tests has a wide margin."""
    cfg = sgd_ref.CASES[name]
    P64, B64, _ = sgd_ref.ref_run(cfg)
    P32, B32, _ = sgd_ref.ref_run(cfg, dtype=np.float32)
    worst = 0.0
    for a, b in list(zip(P32, P64)) + [(x, y) for x, y in zip(B32, B64) if y is not None]:
        assert a.dtype == np.float32
        worst = max(worst, float(np.abs(a.astype(np.float64) - b).max()) / (float(np.abs(b).max()) + 1e-3))
    print(f'{name}: fp32 op-by-op against float64 {worst:.3e} of scale')
    assert worst <= TOL / 4


def test_absent_terms_leave_the_bits():
    """dampening == 0 and weight_decay == 0 in fp32, operation by operation: the bits of the sequence without those terms
    (1 * g is g; the decay is skipped, not added as zero)."""
    cfg = sgd_ref.CASES['momentum']
    a = sgd_ref.ref_run(cfg, dtype=np.float32)
    b = sgd_ref.ref_run(cfg, dtype=np.float32, plain_terms=True)
    for x, y in zip(a[0] + a[1], b[0] + b[1]):
        assert np.array_equal(x.view(np.int32), y.view(np.int32))


def test_nan_gradient_with_clipping_reaches_every_parameter():
    ps = [torch.ones(3, dtype=torch.float64, requires_grad=True), torch.ones(2, dtype=torch.float64, requires_grad=True)]
    opt = torch.optim.SGD(ps, lr=0.1, momentum=0.9)
    grads = [torch.tensor([1.0, float('nan'), 1.0], dtype=torch.float64), torch.ones(2, dtype=torch.float64)]
    for p, g in zip(ps, grads):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(ps, 5.0)
    opt.step()
    P, B, n = sgd_ref.clipped_sgd_step([np.ones(3), np.ones(2)], grads, [None, None], 0.1, 5.0, 0.9)
    assert np.isnan(n) and all(np.isnan(p).all() for p in P) and all(torch.isnan(p).all() for p in ps)
