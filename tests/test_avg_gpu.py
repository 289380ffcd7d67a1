"""-m gpu: bmnas.optim.AveragedModel over the small hypernet of tests/test_sgd_loop_gpu.py (tests/avg_util.py).

  * ten updates with an optimizer step between them, EMA and SWA: the averaged tensors equal tests/avg_ref.py bit for
    bit after every update (integer buffers: copied), and stay within the derived bound 5 * n * 2^-24 * M of torch's
    own class run on the same device over the same snapshots (M: the largest magnitude the tensor took);
  * an update — the first one and a later one — issues no host synchronisation (torch's sync detector in 'error' mode);
  * skip_frozen gives the bits of the full update when the frozen tensors do not move, with fewer tensors in the launch;
  * copy.deepcopy of the hypernet computes the original's forward, eagerly and through bmnas.graph.GraphedForward.  The
    forward holds fp32 atomics (the classifier's split-K sum), so two passes of ONE model agree to round-off, not to the
    bit: the comparison is the one tests/test_graph_forward_gpu.py makes between a replay and an eager pass (1e-5)."""
import copy

import numpy as np
import pytest
import torch
from torch.optim import swa_utils

import avg_ref
import avg_util as au
from gpu_util import assert_close_scaled

pytestmark = pytest.mark.gpu

UPDATES = 10


@pytest.mark.parametrize('decay', [0.9, None], ids=['ema', 'swa'])
def test_ten_updates_are_avg_ref_bit_for_bit_and_torch_within_the_bound(decay):
    from bmnas.optim import AveragedModel
    model, crit, opt, _ = au.build(eta_max=1e-2)
    xs, y = au.batch()
    ours = AveragedModel(model, decay=decay, use_buffers=True)
    fn = swa_utils.get_ema_multi_avg_fn(decay) if decay is not None else None
    # (torch's SWA refuses integer buffers — its addcdiv raises on int64 —: there torch's class averages the parameters
    # only, and only they are compared with it)
    theirs = swa_utils.AveragedModel(model, multi_avg_fn=fn, use_buffers=decay is not None)
    n_params = len(list(model.parameters()))
    want = au.tensors(ours.module)
    assert any(t.dtype == np.int64 for t in want) and sum(t.dtype == np.float32 for t in want) > 10
    biggest = [0.0] * len(want)
    for n in range(UPDATES):
        opt.zero_grad()
        crit(model(xs), y).backward()
        opt.step()
        live = au.tensors(model)
        ours.update_parameters(model)
        theirs.update_parameters(model)
        want = avg_ref.update(want, live, n, decay)
        got = au.tensors(ours.module)
        assert au.same_bits(got, want) == [], (n, au.same_bits(got, want))
        biggest = [max(m, float(np.abs(t).max())) if t.dtype == np.float32 and t.size else m
                   for m, t in zip(biggest, live)]
    assert ours.launches == UPDATES and int(ours.n_averaged) == UPDATES == int(theirs.n_averaged)
    worst = 0.0
    for i, (a, b, m, p) in enumerate(zip(au.tensors(ours.module), au.tensors(theirs.module), biggest,
                                         au.tensors(model))):
        if decay is None and i >= n_params and a.dtype == np.float32:
            continue
        if a.dtype != np.float32:
            assert np.array_equal(a, p)                  # an integer buffer: the live value (torch: a truncated average)
            continue
        err = float(np.abs(a.astype(np.float64) - b.astype(np.float64)).max()) if a.size else 0.0
        worst = max(worst, err / max(avg_ref.bound(UPDATES, m), 1e-300))
        assert err <= avg_ref.bound(UPDATES, m), (err, avg_ref.bound(UPDATES, m))
    print(f'decay {decay}: worst |ours - torch| / bound = {worst:.3f}')
    # ... and the average is no copy of the live weights
    assert any(not np.array_equal(a, p) for a, p in zip(au.tensors(ours.module), au.tensors(model))
               if a.dtype == np.float32)


def test_update_does_not_synchronise():
    from bmnas.optim import AveragedModel
    model, _, _, _ = au.build()
    avg = AveragedModel(model, decay=0.99, use_buffers=True, skip_frozen=True)
    next(iter(model.parameters())).requires_grad_(False)          # (a frozen tensor: the first update's second launch)
    torch.cuda.synchronize()
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for _ in range(3):
            avg.update_parameters(model)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    assert int(avg.n_averaged) == 3 and avg._n == 3 and avg.launches == 4


def test_skip_frozen_equals_the_full_update_when_frozen_tensors_rest():
    from bmnas.optim import AveragedModel
    model, _, _, _ = au.build()
    params = list(model.parameters())
    frozen = params[::3]
    for p in frozen:
        p.requires_grad_(False)
    full = AveragedModel(model, decay=0.75, use_buffers=True)
    skip = AveragedModel(model, decay=0.75, use_buffers=True, skip_frozen=True)
    with torch.no_grad():                                # the first update must COPY the frozen tensors: spoil the copies
        for a, p in zip(skip.module.parameters(), params):
            if not p.requires_grad:
                a.fill_(123.0)
    g = torch.Generator(device='cuda').manual_seed(3)
    for n in range(5):
        with torch.no_grad():
            for p in params:
                if p.requires_grad:
                    p.add_(0.01 * torch.randn(p.shape, generator=g, device=p.device))
        full.update_parameters(model)
        skip.update_parameters(model)
        assert au.same_bits(au.tensors(skip.module), au.tensors(full.module)) == [], n
    for a, p in zip(skip.module.parameters(), params):
        if not p.requires_grad:
            assert torch.equal(a, p)
    n_all = len(full._eager[(id(model), 'all')]['order'])
    assert len(skip._eager[(id(model), 'all')]['order']) == n_all - len(frozen)
    assert len(skip._eager[(id(model), 'frozen')]['order']) == len(frozen)
    assert skip.launches == 6 and full.launches == 5     # one extra launch, once


def test_deepcopy_computes_the_originals_forward_eagerly_and_replayed():
    from bmnas.graph import GraphedForward
    model, crit, _, _ = au.build()
    xs, y = au.batch()
    twin = copy.deepcopy(model)
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(twin.parameters(), model.parameters()))
    for net in (model, twin):
        net.eval()
    with torch.no_grad():
        want, got = model(xs), twin(xs)
    assert_close_scaled('eager forward of the copy', got, want, rel=1e-5)
    fwd_m = GraphedForward.try_build(model, crit, xs, y)
    fwd_t = GraphedForward.try_build(twin, twin.criterion, xs, y)
    assert isinstance(fwd_m, GraphedForward) and isinstance(fwd_t, GraphedForward)
    loss_m, out_m = fwd_m(xs, y)
    loss_t, out_t = fwd_t(xs, y)
    assert_close_scaled('replayed forward of the copy', out_t, out_m, rel=1e-5)
    assert_close_scaled('replayed forward against eager', out_t, want, rel=1e-5)
    assert_close_scaled('replayed loss of the copy', loss_t.reshape(1), loss_m.reshape(1), rel=1e-5)
    # the copy is a model of its own: moving the original does not move it
    with torch.no_grad():
        model.central_classifier.bias.add_(1.0)
    _, out_t2 = fwd_t(xs, y)
    assert_close_scaled('the copy after the original moved', out_t2, want, rel=1e-5)
