"""-m gpu: bmnas.optim.GradAccumulator, eager: the optimizer downstream sees an ordinary `.grad`.  After three
accumulated steps the parameters are bit-equal to those of the same optimizer stepping on tests/accum_ref.py's combine of
the same parts (uploaded as plain gradients) — Adam, and SGD with momentum and max_grad_norm (the norm is that of the
combined gradient).  Plus the refusals of add() and of an unprepared captured combine()."""
import numpy as np
import pytest
import torch

import accum_ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

SHAPES = [(5,), (33, 31), (1024,), (3, 7, 11)]          # ragged float4, one chunk and a bit, a whole chunk, small
WEIGHTS = [1.0 / 3.0, 0.5, 1.0 / 7.0]


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter((torch.randn(s, generator=g) * 0.5).to(dev())) for s in SHAPES]


def _make(kind, ps):
    from bmnas import optim
    if kind == 'adam':
        return optim.Adam([{'params': ps[:2]}, {'params': ps[2:], 'lr': 3e-3}], lr=1e-2, weight_decay=1e-3)
    return optim.SGD(ps, lr=5e-2, momentum=0.9, weight_decay=1e-3, max_grad_norm=0.7)


def _step_parts(step):
    """Three parts per tensor; tensor 3 gets nothing at all in step 1, tensor 1 misses its middle part in step 2."""
    g = torch.Generator().manual_seed(1000 + step)
    parts = [[torch.randn(s, generator=g) * (1.0 + i) for s in SHAPES] for i in range(3)]
    if step == 1:
        for row in parts:
            row[3] = None
    if step == 2:
        parts[1][1] = None
    return parts


@pytest.mark.parametrize('kind', ['adam', 'sgd'])
def test_accumulated_steps_equal_steps_on_the_reference_combine(kind):
    from bmnas import optim
    got_p, want_p = _params(5), _params(5)
    opt, ref = _make(kind, got_p), _make(kind, want_p)
    acc = optim.GradAccumulator(opt)
    assert acc.tensors == got_p
    for step in range(3):
        parts = _step_parts(step)
        for row, w in zip(parts, WEIGHTS):
            acc.add([None if t is None else t.to(dev()) for t in row], w)
        assert acc.pending == 3
        acc.combine()
        assert acc.pending == 0
        for j, p in enumerate(want_p):
            col = [row[j] for row in parts]
            if all(t is None for t in col):
                p.grad = None
                assert got_p[j].grad is None                       # no part covered it
                continue
            want = accum_ref.combine([None if t is None else t.numpy() for t in col], WEIGHTS)
            p.grad = torch.from_numpy(want).to(dev())
            assert got_p[j].grad is acc.accumulation_tensor(got_p[j])
            assert torch.equal(got_p[j].grad.view(torch.int32), p.grad.view(torch.int32)), (step, j)
        opt.step()
        ref.step()
        if kind == 'sgd':
            assert torch.equal(opt.last_grad_norm, ref.last_grad_norm)
    torch.cuda.synchronize()
    for a, b in zip(got_p, want_p):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    assert acc.launches == 3
    # the same parts again: the tables the device holds are re-used only when the bytes are the same
    assert 1 <= acc.uploads <= 3


def test_upload_is_skipped_when_the_device_holds_the_bytes():
    from bmnas import optim
    ps = _params(2)
    acc = optim.GradAccumulator(optim.Adam(ps, lr=1e-3))
    parts = [[torch.randn_like(p) for p in ps] for _ in range(2)]
    for _ in range(3):
        for row in parts:
            acc.add(row, 0.5)
        acc.combine()
    torch.cuda.synchronize()
    assert acc.launches == 3 and acc.uploads == 1
    want = accum_ref.combine([parts[0][1].cpu().numpy(), parts[1][1].cpu().numpy()], [0.5, 0.5])
    assert np.array_equal(ps[1].grad.cpu().numpy().view(np.int32), want.view(np.int32))
    acc.add(parts[0], 1.0)
    acc.reset()
    assert acc.pending == 0


def test_add_refuses_a_ninth_part_a_wrong_dtype_and_an_aliasing_part():
    from bmnas import lib, optim
    ps = _params(3)
    acc = optim.GradAccumulator(optim.Adam(ps, lr=1e-3))
    row = [torch.zeros_like(p) for p in ps]
    with pytest.raises(lib.BmnasError, match='gradients for'):
        acc.add(row[:2], 1.0)
    with pytest.raises(lib.BmnasError, match='contiguous fp32'):
        acc.add([row[0].double()] + row[1:], 1.0)
    with pytest.raises(lib.BmnasError, match='contiguous fp32'):
        acc.add([row[0], torch.zeros(31, 33, device=dev()).t()] + row[2:], 1.0)
    with pytest.raises(lib.BmnasError, match='contiguous fp32'):
        acc.add([torch.zeros(6, device=dev())] + row[1:], 1.0)
    with pytest.raises(lib.BmnasError, match='contiguous fp32'):
        acc.add([row[0].cpu()] + row[1:], 1.0)
    assert acc.pending == 0
    acc.add(row, 1.0)
    acc.combine()
    with pytest.raises(lib.BmnasError, match='aliases'):
        acc.add([ps[0].grad] + row[1:], 1.0)                       # the accumulation tensor itself
    for _ in range(lib.accum_max()):
        acc.add(row, 0.125)
    with pytest.raises(lib.BmnasError, match='at most 8'):
        acc.add(row, 0.125)
    acc.reset()
    with pytest.raises(lib.BmnasError, match='no parts'):
        acc.combine()


def test_combine_inside_a_capture_needs_capture_safe():
    from bmnas import lib, optim
    ps = _params(4)
    acc = optim.GradAccumulator(optim.Adam(ps, lr=1e-3))
    row = [torch.ones_like(p) for p in ps]
    acc.add(row, 1.0)
    acc.combine()                                                  # eager plan and accumulation tensors exist
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    raised = None
    with torch.cuda.graph(graph):
        row[0].add_(0.0)                                           # (the capture is not empty)
        acc.add(row, 1.0)
        try:
            acc.combine()
        except lib.BmnasError as e:                                # raised BEFORE anything is issued: the capture ends clean
            raised = e
    assert raised is not None and 'capture_safe' in str(raised)
    acc.reset()
    # ... and with it: the launch alone is captured, the tables go up in captured_plan(), the replay combines
    acc.capture_safe(2)
    static = [[torch.full_like(p, 2.0) for p in ps], [torch.full_like(p, 4.0) for p in ps]]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        acc.add(static[0], 0.5)
        acc.add(static[1], 0.25)
        acc.combine()
    plan = acc.captured_plan()
    assert plan['weights'] == [0.5, 0.25] and acc.captures == 1
    for p in ps:
        p.grad.fill_(-1.0)
    graph.replay()
    torch.cuda.synchronize()
    for p in ps:
        assert bool((p.grad == 2.0).all())
    with pytest.raises(lib.BmnasError, match='no open capture'):
        acc.captured_plan()
