"""-m gpu: global gradient-norm clipping inside the one-launch Adam step (csrc/adam.hip: grad_sqnorm_multi_k,
adam_multi_clip_k, grad_scale_multi_k; bmnas.optim.Adam(max_grad_norm=...), bmnas.optim.clip_grad_norm_) against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam on the CPU and against float64 (tests/clip_ref.py).

Tolerances.  Norm: |norm - ref| <= 2e-5 * ref — an fp32 sum of non-negative terms is off by at most depth * 2^-24
relative, the depth here is <= ~300 additions (a lane's run over its chunks, the wave and block trees, <= 256 partials),
and the square root halves it.  Parameters and moments: tests/test_optim_gpu.py's 2e-6 of scale — Adam's m / sqrt(v) does
not see a common factor on the gradients, so the norm's rounding does not widen it.

The CPU side runs torch's own functions in float64: torch's fp32 norm on the CPU is itself off by up to 1.5e-6 relative
at these sizes (measured against float64, where the kernel's norm is within 1e-9) — the reference's error, not the
kernel's, and it would enter exp_avg_sq twice and the stand-alone form's gradients once."""
import numpy as np
import pytest
import torch

import clip_ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

SHAPES = [(384, 384, 1), (384,), (7,), (1,), (13, 2), (3, 5, 11), (4099,), (192, 16)]     # test_optim_gpu.py's
NORM_SIZES = [1, 3, 1023, 1024, 1025, 4099, 300001]
NORM_TOL = 2e-5


def _make(seed, shapes):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(*s, generator=g) for s in shapes]


def _table(grads):
    """bmnas_adam_tensor_t[] + (tensor, chunk) list over the gradients that exist, as bmnas.optim.Adam builds them."""
    from bmnas import lib
    from bmnas.optim import _DESC
    grads = [g for g in grads if g is not None]
    E = lib.adam_chunk_elems()
    tab = np.zeros(len(grads), dtype=_DESC)
    tab['grad'] = [g.data_ptr() for g in grads]
    tab['numel'] = [g.numel() for g in grads]
    chunks = [(i, c) for i, g in enumerate(grads) for c in range((g.numel() + E - 1) // E)]
    return (torch.from_numpy(tab.view(np.uint8)).to(dev()),
            torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev()), len(chunks))


def _sqnorm(grads):
    """-> (norm from the kernel's partials summed in float64, the partials buffer, G)"""
    from bmnas import lib
    tab, chunks, n = _table(grads)
    parts = lib.grad_norm_parts()
    assert 0 < parts <= 256
    G = min(n, parts)
    buf = torch.full((parts + 8,), float('nan'), device=dev())
    lib.grad_sqnorm_multi(tab, chunks, n, buf)
    torch.cuda.synchronize()
    assert bool(torch.isnan(buf[G:]).all())                            # G partials written, nothing else
    return float(np.sqrt(buf[:G].double().sum().item())), buf, G


@pytest.mark.parametrize('offset', [0, 1], ids=['aligned', 'offset1'])
def test_norm_kernel_against_float64(offset):
    """304 chunks on the fixed grid of 256 workgroups: the grid-stride loop runs twice for 48 of them and ends ragged.
    offset 1: every gradient 4 bytes off the 16-byte alignment (the element-by-element branch), NaN on both sides."""
    from bmnas import lib
    host = _make(11, [(n,) for n in NORM_SIZES])
    grads = []
    for t in host:
        store = torch.full((t.numel() + 2 * offset,), float('nan'), device=dev())
        view = store[offset:offset + t.numel()]
        view.copy_(t)
        assert view.data_ptr() % 16 == 4 * offset
        grads.append(view)
    grads.insert(3, None)                                              # a parameter without a gradient: left out
    ref = clip_ref.grad_norm(host)
    got, buf, G = _sqnorm(grads)
    assert G == lib.grad_norm_parts() < sum((n + 1023) // 1024 for n in NORM_SIZES)
    print(f'norm {got!r} ref {ref!r} rel {abs(got - ref) / ref:.3e}')
    assert abs(got - ref) <= NORM_TOL * ref
    again, buf2, _ = _sqnorm(grads)
    assert torch.equal(buf[:G].view(torch.int32), buf2[:G].view(torch.int32))      # two calls: identical bits


def test_norm_kernel_fewer_chunks_than_the_grid():
    host = _make(12, [(n,) for n in NORM_SIZES[:6]])
    got, _, G = _sqnorm([t.to(dev()) for t in host])
    ref = clip_ref.grad_norm(host)
    assert G == 11
    assert abs(got - ref) <= NORM_TOL * ref


def _groups(ps):
    return [{'params': ps[:3]}, {'params': ps[3:], 'lr': 3e-3}]


def _run_pair(wd, max_norm, steps=6, edit=None, seed=1):
    """test_adam_matches_torch's layout — two groups, parameter 2 joining at step 2, a per-step lr schedule — with
    clipping: torch on the CPU (clip_grad_norm_ + Adam) beside bmnas.optim.Adam(max_grad_norm=...).
    edit: {step: new max_norm} applied in front of that step.  -> cpu params, gpu params, ref, opt, norms"""
    from bmnas.optim import Adam
    init = _make(seed, SHAPES)
    cpu = [t.double().requires_grad_(True) for t in init]
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in init]
    ref = torch.optim.Adam(_groups(cpu), lr=1e-2, weight_decay=wd)
    opt = Adam(_groups(gpu), lr=1e-2, weight_decay=wd, max_grad_norm=max_norm)
    norms = []
    for step in range(steps):
        if edit and step in edit:
            max_norm = opt.max_grad_norm = edit[step]
        grads = _make(100 + step, SHAPES)
        for i, (c, g_, gr) in enumerate(zip(cpu, gpu, grads)):
            if i == 2 and step < 2:
                c.grad, g_.grad = None, None
                continue
            c.grad, g_.grad = gr.double(), gr.clone().to(dev())
        for grp_c, grp_g in zip(ref.param_groups, opt.param_groups):
            grp_c['lr'] = grp_g['lr'] = grp_c['lr'] * 0.9
        before = [None if g_.grad is None else g_.grad.clone() for g_ in gpu]
        want_norm = float(torch.nn.utils.clip_grad_norm_(cpu, max_norm))
        ref.step()
        opt.step()
        assert opt.last_grad_norm.dim() == 0 and opt.last_grad_norm.dtype == torch.float32 and opt.last_grad_norm.is_cuda
        norms.append((float(opt.last_grad_norm), want_norm))
        for g_, b in zip(gpu, before):                                 # `.grad` is left unclipped
            assert (g_.grad is None and b is None) or torch.equal(g_.grad, b)
    return cpu, gpu, ref, opt, norms


def _assert_matches(cpu, gpu, ref, opt):
    worst = 0.0
    for c, g_ in zip(cpu, gpu):
        scale = float(c.detach().abs().max()) + 1e-3
        err = float((g_.detach().cpu().double() - c.detach()).abs().max())
        worst = max(worst, err / scale)
        assert err <= 2e-6 * scale + 1e-7, (err, scale)
    sd_ref, sd = ref.state_dict(), opt.state_dict()
    for k in sd_ref['state']:
        assert float(sd['state'][k]['step']) == float(sd_ref['state'][k]['step'])
        for name in ('exp_avg', 'exp_avg_sq'):
            a, b = sd['state'][k][name].cpu().double(), sd_ref['state'][k][name]
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            worst = max(worst, err / max(scale, 1e-30))
            assert err <= 2e-6 * scale + 1e-12, (name, k, err, scale)
    print(f'worst error / scale over parameters and moments: {worst:.3e}')


@pytest.mark.parametrize('wd', [1e-4, 0.0])
def test_clipped_step_matches_torch(wd):
    """randn gradients (norm ~ 394) clipped to 5: the coefficient is ~ 0.0127, so at wd = 1e-4 the weight-decay term is
    ~ 1 % of the clipped gradient — clipping after it instead of before would move the moments by that much."""
    cpu, gpu, ref, opt, norms = _run_pair(wd, 5.0)
    for got, want in norms:
        print(f'norm {got!r} torch {want!r}')
        assert 380 < want < 400 and abs(got - want) <= NORM_TOL * want
    _assert_matches(cpu, gpu, ref, opt)
    assert 'max_grad_norm' not in opt.param_groups[0] and 'max_grad_norm' not in opt.state_dict()['param_groups'][0]


def _bits_equal(a_opt, a_params, b_opt, b_params):
    for a, b in zip(a_params, b_params):
        assert torch.equal(a.detach().view(torch.int32), b.detach().view(torch.int32))
    for a, b in zip(a_params, b_params):
        if a in a_opt.state:
            for name in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(a_opt.state[a][name].view(torch.int32), b_opt.state[b][name].view(torch.int32)), name


@pytest.mark.parametrize('zero', [False, True], ids=['randn', 'zero_grads'])
def test_norm_below_the_threshold_leaves_the_unclipped_bits(zero):
    """max_grad_norm = 1e6: the coefficient is exactly 1 and g * 1.0f == g, so six steps give the bits of an optimizer
    without clipping.  All-zero gradients: norm 0, 1e6 / 1e-6 clamps to 1 (weight decay still moves the parameters)."""
    from bmnas.optim import Adam
    init = _make(2, SHAPES)
    a = [t.clone().to(dev()).requires_grad_(True) for t in init]
    b = [t.clone().to(dev()).requires_grad_(True) for t in init]
    clipped = Adam(_groups(a), lr=1e-2, weight_decay=1e-4, max_grad_norm=1e6)
    plain = Adam(_groups(b), lr=1e-2, weight_decay=1e-4)
    assert plain.last_grad_norm is None and plain.grad_norms is None
    for step in range(6):
        for i, (pa, pb, gr) in enumerate(zip(a, b, _make(200 + step, SHAPES))):
            if i == 2 and step < 2:
                pa.grad, pb.grad = None, None
                continue
            if zero:
                gr = torch.zeros_like(gr)
            pa.grad, pb.grad = gr.clone().to(dev()), gr.clone().to(dev())
        clipped.step()
        plain.step()
    torch.cuda.synchronize()
    if zero:
        assert float(clipped.last_grad_norm) == 0.0
    else:
        assert 380 < float(clipped.last_grad_norm) < 400
    _bits_equal(clipped, a, plain, b)
    assert not torch.equal(a[0].detach().cpu(), init[0])


def test_a_nan_gradient_makes_every_parameter_nan():
    """What the trainer loops' nan_escape relies on: one NaN gradient element -> NaN norm -> NaN coefficient (compare and
    select, as torch.clamp) -> every parameter of the optimizer NaN, as with torch.  Plain arithmetic."""
    from bmnas.optim import Adam
    init = _make(3, SHAPES)
    cpu = [t.clone().requires_grad_(True) for t in init]
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in init]
    grads = _make(300, SHAPES)
    grads[4][7, 1] = float('nan')
    for c, g_, gr in zip(cpu, gpu, grads):
        c.grad, g_.grad = gr.clone(), gr.clone().to(dev())
    ref = torch.optim.Adam(_groups(cpu), lr=1e-2, weight_decay=1e-4)
    opt = Adam(_groups(gpu), lr=1e-2, weight_decay=1e-4, max_grad_norm=5.0)
    torch.nn.utils.clip_grad_norm_(cpu, 5.0)
    ref.step()
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isnan(opt.last_grad_norm))
    for c, g_ in zip(cpu, gpu):
        assert bool(torch.isnan(c.detach()).all()) and bool(torch.isnan(g_.detach()).all())


def test_max_grad_norm_edited_between_two_eager_steps():
    """5.0 for the first step, 50.0 for the second: the moments carry the coefficient (exp_avg linearly), so the second
    step's value shows at the parameter tolerance; the switch to None / back rebuilds the plan."""
    from bmnas import lib
    cpu, gpu, ref, opt, norms = _run_pair(1e-4, 5.0, steps=2, edit={1: 50.0})
    _assert_matches(cpu, gpu, ref, opt)
    stale = _run_pair(1e-4, 5.0, steps=2)[1]
    assert float((stale[0].detach() - gpu[0].detach()).abs().max()) > 1e-4          # the edit did change the step
    with pytest.raises(lib.BmnasError):
        opt.max_grad_norm = -1.0
        opt.step()
    opt.max_grad_norm = None
    opt.step()
    assert opt.last_grad_norm is None


def test_stand_alone_clip_grad_norm():
    from bmnas import lib
    from bmnas.optim import clip_grad_norm_
    shapes = SHAPES + [(300001,)]
    host = _make(4, shapes)
    cpu = [torch.zeros(*s, dtype=torch.float64).requires_grad_(True) for s in shapes]
    gpu = [torch.zeros(*s, device=dev()).requires_grad_(True) for s in shapes]
    for i, (c, g_, gr) in enumerate(zip(cpu, gpu, host)):
        if i == 2:
            continue                                                   # no gradient: left out
        c.grad, g_.grad = gr.double(), gr.clone().to(dev())
    for max_norm in (5.0, 1e6):
        want = torch.nn.utils.clip_grad_norm_(cpu, max_norm)
        got = clip_grad_norm_(gpu, max_norm)
        assert got.is_cuda and got.dim() == 0
        print(f'norm {float(got)!r} torch {float(want)!r}')
        assert abs(float(got) - float(want)) <= NORM_TOL * float(want)
        for c, g_ in zip(cpu, gpu):
            if c.grad is None:
                assert g_.grad is None
                continue
            err = (g_.grad.cpu().double() - c.grad).abs()
            assert bool((err <= 1e-6 * c.grad.abs()).all()), float((err / c.grad.abs().clamp_min(1e-30)).max())
    # what it does not cover goes to torch's function
    p = torch.zeros(5, requires_grad=True)
    p.grad = torch.full((5,), 2.0)
    assert abs(float(clip_grad_norm_([p], 1.0)) - 2.0 * 5 ** 0.5) < 1e-5 and abs(float(p.grad.norm()) - 1.0) < 1e-5
    q = torch.zeros(5, device=dev(), requires_grad=True)
    q.grad = torch.full((5,), 3.0, device=dev())
    assert abs(float(clip_grad_norm_(q, 1.0, norm_type=float('inf'))) - 3.0) < 1e-6
    # ... and a capture is refused, naming the optimizer form
    x = torch.zeros(4, device=dev())
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        x.add_(1.0)
        with pytest.raises(lib.BmnasError, match='max_grad_norm'):
            clip_grad_norm_(gpu, 5.0)
    torch.cuda.current_stream().wait_stream(s)


def test_captured_clipped_step_replays_with_an_edited_max_grad_norm():
    """capture_safe() + a captured step(): partials, clip scalar and norm output are the plan's; max_grad_norm travels with
    the staged scalars, so an edit takes effect at the next replay without re-capture (copy-node and poke plans)."""
    from bmnas import lib
    from bmnas.optim import Adam
    for poke in (False, True):
        init = _make(5, SHAPES)
        cpu = [t.double().requires_grad_(True) for t in init]
        gpu = [t.clone().to(dev()).requires_grad_(True) for t in init]
        ref = torch.optim.Adam(cpu, lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-3)
        opt = Adam(gpu, lr=1e-2, betas=(0.5, 0.999), weight_decay=1e-3, max_grad_norm=5.0)
        for g_ in gpu:
            g_.grad = torch.zeros_like(g_)
        opt.capture_safe(poke=poke)
        graph = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
            opt.step()
        torch.cuda.current_stream().wait_stream(s)
        plan = opt.captured_plan()
        assert plan['poke'] == poke
        static = [g_.grad for g_ in gpu]
        for step in range(5):
            max_norm = opt.max_grad_norm = 5.0 if step < 2 else 40.0
            grads = _make(70 + step, SHAPES)
            for c, s_, gr in zip(cpu, static, grads):
                c.grad = gr.double()
                s_.copy_(gr)
            want = float(torch.nn.utils.clip_grad_norm_(cpu, max_norm))
            ref.step()
            if step == 3:
                # an eager step in between, on brand-new gradient tensors: a plan of its own (with its own partials, clip
                # scalar and norm output); activate() then brings the captured plan's back
                for g_, gr in zip(gpu, grads):
                    g_.grad = gr.clone().to(dev())
                opt.step()
                assert opt._plan is not plan and abs(float(opt.last_grad_norm) - want) <= NORM_TOL * want
                continue
            opt.activate(plan)
            opt.wait_staging()
            opt.prepare_replay()
            blob = opt.replay_blob()
            if poke:
                lib.copy_batch([], blob)
            else:
                assert blob is None
            graph.replay()
            opt.mark_launched()
            assert abs(float(opt.last_grad_norm) - want) <= NORM_TOL * want
        torch.cuda.synchronize()
        _assert_matches(cpu, gpu, ref, opt)
