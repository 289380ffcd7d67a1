"""-m gpu: the one-launch SGD step (csrc/adam.hip: sgd_multi_k; bmnas_sgd_multi; bmnas.optim.SGD) against torch.optim.SGD on
the CPU in float64 and against tests/sgd_ref.py.

Layout: tests/test_adam_variants_gpu.py's (tests/sgd_ref.py holds it) — SHAPES, two groups (the second with lr 3e-3),
parameter 2 joining at step 2 (its first-step rule runs in a launch where the others are past theirs), lr *= 0.9 per step,
6 steps, step s's randn gradients times MULT[s].

Tolerance: the project's optimizer tolerance, 2e-6 of the tensor's scale (test_optim_gpu.py), for parameters and
momentum_buffer — the kernel's own arithmetic, fp32 operation by operation, is within a quarter of it (5e-7 of scale) from
float64 on these inputs, which tests/test_sgd_ref.py asserts.  Every comparison case first shows, on the float64 references
alone, that it is >= 100 x that tolerance away from the configuration it could be confused with.

Bit properties: the kernel contracts nothing into a fused multiply-add, so sgd_ref's fp32 mode — numpy, every operation
rounded on its own — is its bit-for-bit reference.  A clip coefficient below 1 is rebuilt on the host from the norm the
launch itself reports (norm_out): c = max_norm / (norm + 1e-6) in fp32, one correctly rounded add and divide, as
clip_coef computes it."""
import copy

import numpy as np
import pytest
import torch

import clip_ref
import sgd_ref
from gpu_util import dev
from sgd_ref import CASES, LR, NEIGHBOUR, SHAPES, ctor_args, decay_lr, grads_of, groups, make

pytestmark = pytest.mark.gpu

TOL = 2e-6
SIZES = [1, 3, 1023, 1024, 1025, 4099]
PAD = 4                                   # guard floats on each side of a directly driven buffer (keeps 16-byte alignment)


def _bits(t):
    return t.detach().view(torch.int32)


def _np_bits(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).view(torch.int32)


def _set_grads(step, gpu, **kw):
    for p, g in zip(gpu, grads_of(step, **kw)):
        p.grad = None if g is None else g.clone().to(dev())


def _gpu_run(cfg, seed=1, steps=sgd_ref.STEPS, after=None):
    """bmnas.optim.SGD on the GPU over the inputs of sgd_ref.torch_run -> (parameters, optimizer)"""
    from bmnas.optim import SGD
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(seed)]
    opt = SGD(groups(gpu, cfg), lr=LR, max_grad_norm=cfg.get('max_norm'), **ctor_args(cfg))
    for step in range(steps):
        _set_grads(step, gpu)
        decay_lr(opt)
        opt.step()
        if after is not None:
            after(step, gpu, opt)
    torch.cuda.synchronize()
    return gpu, opt


def _assert_matches(cpu, gpu, ref, opt, label=''):
    worst = 0.0
    for c, g_ in zip(cpu, gpu):
        scale = float(c.detach().abs().max()) + 1e-3
        err = float((g_.detach().cpu().double() - c.detach().double()).abs().max())
        worst = max(worst, err / scale)
        assert err <= TOL * scale + 1e-7, (err, scale)
    sd_ref, sd = ref.state_dict(), opt.state_dict()
    assert set(sd_ref['state']) == set(sd['state'])
    for k in sd_ref['state']:
        assert set(sd['state'][k]) == set(sd_ref['state'][k]) == {'momentum_buffer'}
        a, b = sd['state'][k]['momentum_buffer'].cpu().double(), sd_ref['state'][k]['momentum_buffer'].double()
        err, scale = float((a - b).abs().max()), float(b.abs().max())
        worst = max(worst, err / max(scale, 1e-30))
        assert err <= TOL * scale + 1e-12, (k, err, scale)
    print(f'{label} worst error / scale over parameters and momentum_buffer: {worst:.3e}')


@pytest.mark.parametrize('name', list(CASES))
def test_case_matches_torch(name):
    cfg = CASES[name]
    cpu, ref = sgd_ref.torch_cached(name)
    if name in NEIGHBOUR:
        apart = sgd_ref.distance(cpu, sgd_ref.torch_cached(NEIGHBOUR[name])[0])
        print(f'float64: {name} against {NEIGHBOUR[name]} {apart:.3e} of scale')
        assert apart >= 100 * TOL                                      # the comparison below cannot pass vacuously
    gpu, opt = _gpu_run(cfg)
    _assert_matches(cpu, gpu, ref, opt, name)
    assert opt._plan['flags'] == (1 if cfg['momentum'] else 0) | (2 if cfg.get('nesterov') else 0)
    sd = opt.state_dict()
    assert sd['param_groups'] == ref.state_dict()['param_groups']      # torch's keys and values, nothing else
    if name == 'plain':
        assert len(sd['state']) == 0


def test_small_weight_decay_matches_too():
    """weight_decay 3e-4 is only 3.3e-5 of scale from no decay — too little to serve as THE decay case, still compared"""
    cfg = dict(momentum=0.9, weight_decay=3e-4)
    cpu, ref = sgd_ref.torch_run(cfg)
    gpu, opt = _gpu_run(cfg)
    _assert_matches(cpu, gpu, ref, opt, 'wd 3e-4')


# ---------------------------------------------------------------------------------------------- the C ABI, driven directly
def _guarded(host, offset):
    """host tensor -> (view at PAD + offset floats into a NaN-filled store with PAD + 1 spare floats behind, the store)"""
    n = host.numel()
    store = torch.full((n + 2 * PAD + 1,), float('nan'), device=dev())
    view = store[PAD + offset:PAD + offset + n]
    view.copy_(host.reshape(-1))
    assert view.data_ptr() % 16 == 4 * offset
    return view, store


class _Direct:
    """Device tensors + bmnas_adam_tensor_t[] + chunk list for a direct call; one scalar row for all tensors.
    off: which buffers sit one float off the 16-byte alignment; buf: 'rand' | 'zero' | None (a null pointer)."""

    def __init__(self, sizes, seed, off=(), buf='rand'):
        from bmnas import lib
        from bmnas.optim import _DESC
        shapes = [(n,) for n in sizes]
        self.sizes = sizes
        self.host = {'p': make(seed, shapes), 'g': make(seed + 1, shapes)}
        if buf is not None:
            self.host['b'] = [(0.1 if buf == 'rand' else 0.0) * t for t in make(seed + 2, shapes)]
        self.dev, self.stores = {}, {}
        for k, ts in self.host.items():
            pairs = [_guarded(t, 1 if k in off else 0) for t in ts]
            self.dev[k], self.stores[k] = [v for v, _ in pairs], [s for _, s in pairs]
        self.guard_bits = {k: [_bits(s).clone() for s in ss] for k, ss in self.stores.items()}
        E = lib.adam_chunk_elems()
        tab = np.zeros(len(sizes), dtype=_DESC)
        for field, k in (('param', 'p'), ('grad', 'g'), ('exp_avg', 'b')):
            if k in self.dev:
                tab[field] = [t.data_ptr() for t in self.dev[k]]
        tab['numel'] = sizes
        chunks = [(i, c) for i, n in enumerate(sizes) for c in range((n + E - 1) // E)]
        self.tab = torch.from_numpy(tab.view(np.uint8)).to(dev())
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev())
        self.n = len(chunks)
        self.partials = torch.empty(lib.grad_norm_parts(), device=dev())
        self.n_parts = min(self.n, lib.grad_norm_parts())
        self.clip = torch.tensor([5.0], device=dev())
        self.norm = torch.zeros(1, device=dev())

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: [t.clone() for t in v] for k, v in self.dev.items()}

    def check_guards(self, untouched=()):
        """The floats around every view are bit-unchanged (`untouched`: these buffers' views as well)."""
        torch.cuda.synchronize()
        for k, ss in self.stores.items():
            for i, (s, was) in enumerate(zip(ss, self.guard_bits[k])):
                n, o = self.sizes[i], PAD + (1 if self.dev[k][i].data_ptr() % 16 else 0)
                now = _bits(s)
                assert torch.equal(now[:o], was[:o]) and torch.equal(now[o + n:], was[o + n:]), (k, i)
                if k in untouched:
                    assert torch.equal(now, was), (k, i)


def _hyp(lr, mu, damp, wd, first=False):
    return torch.tensor([[-lr, 0.0 if first else mu, 1.0 if first else 1 - damp, mu, wd, 0, 0, 0]], dtype=torch.float32,
                        device=dev())


MODES = {'plain': dict(flags=0, mu=0.0, damp=0.0, wd=0.1, clipped=False),
         'momentum': dict(flags=1, mu=0.9, damp=0.5, wd=0.1, clipped=False),
         'nesterov_clipped': dict(flags=3, mu=0.9, damp=0.0, wd=0.1, clipped=True)}


@pytest.mark.parametrize('off', [(), ('p',), ('b',)], ids=['aligned', 'param_offset1', 'buffer_offset1'])
@pytest.mark.parametrize('mode', list(MODES))
def test_direct_call_against_float64(mode, off):
    """bmnas_sgd_multi on a hand-built table, tensors of 1 ... 4099 elements: all buffers 16-byte aligned (float4 path with
    the scalar tail), or the parameter / the momentum buffer 4 bytes off it (their pointers are part of the test that
    selects the float4 branch: the scalar path runs), NaN guards on both sides of every buffer."""
    from bmnas import lib
    m = MODES[mode]
    if off == ('b',) and not m['flags']:
        off = ('g',)                                   # no buffer without momentum: the gradient is the one off alignment
    d = _Direct(SIZES, 30, off, buf='rand' if m['flags'] else None)
    lr = 1e-2
    hyp = _hyp(lr, m['mu'], m['damp'], m['wd'])
    grads = d.host['g']
    if m['clipped']:
        lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
        lib.sgd_multi(d.tab, d.chunks, d.n, hyp, m['flags'], d.partials, d.n_parts, d.clip, d.norm)
        grads, norm = clip_ref.clip(grads, 5.0)
    else:
        lib.sgd_multi(d.tab, d.chunks, d.n, hyp, m['flags'])
    got = d.snapshot()
    d.check_guards(untouched=('g',))                                     # `.grad` is not written
    if m['clipped']:
        assert norm > 5.0 and abs(float(d.norm) - norm) <= 2e-5 * norm
    for i in range(len(SIZES)):
        buf = d.host['b'][i] if m['flags'] else None
        want_p, want_b = sgd_ref.sgd_step(d.host['p'][i], grads[i], buf, lr, m['mu'], m['damp'], m['wd'], m['flags'] == 3)
        pairs = [('p', want_p)] + ([('b', want_b)] if m['flags'] else [])
        for k, w in pairs:
            err = np.abs(got[k][i].cpu().double().numpy() - w).max()
            assert err <= TOL * np.abs(w).max() + 1e-12, (k, i, err)
        assert not torch.equal(got['p'][i].cpu(), d.host['p'][i])


def test_direct_call_is_fp32_operation_by_operation():
    """Unclipped: the bits of sgd_ref's fp32 mode (numpy, one rounding per operation) — no fused multiply-add in the
    kernel, on the float4 path and on the scalar one."""
    from bmnas import lib
    for off in ((), ('p',)):
        for flags, mu, damp in ((0, 0.0, 0.0), (1, 0.9, 0.5), (3, 0.9, 0.0)):
            d = _Direct(SIZES, 60, off, buf='rand' if flags else None)
            lib.sgd_multi(d.tab, d.chunks, d.n, _hyp(1e-2, mu, damp, 0.1), flags)
            got = d.snapshot()
            for i in range(len(SIZES)):
                buf = d.host['b'][i] if flags else None
                want_p, want_b = sgd_ref.sgd_step(d.host['p'][i], d.host['g'][i], buf, 1e-2, mu, damp, 0.1, flags == 3,
                                                  dtype=np.float32)
                assert torch.equal(_bits(got['p'][i].cpu()), _np_bits(want_p)), (off, flags, i)
                if flags:
                    assert torch.equal(_bits(got['b'][i].cpu()), _np_bits(want_b)), (off, flags, i)


def _host_coef(norm_out, max_norm):
    """clip_coef's coefficient from the norm the launch reported, in fp32: one add, one divide, compare and select"""
    c = np.float32(max_norm) / (norm_out.cpu().numpy()[0] + np.float32(1e-6))
    assert c.dtype == np.float32
    return np.float32(1.0) if c > 1 else c


def test_first_step_row_leaves_the_buffer_equal_to_the_clipped_and_decayed_gradient():
    """mu = 0, damp1 = 1 over a zero buffer: buf = 0 * 0 + 1 * g' = g', bit for bit, with g' = c * g + wd * p formed in fp32
    operation by operation and c rebuilt from the launch's own norm_out — at max_norm = 5, where the clip bites (c < 1: a
    clip product contracted into the decay add would show), and at max_norm = 1e30 (c == 1 exactly).  The parameter too:
    p + (-lr) * g'.  Beside it, torch's first step in float64 with the float64 norm, at the tolerance."""
    from bmnas import lib
    wd, mu, lr = 0.1, 0.9, 1e-2
    for clip_at in (5.0, 1e30):
        d = _Direct(SIZES, 70, buf='zero')
        d.clip.fill_(clip_at)
        lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
        lib.sgd_multi(d.tab, d.chunks, d.n, _hyp(lr, mu, 0.5, wd, first=True), 1, d.partials, d.n_parts, d.clip, d.norm)
        got = d.snapshot()
        d.check_guards(untouched=('g',))
        grads, norm = clip_ref.clip(d.host['g'], clip_at)
        assert (norm > clip_at) == (clip_at == 5.0) and abs(float(d.norm) - norm) <= 2e-5 * norm
        c = _host_coef(d.norm, clip_at)
        assert (c < 1) == (clip_at == 5.0)
        for i in range(len(SIZES)):
            want = c * d.host['g'][i].numpy() + np.float32(wd) * d.host['p'][i].numpy()         # fp32, op by op
            assert want.dtype == np.float32
            assert torch.equal(_bits(got['b'][i].cpu()), _np_bits(want)), (clip_at, i)
            want_p = d.host['p'][i].numpy() + np.float32(-lr) * want
            assert torch.equal(_bits(got['p'][i].cpu()), _np_bits(want_p)), (clip_at, i)
            # ... and torch's first step in float64: buf = clone(g'), dampening (0.5 here) not applied
            want_p, want_b = sgd_ref.sgd_step(d.host['p'][i], grads[i], None, lr, mu, 0.5, wd)
            for k, w in (('p', want_p), ('b', want_b)):
                err = np.abs(got[k][i].cpu().double().numpy() - w).max()
                assert err <= TOL * np.abs(w).max() + 1e-12, (k, i, err)


def test_clipped_direct_call_is_fp32_operation_by_operation():
    """A clip that bites, every instantiation, aligned and with the parameter one float off: the bits of sgd_ref's fp32
    sequence over gradients scaled by the coefficient rebuilt from norm_out."""
    from bmnas import lib
    for off in ((), ('p',)):
        for flags, mu, damp in ((0, 0.0, 0.0), (1, 0.9, 0.5), (3, 0.9, 0.0)):
            d = _Direct(SIZES, 65, off, buf='rand' if flags else None)
            lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
            lib.sgd_multi(d.tab, d.chunks, d.n, _hyp(1e-2, mu, damp, 0.1), flags, d.partials, d.n_parts, d.clip, d.norm)
            got = d.snapshot()
            c = _host_coef(d.norm, 5.0)
            assert c < 1
            for i in range(len(SIZES)):
                buf = d.host['b'][i] if flags else None
                want_p, want_b = sgd_ref.sgd_step(d.host['p'][i], c * d.host['g'][i].numpy(), buf, 1e-2, mu, damp, 0.1,
                                                  flags == 3, dtype=np.float32)
                assert torch.equal(_bits(got['p'][i].cpu()), _np_bits(want_p)), (off, flags, i)
                if flags:
                    assert torch.equal(_bits(got['b'][i].cpu()), _np_bits(want_b)), (off, flags, i)


def test_without_momentum_a_null_buffer_is_accepted():
    from bmnas import lib
    d = _Direct(SIZES, 80, buf=None)
    lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
    lib.sgd_multi(d.tab, d.chunks, d.n, _hyp(1e-2, 0.0, 0.0, 0.0), 0, d.partials, d.n_parts, d.clip, d.norm)
    got = d.snapshot()
    d.check_guards(untouched=('g',))
    grads, _ = clip_ref.clip(d.host['g'], 5.0)
    for i in range(len(SIZES)):
        want_p, _ = sgd_ref.sgd_step(d.host['p'][i], grads[i], None, 1e-2)
        assert np.abs(got['p'][i].cpu().double().numpy() - want_p).max() <= TOL * np.abs(want_p).max() + 1e-12


def test_rejected_arguments_launch_nothing():
    from bmnas import lib
    d = _Direct([1025, 7], 40)
    hyp = _hyp(1e-2, 0.9, 0.0, 0.1)
    lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
    before = d.snapshot()
    M, N = lib.SGD_MOMENTUM, lib.SGD_NESTEROV
    clip = (d.partials, d.n_parts, d.clip, d.norm)
    bad = [
        (4,), (M | 8,), (-1,),                                                         # unknown flag bits
        (N,), (N,) + clip,                                                             # nesterov without momentum
        (M, d.partials, d.n_parts, None, None), (M, d.partials, d.n_parts, d.clip, None),    # partials / clip /
        (M, None, 0, d.clip, d.norm), (M, None, 0, None, d.norm), (0, None, 0, d.clip, None),    # norm_out: not all set
        (M, d.partials, d.n_parts + 1, d.clip, d.norm), (M, d.partials, 0, d.clip, d.norm),  # not what the norm launch
        (M | N, d.partials, 256, d.clip, d.norm),                                            # wrote
    ]
    for args in bad:
        with pytest.raises(lib.BmnasError, match='bad argument'):
            lib.sgd_multi(d.tab, d.chunks, d.n, hyp, *args)
    # null pointers and a negative chunk count: through the raw entry point
    raw = lib.load().bmnas_sgd_multi
    stream = torch.cuda.current_stream().cuda_stream
    t, c, h = d.tab.data_ptr(), d.chunks.data_ptr(), hyp.data_ptr()
    for a in ((None, c, d.n, h), (t, None, d.n, h), (t, c, d.n, None), (t, c, -1, h)):
        assert raw(*a, M, None, 0, None, None, stream) == -1
    assert raw(t, c, 0, h, M, d.partials.data_ptr(), 0, d.clip.data_ptr(), d.norm.data_ptr(), stream) == -1
    assert raw(t, c, 0, h, M, None, 0, None, None, stream) == 0                          # nothing to do: no error
    after = d.snapshot()
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert torch.equal(_bits(x), _bits(y)), k
    assert float(d.norm) == 0.0
    d.check_guards(untouched=('p', 'g', 'b'))
    lib.sgd_multi(d.tab, d.chunks, d.n, hyp, M | N, *clip)                                # the accepted form does launch
    assert not torch.equal(_bits(d.snapshot()['p'][0]), _bits(before['p'][0]))


# ---------------------------------------------------------------------------------------------------------- bit properties
def _same_bits(a, opt_a, b, opt_b):
    for pa, pb in zip(a, b):
        assert torch.equal(_bits(pa), _bits(pb))
        ba, bb = opt_a.state.get(pa, {}).get('momentum_buffer'), opt_b.state.get(pb, {}).get('momentum_buffer')
        assert (ba is None) == (bb is None)
        if ba is not None:
            assert torch.equal(_bits(ba), _bits(bb))


def test_a_clip_that_never_bites_leaves_the_bits_and_two_runs_agree():
    cfg = dict(momentum=0.9, dampening=0.5, weight_decay=0.1, nesterov=False)
    a, opt_a = _gpu_run(dict(cfg, max_norm=1e30), seed=2)
    b, opt_b = _gpu_run(cfg, seed=2)
    assert opt_a._plan['clip'] and not opt_b._plan['clip']
    assert float(opt_a.last_grad_norm) > 0 and opt_b.last_grad_norm is None
    _same_bits(a, opt_a, b, opt_b)
    c, opt_c = _gpu_run(dict(cfg, max_norm=1e30), seed=2)                # two runs: identical bits
    _same_bits(a, opt_a, c, opt_c)
    assert not torch.equal(a[0].detach().cpu(), make(2)[0])


@pytest.mark.parametrize('nesterov', [False, True], ids=['momentum', 'nesterov'])
def test_zero_decay_and_zero_dampening_leave_the_bits_of_the_sequence_without_them(nesterov):
    """The whole six-step run, late tensor and first-step rows included, against the fp32 reference sequence in which the
    decay term and the dampening product do not exist."""
    cfg = dict(momentum=0.9, dampening=0.0, weight_decay=0.0, nesterov=nesterov)
    gpu, opt = _gpu_run(cfg, seed=3)
    P, B, _ = sgd_ref.ref_run(cfg, seed=3, dtype=np.float32, plain_terms=True)
    for i, p in enumerate(gpu):
        assert torch.equal(_bits(p.cpu()), _np_bits(P[i]).view(p.shape)), i
        assert torch.equal(_bits(opt.state[p]['momentum_buffer'].cpu()), _np_bits(B[i]).view(p.shape)), i


def test_clipped_step_leaves_grad_unclipped_and_reports_the_norm():
    from bmnas.optim import SGD
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(5)]
    opt = SGD(groups(gpu), lr=LR, momentum=0.9, max_grad_norm=5.0)
    _set_grads(0, gpu, late=False)
    before = [_bits(p.grad).clone() for p in gpu]
    opt.step()
    torch.cuda.synchronize()
    assert all(torch.equal(_bits(p.grad), b) for p, b in zip(gpu, before))
    norm = clip_ref.grad_norm(grads_of(0, late=False))
    assert norm > 5.0 and abs(float(opt.last_grad_norm) - norm) <= 2e-5 * norm
    assert opt.grad_norms.shape == (1,)


def test_a_nan_gradient_element_makes_every_parameter_nan_under_clipping():
    from bmnas.optim import SGD
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(6)]
    opt = SGD(groups(gpu), lr=LR, momentum=0.9, max_grad_norm=5.0)
    _set_grads(0, gpu, late=False)
    gpu[4].grad[7, 1] = float('nan')
    opt.step()
    torch.cuda.synchronize()
    assert bool(torch.isnan(opt.last_grad_norm))
    for p in gpu:
        assert bool(torch.isnan(p).all()) and bool(torch.isnan(opt.state[p]['momentum_buffer']).all())


# ------------------------------------------------------------------------------------------------------------ checkpoints
CKPT = dict(momentum=0.9, dampening=0.5, weight_decay=0.1)
CK_SHAPES = SHAPES[1:5]


def _ck_grads(step, cpu, gpu):
    for i, g in enumerate(make(50 + step, CK_SHAPES, sgd_ref.MULT[step])):
        if cpu is not None:
            cpu[i].grad = g.double()
        if gpu is not None:
            gpu[i].grad = g.clone().to(dev())


def test_a_torch_checkpoint_continues_here():
    from bmnas.optim import SGD
    cpu = [t.double().requires_grad_(True) for t in make(2, CK_SHAPES)]
    ref = torch.optim.SGD(cpu, lr=LR, **CKPT)
    for step in range(3):
        _ck_grads(step, cpu, None)
        ref.step()
    gpu = [c.detach().float().to(dev()).requires_grad_(True) for c in cpu]
    opt = SGD(gpu, lr=1.0)                                              # everything else: the checkpoint's
    opt.load_state_dict(copy.deepcopy(ref.state_dict()))
    assert opt.param_groups[0]['momentum'] == 0.9 and opt.param_groups[0]['dampening'] == 0.5
    for step in range(3, 6):
        _ck_grads(step, cpu, gpu)
        ref.step()
        opt.step()
    torch.cuda.synchronize()
    _assert_matches(cpu, gpu, ref, opt, 'torch -> ours')
    # had the restored buffers been taken for unstepped ones, step 3 would have dropped the dampening: far outside TOL
    assert float(opt._plan['hyp'][0][2]) == 0.5 and float(opt._plan['hyp'][0][1]) == np.float32(0.9)


def test_our_checkpoint_loads_into_torch():
    from bmnas.optim import SGD
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(2, CK_SHAPES)]
    opt = SGD(gpu, lr=LR, **CKPT)
    for step in range(3):
        _ck_grads(step, None, gpu)
        opt.step()
    torch.cuda.synchronize()
    cpu = [p.detach().cpu().double().requires_grad_(True) for p in gpu]
    ref = torch.optim.SGD(cpu, lr=1.0)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert ref.state[cpu[0]]['momentum_buffer'].dtype == torch.float64 and ref.param_groups[0]['dampening'] == 0.5
    for step in range(3, 5):
        _ck_grads(step, cpu, gpu)
        ref.step()
        opt.step()
    torch.cuda.synchronize()
    _assert_matches(cpu, gpu, ref, opt, 'ours -> torch')


def test_a_checkpoint_taken_after_capture_safe_keeps_the_first_step_rule():
    """capture_safe() allocates the zero buffers a graph needs; no step has written them, so state_dict() shows none and
    torch's next step is its first one (buf = g, dampening 0.5 NOT applied) — and so is ours."""
    from bmnas.optim import SGD
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(2, CK_SHAPES)]
    opt = SGD(gpu, lr=LR, **CKPT)
    _ck_grads(0, None, gpu)
    opt.capture_safe()
    assert len(opt._pending) == len(gpu) and opt._plan['momentum']
    sd = copy.deepcopy(opt.state_dict())
    assert len(sd['state']) == 0
    cpu = [p.detach().cpu().double().requires_grad_(True) for p in gpu]
    ref = torch.optim.SGD(cpu, lr=1.0)
    ref.load_state_dict(sd)
    for step in range(2):
        _ck_grads(step, cpu, gpu)
        ref.step()
        opt.step()
        if step == 0:
            # the first step: buf = g + wd * p, bit for bit (fp32, operation by operation), not half of it
            torch.cuda.synchronize()
            assert not opt._pending
            for p0, g0, p in zip(make(2, CK_SHAPES), make(50, CK_SHAPES, sgd_ref.MULT[0]), gpu):
                want = g0.numpy() + np.float32(0.1) * p0.numpy()
                assert torch.equal(_bits(opt.state[p]['momentum_buffer'].cpu()), _np_bits(want).view(p.shape))
    torch.cuda.synchronize()
    _assert_matches(cpu, gpu, ref, opt, 'checkpoint before the first step')


def test_groups_that_disagree_and_maximize_are_refused_before_anything_moves():
    from bmnas import lib
    from bmnas.optim import SGD
    for edit in (dict(momentum=0.0), dict(nesterov=True, dampening=0)):
        gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(2, CK_SHAPES)]
        opt = SGD(groups(gpu), lr=LR, momentum=0.9)
        opt.param_groups[1].update(edit)
        _ck_grads(0, None, gpu)
        start = [_bits(p).clone() for p in gpu]
        name = 'momentum' if 'momentum' in edit else 'nesterov'
        with pytest.raises(lib.BmnasError, match=f"param_groups disagree on '{name}'"):
            opt.step()
        with pytest.raises(lib.BmnasError, match=f"param_groups disagree on '{name}'"):
            opt.capture_safe()
        torch.cuda.synchronize()
        assert not opt.state and not opt._pending and all(torch.equal(_bits(p), s) for p, s in zip(gpu, start))
    with pytest.raises(lib.BmnasError, match='maximize'):
        SGD(gpu, lr=LR, maximize=True)
    opt = SGD(gpu, lr=LR, momentum=0.9)
    with pytest.raises(lib.BmnasError, match='maximize'):
        opt.load_state_dict(torch.optim.SGD(gpu, lr=LR, momentum=0.9, maximize=True).state_dict())
    opt.param_groups[0]['maximize'] = True
    with pytest.raises(lib.BmnasError, match='maximize'):
        opt.step()


def test_a_refused_step_leaves_the_buffers_unstepped():
    """A gradient the step refuses (not contiguous): nothing was staged, so the zero buffers the plan allocated are still
    not state, and the next step is the first one (buf = g, dampening 0.5 not applied)."""
    from bmnas import lib
    from bmnas.optim import SGD
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(2, CK_SHAPES)]
    opt = SGD(gpu, lr=LR, momentum=0.9, dampening=0.5)
    _ck_grads(0, None, gpu)
    good = gpu[3].grad
    gpu[3].grad = torch.zeros(2, 13, device=dev()).t()                  # (13, 2), not contiguous
    start = [_bits(p).clone() for p in gpu]
    with pytest.raises(lib.BmnasError, match='gradients must be contiguous'):
        opt.step()
    torch.cuda.synchronize()
    assert len(opt.state_dict()['state']) == 0 and len(opt._pending) == len(gpu)
    assert all(torch.equal(_bits(p), s) for p, s in zip(gpu, start))
    gpu[3].grad = good
    opt.step()
    torch.cuda.synchronize()
    for p in gpu:
        assert torch.equal(_bits(opt.state[p]['momentum_buffer']), _bits(p.grad))


# --------------------------------------------------------------------------------------------------------------- captured
def _capture(opt, steps=1):
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        for _ in range(steps):
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    return graph


def _new(seed, **kw):
    from bmnas.optim import SGD
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in make(seed)]
    return gpu, SGD(groups(gpu, kw), lr=LR, **{k: v for k, v in kw.items() if k != 'group2'})


CAP = dict(momentum=0.9, dampening=0.5, weight_decay=0.1, max_grad_norm=5.0, group2=dict(momentum=0.5, dampening=0.1))


def _schedule(step, *opts):
    """a new lr per step and an edited max_grad_norm from step 2 on"""
    for opt in opts:
        for gi, grp in enumerate(opt.param_groups):
            grp['lr'] = (LR if gi == 0 else sgd_ref.LR2) * (0.8 ** step)
        opt.max_grad_norm = 5.0 if step < 2 else 2.0


@pytest.mark.parametrize('poke', [False, True], ids=['copy_node', 'poke'])
def test_captured_step_replays_bit_equal_to_eager_steps(poke):
    """One graph, four replays with a new lr and an edited max_grad_norm between them: the first replay is the first step
    of every tensor (rows mu = 0, damp1 = 1 over the zero buffers capture_safe() allocated), the later ones are not — the
    row flip under one graph.  Then an eager step between replays, a restored state between replays (the replay must
    write the NEW buffers), and the refusal of a switch flipped under the captured plan.  Bit-equal to an eager twin;
    the twin against torch in float64."""
    from bmnas import lib
    gpu, opt = _new(4, **CAP)
    twin, opt_t = _new(4, **CAP)
    cpu = [t.double().requires_grad_(True) for t in make(4)]
    ref = torch.optim.SGD(groups(cpu, CAP), lr=LR, **ctor_args({k: v for k, v in CAP.items() if k != 'max_grad_norm'}))
    static = [torch.zeros_like(g_) for g_ in gpu]
    for g_, s_ in zip(gpu, static):
        g_.grad = s_
    opt.capture_safe(poke=poke)
    assert len(opt.state_dict()['state']) == 0
    graph = _capture(opt)
    plan = opt.captured_plan()
    assert plan['poke'] == poke and plan['flags'] == 1 and plan['key'] == (True, True, False)
    assert plan['count'] == [0.0, 0.0]

    def one(step, eager=False):
        _schedule(step, opt, opt_t, ref)
        grads = make(90 + step, SHAPES, sgd_ref.MULT[step % 6])
        for c, t_, gr in zip(cpu, twin, grads):
            c.grad = gr.double()
            t_.grad = gr.clone().to(dev())
        torch.nn.utils.clip_grad_norm_(cpu, opt.max_grad_norm)
        ref.step()
        opt_t.step()
        if eager:                                    # on brand-new gradient tensors: a plan of its own
            for g_, gr in zip(gpu, grads):
                g_.grad = gr.clone().to(dev())
            opt.step()
            assert opt._plan is not plan
            return
        for s_, gr in zip(static, grads):
            s_.copy_(gr)
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

    for step in range(4):
        one(step)
        if step == 0:
            assert [float(r[1]) for r in plan['hyps'][0]] == [0.0, 0.0] and [float(r[2]) for r in plan['hyps'][0]] == [1, 1]
        else:
            assert [float(r[1]) for r in plan['hyps'][0]] == [np.float32(0.9), 0.5]
            assert [float(r[2]) for r in plan['hyps'][0]] == [0.5, np.float32(0.9)]
        assert opt.staged_lrs() == [float(np.float32(g['lr'])) for g in opt.param_groups]
    torch.cuda.synchronize()
    _same_bits(gpu, opt, twin, opt_t)
    assert float(opt.last_grad_norm) == float(opt_t.last_grad_norm) > 2.0
    _assert_matches(cpu, twin, ref, opt_t, 'four replays')
    one(4, eager=True)                               # an eager step between replays
    one(5)
    torch.cuda.synchronize()
    _same_bits(gpu, opt, twin, opt_t)
    # a checkpoint restored between replays
    old = [opt.state[p]['momentum_buffer'] for p in gpu]
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    new = [opt.state[p]['momentum_buffer'] for p in gpu]
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(old, new))
    old_bits = [_bits(t).clone() for t in old]
    one(6)
    torch.cuda.synchronize()
    _same_bits(gpu, opt, twin, opt_t)
    assert all(torch.equal(_bits(t), b) for t, b in zip(old, old_bits))            # the old tensors: no longer written
    _assert_matches(cpu, twin, ref, opt_t, 'after the restored state')
    # ... and one from before the first step: every row is a first-step row again
    gpu2, fresh = _new(4, **CAP)
    opt.load_state_dict(copy.deepcopy(fresh.state_dict()))
    opt_t.load_state_dict(copy.deepcopy(fresh.state_dict()))
    opt.max_grad_norm = opt_t.max_grad_norm = 2.0
    grads = make(97, SHAPES)                          # (the float64 run is not followed past this point)
    for t_, s_, gr in zip(twin, static, grads):
        t_.grad = gr.clone().to(dev())
        s_.copy_(gr)
    opt_t.step()
    opt.activate(plan)
    opt.wait_staging()
    opt.prepare_replay()
    assert [float(r[1]) for r in plan['hyps'][0]] == [0.0, 0.0]
    blob = opt.replay_blob()
    if poke:
        lib.copy_batch([], blob)
    graph.replay()
    opt.mark_launched()
    torch.cuda.synchronize()
    _same_bits(gpu, opt, twin, opt_t)
    # one launch is one instantiation: a switch flipped under the captured plan is refused
    opt.activate(plan)
    for edit in (dict(nesterov=True), dict(momentum=0.0)):
        saved = [dict(g) for g in opt.param_groups]
        for g in opt.param_groups:
            g.update(edit, dampening=0)
        with pytest.raises(lib.BmnasError, match='re-capture'):
            opt.prepare_replay()
        for g, s_ in zip(opt.param_groups, saved):
            g.update(s_)
    opt.max_grad_norm = None
    with pytest.raises(lib.BmnasError, match='re-capture'):
        opt.prepare_replay()


def test_two_steps_per_replay_equal_four_eager_steps():
    """slots = 2 in poke mode: two replays of a two-step graph, each step with its own gradients, lr and max_grad_norm —
    bit-equal to four eager steps; slot 0 of the first replay holds the first-step rows, slot 1 does not."""
    from bmnas import lib
    gpu, opt = _new(8, **CAP)
    twin, opt_t = _new(8, **CAP)
    statics = [[torch.zeros_like(g_) for g_ in gpu] for _ in range(2)]
    for g_, s_ in zip(gpu, statics[0]):
        g_.grad = s_
    opt.capture_safe(poke=True, slots=2)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        for j in range(2):
            for g_, s_ in zip(gpu, statics[j]):
                g_.grad = s_
            opt.step()
    torch.cuda.current_stream().wait_stream(s)
    plan = opt.captured_plan()
    assert plan['poke'] and plan['slots'] == 2
    for r in range(2):
        opt.activate(plan)
        for j in range(2):
            step = 2 * r + j
            _schedule(step, opt, opt_t)
            grads = make(190 + step, SHAPES, sgd_ref.MULT[step])
            for t_, s_, gr in zip(twin, statics[j], grads):
                t_.grad = gr.clone().to(dev())
                s_.copy_(gr)
            opt_t.step()
            opt.prepare_replay(slot=j)
        if r == 0:
            assert [float(x[1]) for x in plan['hyps'][0]] == [0.0, 0.0]
            assert [float(x[1]) for x in plan['hyps'][1]] == [np.float32(0.9), 0.5]
        lib.copy_batch([], opt.replay_blob())
        graph.replay()
        opt.mark_launched()
    torch.cuda.synchronize()
    _same_bits(gpu, opt, twin, opt_t)
    assert opt.grad_norms.shape == (2,) and float(opt.grad_norms[1]) == float(opt_t.last_grad_norm)
