"""-m gpu: AMSGrad and decoupled weight decay in the one-launch Adam step (csrc/adam.hip: adam_multi_ex_k;
bmnas_adam_multi_ex; bmnas.optim.Adam(amsgrad=..., decoupled_weight_decay=...), bmnas.optim.AdamW) against torch.optim.Adam /
torch.optim.AdamW on the CPU in float64 and against tests/adam_ref.py.

Layout: tests/test_optim_gpu.py's — SHAPES, two groups (the second with lr 3e-3), parameter 2 joining at step 2, lr *= 0.9
per step, 6 steps.  betas = (0.9, 0.9) and step s's randn gradients times MULT[s]: with beta2 = 0.999 and plain randn
gradients exp_avg_sq only grows over 6 steps, max_exp_avg_sq equals it and AMSGrad could not be told from plain Adam.

Tolerance: the project's optimizer tolerance, 2e-6 of the tensor's scale (test_optim_gpu.py; _assert_matches of
test_grad_clip_gpu.py) — torch's own fp32 CPU run of these inputs is 2.5e-7 of scale from float64.  Every comparison case
first shows, on the float64 references alone, that the variant differs from plain Adam by >= 100 x that tolerance."""
import copy
import math

import numpy as np
import pytest
import torch

import adam_ref
from gpu_util import dev

pytestmark = pytest.mark.gpu

SHAPES = [(384, 384, 1), (384,), (7,), (1,), (13, 2), (3, 5, 11), (4099,), (192, 16)]     # test_optim_gpu.py's
MULT = [10, 10, 1, 0.1, 0.1, 1]
BETAS = (0.9, 0.9)
TOL = 2e-6
UNALIGNED = [1, 3, 1023, 1024, 1025, 4099]


def _make(seed, shapes, mult=1.0):
    g = torch.Generator().manual_seed(seed)
    return [mult * torch.randn(*s, generator=g) for s in shapes]


def _groups(ps):
    return [{'params': ps[:3]}, {'params': ps[3:], 'lr': 3e-3}]


def _torch_ref(cpu, amsgrad, decoupled, wd, groups=_groups):
    return torch.optim.Adam(groups(cpu), lr=1e-2, betas=BETAS, weight_decay=wd, amsgrad=amsgrad,
                            decoupled_weight_decay=decoupled)


def _set_grads(step, cpu, gpu, seed=100, shapes=SHAPES, late=True):
    for i, gr in enumerate(_make(seed + step, shapes, MULT[step % len(MULT)])):
        none = late and i == 2 and step < 2
        if cpu is not None:
            cpu[i].grad = None if none else gr.double()
        if gpu is not None:
            gpu[i].grad = None if none else gr.clone().to(dev())


def _decay_lr(*opts):
    for grps in zip(*[o.param_groups for o in opts]):
        lr = grps[0]['lr'] * 0.9
        for g in grps:
            g['lr'] = lr


def _cpu_run(amsgrad, decoupled, wd, max_norm, seed=1, steps=6):
    """torch on the CPU in float64 alone -> (parameters, optimizer)"""
    cpu = [t.double().requires_grad_(True) for t in _make(seed, SHAPES)]
    ref = _torch_ref(cpu, amsgrad, decoupled, wd)
    for step in range(steps):
        _set_grads(step, cpu, None)
        _decay_lr(ref)
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(cpu, max_norm)
        ref.step()
    return cpu, ref


_CPU = {}


def _cpu_cached(*key):
    """One float64 run per configuration, shared and left unchanged."""
    if key not in _CPU:
        _CPU[key] = _cpu_run(*key)
    return _CPU[key]


def _distance(a, b):
    """worst |a - b| / scale over the parameters of two float64 runs"""
    return max(float((x.detach() - y.detach()).abs().max()) / (float(y.detach().abs().max()) + 1e-3) for x, y in zip(a, b))


def _assert_matches(cpu, gpu, ref, opt, names=('exp_avg', 'exp_avg_sq'), label=''):
    worst = 0.0
    for c, g_ in zip(cpu, gpu):
        scale = float(c.detach().abs().max()) + 1e-3
        err = float((g_.detach().cpu().double() - c.detach().double()).abs().max())
        worst = max(worst, err / scale)
        assert err <= TOL * scale + 1e-7, (err, scale)
    sd_ref, sd = ref.state_dict(), opt.state_dict()
    assert set(sd_ref['state']) == set(sd['state'])
    for k in sd_ref['state']:
        assert float(sd['state'][k]['step']) == float(sd_ref['state'][k]['step'])
        assert set(sd['state'][k]) == set(sd_ref['state'][k]), (set(sd['state'][k]), set(sd_ref['state'][k]))
        for name in names:
            a, b = sd['state'][k][name].cpu().double(), sd_ref['state'][k][name].double()
            err, scale = float((a - b).abs().max()), float(b.abs().max())
            worst = max(worst, err / max(scale, 1e-30))
            assert err <= TOL * scale + 1e-12, (name, k, err, scale)
    print(f'{label} worst error / scale over parameters and {names}: {worst:.3e}')


def _bits(t):
    return t.detach().view(torch.int32)


def _gpu_run(amsgrad, decoupled, wd, max_norm, seed=1, steps=6, after=None, cls=None):
    """bmnas.optim.Adam on the GPU over the same inputs as _cpu_run -> (parameters, optimizer)"""
    from bmnas.optim import Adam
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in _make(seed, SHAPES)]
    if cls is not None:
        opt = cls(_groups(gpu), lr=1e-2, betas=BETAS, weight_decay=wd, amsgrad=amsgrad, max_grad_norm=max_norm)
    else:
        opt = Adam(_groups(gpu), lr=1e-2, betas=BETAS, weight_decay=wd, amsgrad=amsgrad, max_grad_norm=max_norm,
                   decoupled_weight_decay=decoupled)
    for step in range(steps):
        _set_grads(step, None, gpu)
        _decay_lr(opt)
        before = {p: opt.state[p]['max_exp_avg_sq'].clone() for p in gpu if 'max_exp_avg_sq' in opt.state.get(p, {})}
        opt.step()
        if after is not None:
            after(step, gpu, opt, before)
    torch.cuda.synchronize()
    return gpu, opt


CASES = [('amsgrad', True, False, 1e-4, None), ('decoupled_wd0.1', False, True, 0.1, None),
         ('both_wd0.1', True, True, 0.1, None), ('both_wd1e-4', True, True, 1e-4, None),
         ('both_clipped', True, True, 0.1, 5.0)]


@pytest.mark.parametrize('amsgrad,decoupled,wd,max_norm', [c[1:] for c in CASES], ids=[c[0] for c in CASES])
def test_variant_matches_torch(amsgrad, decoupled, wd, max_norm):
    from bmnas.optim import AdamW
    cpu, ref = _cpu_cached(amsgrad, decoupled, wd, max_norm)
    plain, _ = _cpu_cached(False, False, wd, max_norm)
    apart = _distance(cpu, plain)
    print(f'float64: variant against plain Adam {apart:.3e} of scale')
    assert apart >= 100 * TOL                                          # the comparison below cannot pass vacuously

    def running_max(step, gpu, opt, before):
        # AMSGrad's invariant, bit for bit after every step: max = torch.maximum(max before, exp_avg_sq after)
        for p in gpu:
            st = opt.state.get(p, {})
            if 'max_exp_avg_sq' in st:
                was = before.get(p, torch.zeros_like(st['exp_avg_sq']))
                assert torch.equal(_bits(st['max_exp_avg_sq']), _bits(torch.maximum(was, st['exp_avg_sq']))), step

    gpu, opt = _gpu_run(amsgrad, decoupled, wd, max_norm, after=running_max if amsgrad else None)
    names = ('exp_avg', 'exp_avg_sq') + (('max_exp_avg_sq',) if amsgrad else ())
    _assert_matches(cpu, gpu, ref, opt, names)
    if amsgrad and max_norm is None:
        above = sum(int((opt.state[p]['max_exp_avg_sq'] > opt.state[p]['exp_avg_sq']).sum()) for p in gpu)
        total = sum(p.numel() for p in gpu)
        print(f'max_exp_avg_sq > exp_avg_sq on {above} of {total} elements')
        assert above >= total / 2
    if decoupled and amsgrad and wd == 0.1:
        # bmnas.optim.AdamW is the same optimizer
        gpu_w, opt_w = _gpu_run(amsgrad, None, wd, max_norm, cls=AdamW)
        for a, b in zip(gpu, gpu_w):
            assert torch.equal(_bits(a), _bits(b))
        assert opt_w.state_dict()['param_groups'] == opt.state_dict()['param_groups']


def test_a_nan_gradient_element_stays_nan_in_moment_maximum_and_parameter():
    """No clipping: the NaN stays in its element.  The running maximum must take it (torch.maximum; fmaxf would keep the
    finite operand and the parameter would recover)."""
    from bmnas.optim import Adam
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in _make(3, SHAPES)]
    opt = Adam(_groups(gpu), lr=1e-2, betas=BETAS, weight_decay=1e-4, amsgrad=True)
    where = (4, (7, 1))
    for step in range(3):
        _set_grads(step, None, gpu, late=False)
        if step == 1:
            gpu[where[0]].grad[where[1]] = float('nan')
        opt.step()
        if step == 0:
            continue
        torch.cuda.synchronize()
        for i, p in enumerate(gpu):
            st = opt.state[p]
            for name, t in (('param', p.detach()), ('exp_avg_sq', st['exp_avg_sq']),
                            ('max_exp_avg_sq', st['max_exp_avg_sq'])):
                bad = torch.isnan(t)
                if i == where[0]:
                    assert bool(bad[where[1]]), (step, name)
                    assert int(bad.sum()) == 1, (step, name)
                else:
                    assert not bool(bad.any()), (step, name, i)
                assert not bool(torch.isinf(t).any())


def test_decoupled_decay_of_zero_leaves_the_bits_of_plain_adam():
    """f = 1 - lr * 0 = 1 and p * 1.0f == p: six steps of the decoupled kernel give the bits of adam_multi_k."""
    a, opt_a = _gpu_run(False, True, 0.0, None, seed=2)
    b, opt_b = _gpu_run(False, False, 0.0, None, seed=2)
    assert opt_a._plan['flags'] == 2 and opt_b._plan['flags'] == 0
    for pa, pb in zip(a, b):
        assert torch.equal(_bits(pa), _bits(pb))
        for name in ('exp_avg', 'exp_avg_sq'):
            assert torch.equal(_bits(opt_a.state[pa][name]), _bits(opt_b.state[pb][name])), name
    assert not torch.equal(a[0].detach().cpu(), _make(2, SHAPES)[0])


def test_amsgrad_on_constant_gradients_keeps_the_maximum_equal_to_the_moment():
    """The same gradient tensors at every step, no weight decay: v' = fl(v * beta2 + w2 * g * g) is a monotone map of v
    and v_1 >= v_0 = 0, so v never falls, in fp32 as in exact arithmetic — the maximum bit-equals it after every step and
    the update is plain Adam's."""
    from bmnas.optim import Adam
    init = _make(6, SHAPES)
    grads = [g.to(dev()) for g in _make(7, SHAPES)]
    a = [t.clone().to(dev()).requires_grad_(True) for t in init]
    b = [t.clone().to(dev()).requires_grad_(True) for t in init]
    ams = Adam(_groups(a), lr=1e-2, betas=BETAS, amsgrad=True)
    plain = Adam(_groups(b), lr=1e-2, betas=BETAS)
    for step in range(6):
        for i, (pa, pb, gr) in enumerate(zip(a, b, grads)):
            pa.grad, pb.grad = (None, None) if i == 2 and step < 2 else (gr, gr)
        ams.step()
        plain.step()
        for pa in a:
            if pa.grad is not None:
                assert torch.equal(_bits(ams.state[pa]['max_exp_avg_sq']), _bits(ams.state[pa]['exp_avg_sq'])), step
    torch.cuda.synchronize()
    for pa, pb in zip(a, b):
        scale = float(pb.detach().abs().max()) + 1e-3
        assert float((pa.detach() - pb.detach()).abs().max()) <= TOL * scale + 1e-7


# ---------------------------------------------------------------------------------------------- the C ABI, driven directly
def _hyp(t, lr, wd, decoupled, betas=BETAS, eps=1e-8):
    b1, b2 = betas
    slot5 = (1 - lr * wd if wd != 0 else 1.0) if decoupled else wd
    return torch.tensor([[-(lr / (1 - b1 ** t)), math.sqrt(1 - b2 ** t), b1, b2, eps, slot5, 1 - b1, 1 - b2]],
                        dtype=torch.float32, device=dev())


def _guarded(host, offset):
    """host tensor -> (view at `offset` floats into a NaN-filled store with two spare floats, the store)"""
    store = torch.full((host.numel() + 2,), float('nan'), device=dev())
    view = store[offset:offset + host.numel()]
    view.copy_(host.reshape(-1))
    assert view.data_ptr() % 16 == 4 * offset
    return view, store


class _Direct:
    """Device tensors + bmnas_adam_tensor_t[] + chunk list for a direct call, one scalar row for all tensors."""

    def __init__(self, sizes, seed, max_offset=0):
        from bmnas import lib
        from bmnas.optim import _DESC
        shapes = [(n,) for n in sizes]
        self.host = {k: _make(seed + j, shapes) for j, k in enumerate(('p', 'g', 'm'))}
        self.host['m'] = [0.1 * t for t in self.host['m']]
        self.host['v'] = [0.01 * t.abs() for t in _make(seed + 3, shapes)]
        self.host['x'] = [0.02 * t.abs() for t in _make(seed + 4, shapes)]      # above v on about half the elements
        self.dev = {k: [t.clone().to(dev()) for t in v] for k, v in self.host.items() if k != 'x'}
        pairs = [_guarded(t, max_offset) for t in self.host['x']]
        self.dev['x'], self.stores = [v for v, _ in pairs], [s for _, s in pairs]
        E = lib.adam_chunk_elems()
        tab = np.zeros(len(sizes), dtype=_DESC)
        for field, k in (('param', 'p'), ('grad', 'g'), ('exp_avg', 'm'), ('exp_avg_sq', 'v')):
            tab[field] = [t.data_ptr() for t in self.dev[k]]
        tab['numel'] = sizes
        chunks = [(i, c) for i, n in enumerate(sizes) for c in range((n + E - 1) // E)]
        self.tab = torch.from_numpy(tab.view(np.uint8)).to(dev())
        self.chunks = torch.tensor(chunks, dtype=torch.int32).reshape(-1, 2).to(dev())
        self.n = len(chunks)
        self.maxes = torch.tensor([t.data_ptr() for t in self.dev['x']], dtype=torch.int64, device=dev())
        self.partials = torch.empty(lib.grad_norm_parts(), device=dev())
        self.n_parts = min(self.n, lib.grad_norm_parts())
        self.clip = torch.tensor([5.0], device=dev())
        self.norm = torch.zeros(1, device=dev())

    def snapshot(self):
        torch.cuda.synchronize()
        return {k: [t.clone() for t in v] for k, v in self.dev.items()}


@pytest.mark.parametrize('clipped', [False, True], ids=['unclipped', 'clipped'])
def test_flags_zero_runs_the_existing_kernels_bit_for_bit(clipped):
    from bmnas import lib
    hyp = _hyp(3, 1e-2, 1e-4, False)
    a, b = _Direct(UNALIGNED + [300001], 20), _Direct(UNALIGNED + [300001], 20)
    if clipped:
        lib.grad_sqnorm_multi(a.tab, a.chunks, a.n, a.partials)
        lib.adam_multi_clip(a.tab, a.chunks, a.n, hyp, a.partials, a.n_parts, a.clip, a.norm)
        lib.grad_sqnorm_multi(b.tab, b.chunks, b.n, b.partials)
        lib.adam_multi_ex(b.tab, b.chunks, b.n, hyp, None, 0, b.partials, b.n_parts, b.clip, b.norm)
    else:
        lib.adam_multi(a.tab, a.chunks, a.n, hyp)
        lib.adam_multi_ex(b.tab, b.chunks, b.n, hyp, None, 0)
    sa, sb = a.snapshot(), b.snapshot()
    for k in ('p', 'm', 'v', 'x'):
        for x, y in zip(sa[k], sb[k]):
            assert torch.equal(_bits(x), _bits(y)), k
    assert not torch.equal(sa['p'][-1].cpu(), a.host['p'][-1])
    if clipped:
        assert float(a.norm) == float(b.norm) > 5.0


@pytest.mark.parametrize('max_offset', [0, 1], ids=['aligned', 'max_exp_avg_sq_offset1'])
@pytest.mark.parametrize('clipped', [False, True], ids=['unclipped', 'clipped'])
def test_direct_call_against_float64(max_offset, clipped):
    """bmnas_adam_multi_ex with both switches on a hand-built table.  offset 1: ONLY the max_exp_avg_sq buffers are 4
    bytes off the 16-byte alignment — their pointers are part of the test that selects the float4 branch — with NaN on
    both sides of each."""
    from bmnas import lib
    import clip_ref
    t, lr, wd = 3, 1e-2, 0.1
    d = _Direct(UNALIGNED, 30, max_offset)
    grads = d.host['g']
    if clipped:
        lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
        lib.adam_multi_ex(d.tab, d.chunks, d.n, _hyp(t, lr, wd, True), d.maxes, lib.ADAM_AMSGRAD | lib.ADAM_DECOUPLED,
                          d.partials, d.n_parts, d.clip, d.norm)
        grads, norm = clip_ref.clip(grads, 5.0)
    else:
        lib.adam_multi_ex(d.tab, d.chunks, d.n, _hyp(t, lr, wd, True), d.maxes, lib.ADAM_AMSGRAD | lib.ADAM_DECOUPLED)
    got = d.snapshot()
    if clipped:
        assert norm > 5.0 and abs(float(d.norm) - norm) <= 2e-5 * norm
    raised = 0
    for i in range(len(UNALIGNED)):
        want = adam_ref.adam_step(d.host['p'][i], grads[i], d.host['m'][i], d.host['v'][i], d.host['x'][i], t, lr, BETAS,
                                  1e-8, wd, amsgrad=True, decoupled=True)
        for k, w in zip(('p', 'm', 'v', 'x'), want):
            err = np.abs(got[k][i].cpu().double().numpy() - w).max()
            assert err <= TOL * np.abs(w).max() + 1e-12, (k, i, err)
        raised += int((got['x'][i].cpu() > d.host['x'][i]).sum())
        assert bool(torch.isnan(d.stores[i][[0, -1]] if max_offset else d.stores[i][-2:]).all())
        assert torch.equal(got['g'][i].cpu(), d.host['g'][i])           # `.grad` is not written
    assert 0 < raised < sum(UNALIGNED)                                   # the maximum moved on some elements only


def test_unaligned_parameters_take_the_scalar_path():
    """test_adam_unaligned_parameters_take_the_scalar_path's arrangement with AMSGrad + decoupled decay."""
    from bmnas.optim import AdamW
    shapes = [(n,) for n in UNALIGNED]
    init = _make(5, shapes)
    cpu = [t.double().requires_grad_(True) for t in init]
    gpu, stores = [], []
    for t in init:
        store = torch.full((t.numel() + 2,), float('nan'), device=dev())
        store[1:-1].copy_(t)
        p = store[1:-1].detach().requires_grad_()
        assert p.is_leaf and p.storage_offset() == 1 and p.data_ptr() % 16 == 4
        gpu.append(p)
        stores.append(store)
    ref = torch.optim.AdamW(cpu, lr=1e-2, betas=BETAS, weight_decay=0.1, amsgrad=True)
    opt = AdamW(gpu, lr=1e-2, betas=BETAS, weight_decay=0.1, amsgrad=True)
    for step in range(6):
        _set_grads(step, cpu, gpu, seed=300, shapes=shapes, late=False)
        ref.step()
        opt.step()
    torch.cuda.synchronize()
    _assert_matches(cpu, gpu, ref, opt, ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'))
    for store in stores:
        assert bool(torch.isnan(store[[0, -1]]).all())                  # the floats around the view: untouched


def test_rejected_arguments_launch_nothing():
    from bmnas import lib
    d = _Direct([1025, 7], 40)
    hyp = _hyp(1, 1e-2, 0.1, True)
    lib.grad_sqnorm_multi(d.tab, d.chunks, d.n, d.partials)
    before = d.snapshot()
    A, D = lib.ADAM_AMSGRAD, lib.ADAM_DECOUPLED
    clip = (d.partials, d.n_parts, d.clip, d.norm)
    bad = [
        (d.maxes, 4), (d.maxes, A | 8), (None, -1),                                     # unknown flag bits
        (None, A), (None, A | D),                                                      # AMSGRAD without the table
        (d.maxes, 0), (d.maxes, D),                                                    # the table without the flag
        (d.maxes, A | D, d.partials, d.n_parts, None, None),                           # partials / clip / norm_out: not
        (d.maxes, A | D, d.partials, d.n_parts, d.clip, None),                         # all set ...
        (d.maxes, A | D, None, 0, d.clip, d.norm), (d.maxes, A | D, None, 0, None, d.norm),
        (None, 0, d.partials, d.n_parts, d.clip, None),                                # ... with flags == 0 as well
        (d.maxes, A | D, d.partials, d.n_parts + 1, d.clip, d.norm),                   # not what the norm launch wrote
        (d.maxes, A, d.partials, 0, d.clip, d.norm), (None, D, d.partials, 256, d.clip, d.norm),
    ]
    for args in bad:
        with pytest.raises(lib.BmnasError, match='bad argument'):
            lib.adam_multi_ex(d.tab, d.chunks, d.n, hyp, *args)
    after = d.snapshot()
    for k in before:
        for x, y in zip(before[k], after[k]):
            assert torch.equal(_bits(x), _bits(y)), k
    assert float(d.norm) == 0.0
    lib.adam_multi_ex(d.tab, d.chunks, d.n, hyp, d.maxes, A | D, *clip)                 # the accepted form does launch
    assert not torch.equal(_bits(d.snapshot()['p'][0]), _bits(before['p'][0]))


# ------------------------------------------------------------------------------------------------------------ checkpoints
def _continue_from_torch(torch_cls, our_cls, kw):
    shapes = SHAPES[:4]
    cpu = [t.double().requires_grad_(True) for t in _make(2, shapes)]
    ref = torch_cls(cpu, lr=1e-2, betas=BETAS, **kw)
    for step in range(3):
        _set_grads(step, cpu, None, seed=50, shapes=shapes, late=False)
        ref.step()
    gpu = [c.detach().float().to(dev()).requires_grad_(True) for c in cpu]
    opt = our_cls(gpu, lr=1e-2, betas=BETAS)                           # switches and weight decay: the checkpoint's
    opt.load_state_dict(copy.deepcopy(ref.state_dict()))               # (torch casts the moments to the parameters' fp32)
    for step in range(3, 6):
        _set_grads(step, cpu, gpu, seed=50, shapes=shapes, late=False)
        ref.step()
        opt.step()
    torch.cuda.synchronize()
    return cpu, gpu, ref, opt


def test_a_torch_amsgrad_checkpoint_continues():
    from bmnas.optim import Adam
    cpu, gpu, ref, opt = _continue_from_torch(torch.optim.Adam, Adam, dict(weight_decay=1e-4, amsgrad=True))
    assert all(g['amsgrad'] is True for g in opt.param_groups) and opt._plan['flags'] == 1
    _assert_matches(cpu, gpu, ref, opt, ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'))
    assert float(opt.state_dict()['state'][0]['step']) == 6.0


def test_a_torch_adamw_checkpoint_continues():
    from bmnas.optim import AdamW
    cpu, gpu, ref, opt = _continue_from_torch(torch.optim.AdamW, AdamW, dict(weight_decay=0.1))
    assert all(g['decoupled_weight_decay'] is True and g['weight_decay'] == 0.1 for g in opt.param_groups)
    assert opt._plan['flags'] == 2
    _assert_matches(cpu, gpu, ref, opt)
    l2 = _cpu_cached(False, False, 0.1, None)[0], _cpu_cached(False, True, 0.1, None)[0]
    assert _distance(*l2) >= 100 * TOL


def test_our_checkpoint_loads_into_torch():
    from bmnas.optim import AdamW
    gpu, opt = _gpu_run(True, None, 0.1, None, cls=AdamW)
    cpu = [p.detach().cpu().double().requires_grad_(True) for p in gpu]
    ref = torch.optim.AdamW(_groups(cpu), lr=1e-2, betas=BETAS, weight_decay=0.1, amsgrad=True)
    ref.load_state_dict(copy.deepcopy(opt.state_dict()))
    assert ref.param_groups[1]['lr'] == opt.param_groups[1]['lr'] != ref.param_groups[0]['lr']
    assert ref.state[cpu[0]]['max_exp_avg_sq'].dtype == torch.float64
    _set_grads(5, cpu, gpu, seed=900)
    ref.step()
    opt.step()
    torch.cuda.synchronize()
    _assert_matches(cpu, gpu, ref, opt, ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq'))


def test_a_checkpoint_without_the_maximum_continues_with_amsgrad_from_zeros():
    from bmnas.optim import Adam
    gpu, opt = _gpu_run(False, False, 1e-4, None, steps=3)
    sd = copy.deepcopy(opt.state_dict())
    assert 'max_exp_avg_sq' not in sd['state'][0]
    gpu2 = [p.detach().clone().requires_grad_(True) for p in gpu]
    opt2 = Adam(_groups(gpu2), lr=1e-2, betas=BETAS, weight_decay=1e-4)
    opt2.load_state_dict(sd)
    for g in opt2.param_groups:
        g['amsgrad'] = True
    _set_grads(3, None, gpu2)
    opt2.step()
    torch.cuda.synchronize()
    assert opt2._plan['flags'] == 1
    for p in gpu2:
        st = opt2.state[p]
        assert torch.equal(_bits(st['max_exp_avg_sq']), _bits(st['exp_avg_sq']))    # maximum(0, v) == v
        assert float(st['exp_avg_sq'].max()) > 0
    # the step itself is then plain Adam's
    _set_grads(3, None, gpu)
    opt.step()
    torch.cuda.synchronize()
    for a, b in zip(gpu, gpu2):
        assert float((a.detach() - b.detach()).abs().max()) <= TOL * (float(a.detach().abs().max()) + 1e-3) + 1e-7


# --------------------------------------------------------------------------------------------------------------- captured
@pytest.mark.parametrize('poke', [False, True], ids=['copy_node', 'poke'])
def test_captured_variant_step_replays_and_follows_a_restored_state(poke):
    """test_adam_in_graph_replays_with_new_rates / test_eager_step_between_replays_does_not_poison_the_graph with
    AMSGrad + decoupled decay + max_grad_norm: a new lr per replay, eager steps on fresh gradient tensors in between, a
    state restored after the capture (the replay must follow the NEW max_exp_avg_sq tensors), and the refusal of a
    switch flipped under the captured plan."""
    from bmnas import lib
    from bmnas.optim import AdamW
    init = _make(4, SHAPES)
    cpu = [t.double().requires_grad_(True) for t in init]
    gpu = [t.clone().to(dev()).requires_grad_(True) for t in init]
    ref = torch.optim.AdamW(cpu, lr=1e-2, betas=BETAS, weight_decay=0.1, amsgrad=True)
    opt = AdamW(gpu, lr=1e-2, betas=BETAS, weight_decay=0.1, amsgrad=True, max_grad_norm=5.0)
    static = [torch.zeros_like(g_) for g_ in gpu]
    for g_, s_ in zip(gpu, static):
        g_.grad = s_
    opt.capture_safe(poke=poke)
    graph = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.cuda.graph(graph, stream=s):
        opt.step()
    torch.cuda.current_stream().wait_stream(s)
    plan = opt.captured_plan()
    assert plan['poke'] == poke and plan['flags'] == 3 and plan['key'] == (True, True, True)

    def one(step, eager=False):
        lr = 1e-2 * (0.8 ** step)
        for grp in list(ref.param_groups) + list(opt.param_groups):
            grp['lr'] = lr
        grads = _make(90 + step, SHAPES, MULT[step % len(MULT)])
        for c, gr in zip(cpu, grads):
            c.grad = gr.double()
        torch.nn.utils.clip_grad_norm_(cpu, 5.0)
        ref.step()
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

    for step in range(6):
        one(step, eager=step in (2, 4))
    torch.cuda.synchronize()
    names = ('exp_avg', 'exp_avg_sq', 'max_exp_avg_sq')
    _assert_matches(cpu, gpu, ref, opt, names, label='six steps')
    # a checkpoint restored after the capture
    old = [opt.state[p]['max_exp_avg_sq'] for p in gpu]
    opt.load_state_dict(copy.deepcopy(opt.state_dict()))
    new = [opt.state[p]['max_exp_avg_sq'] for p in gpu]
    assert all(a.data_ptr() != b.data_ptr() for a, b in zip(old, new))
    old_bits = [_bits(t).clone() for t in old]
    new_bits = [_bits(t).clone() for t in new]
    one(6)
    torch.cuda.synchronize()
    _assert_matches(cpu, gpu, ref, opt, names, label='after the restored state')
    assert all(torch.equal(_bits(t), b) for t, b in zip(old, old_bits))            # the old tensors: no longer written
    assert any(not torch.equal(_bits(t), b) for t, b in zip(new, new_bits))
    assert float(opt.state_dict()['state'][0]['step']) == 7.0
    # one launch is one instantiation: a switch flipped under the captured plan is refused
    for name in ('amsgrad', 'decoupled_weight_decay'):
        opt.activate(plan)
        opt.param_groups[0][name] = False
        with pytest.raises(lib.BmnasError, match='re-capture'):
            opt.prepare_replay()
        opt.param_groups[0][name] = True
