"""-m gpu: the Attention / MultiHeadAttn modules (reference models/search/darts/operations.py:67-86) on the gfx950
kernels — projection GEMMs (bmnas_conv1x1_*), the per-head core (csrc/mha.hip), bmnas.functions.MhaFn — against the
reference's own numbers (tests/golden/mha.npz), against the float64 statement of tests/mha_ref.py under the exported
dropout multipliers, and against the composed route (MHA_NATIVE = False) on the same module.  Tolerances are the
project's: 1e-4 forward, 2e-4 gradients of |want| + max|want|."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import mha_ref as mr
from fc_edges_util import device_kernels, recorded_sites
from gpu_util import Pool, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mha.npz')
FWD_REL, BWD_REL = 1e-4, 2e-4
META = json.loads(str(np.load(GOLDEN)['meta']))
SHAPES = [tuple(s) + (seed,) for s, seed in zip(META['shapes'], META['seeds'])]


class Args:
    def __init__(self, heads, drpt):
        self.num_heads, self.drpt = heads, drpt


@contextlib.contextmanager
def forced_composed():
    import models.search.darts.operations as ops
    ops.MHA_NATIVE = False
    try:
        yield
    finally:
        ops.MHA_NATIVE = True


def build(kind, C, L, heads, drpt, p, training):
    import models.search.darts.node_operations as no
    from models.search.darts.operations import Attention
    m = Attention(C, heads, drpt) if kind == 'Attention' else no.MultiHeadAttn(C, L, Args(heads, drpt))
    m.load_state_dict({'attn.' + k: v.clone() for k, v in p.items()})
    return m.to(dev()).train(training)


def run(m, kind, srcs, g):
    """forward + backward of module m over the device tensors `srcs` = (q, k, v), aliases among them allowed ->
    (out, the gradient of every distinct source in order of first use, parameter gradients by name)."""
    uniq = []
    for t in srcs:
        if all(t is not u for u in uniq):
            uniq.append(t)
    m.zero_grad()
    for u in uniq:
        u.grad = None
    out = m(srcs[0], srcs[1]) if kind == 'MultiHeadAttn' else m(*srcs)
    out.backward(g)
    torch.cuda.synchronize()
    return out.detach(), [u.grad for u in uniq], {k: v.grad for k, v in m.named_parameters()}


def leaf(t):
    return t.to(dev()).requires_grad_(True)


# ------------------------------------------------------------------ against the reference's own numbers
@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('kind,form', [('Attention', 'qkk'), ('Attention', 'qqq'), ('MultiHeadAttn', 'qkk')])
@pytest.mark.parametrize('b,C,L,heads,seed', SHAPES)
def test_modules_match_the_reference_fixture(b, C, L, heads, seed, kind, form, mode):
    import models.search.darts.operations as ops
    z = np.load(GOLDEN)
    p, t = mr.make_params(C, seed), mr.make_inputs(C, L, b, seed)
    m = build(kind, C, L, heads, 0.0, p, mode == 'train')
    q = leaf(t['q'])
    k = q if form == 'qqq' else leaf(t['k'])
    assert ops.attention_route(m, q, k, k) == 'native'
    out, dsrc, dpar = run(m, kind, (q, k, k), t['g'].to(dev()))
    assert dsrc[0] is not None
    tag = f'b{b}C{C}L{L}h{heads}:{form}:{mode}'
    assert_close_scaled(tag + ' out', out, z[tag + ':out'], rel=FWD_REL)
    assert_close_scaled(tag + ' dq', dsrc[0], z[tag + ':grad:q'], rel=BWD_REL)
    if form == 'qkk':
        assert_close_scaled(tag + ' dk', dsrc[1], z[tag + ':grad:k'], rel=BWD_REL)
    assert sorted(dpar) == sorted('attn.' + n for n in mr.PARAM_KEYS)
    for n, gr in dpar.items():
        assert_close_scaled(f'{tag} d{n}', gr, z[f'{tag}:grad:{n}'], rel=BWD_REL)


def test_forward_runs_as_mha_fn_and_launches_no_aten_kernel_in_between():
    """The native forward is an MhaFn node; between the first and the last launch of either direction no aten kernel
    runs (the zero fill of the atomically accumulated weight gradients comes before the backward's first launch)."""
    b, C, L, heads, seed = SHAPES[1]
    p, t = mr.make_params(C, seed), mr.make_inputs(C, L, b, seed)
    m = build('MultiHeadAttn', C, L, heads, 0.0, p, True)
    x, y, g = leaf(t['q']), leaf(t['k']), t['g'].to(dev())
    out = m(x, y)
    assert type(out.grad_fn).__name__ == 'MhaFnBackward'
    out.backward(g)                                            # (warm-up: allocator, pools)
    res = {}
    fwd = device_kernels(lambda: res.setdefault('out', m(x, y)))
    bwd = device_kernels(lambda: res['out'].backward(g))
    for name, names in (('forward', fwd), ('backward', bwd)):
        own = [i for i, n in enumerate(names) if 'at::native' not in n and 'Memset' not in n and 'Memcpy' not in n]
        assert own, names
        between = names[own[0]:own[-1] + 1]
        print(f'{name}: {len(names)} device events, {len(between)} from first to last launch')
        assert not [n for n in between if 'at::native' in n], between
    assert sum('mha_core_fwd_k' in n for n in fwd) == 1 and sum('mha_core_bwd_k' in n for n in bwd) == 1
    assert not [n for n in fwd if 'at::native' in n], fwd       # the forward holds no aten kernel at all


# ------------------------------------------------------------------ live dropout, under the exported multipliers
@pytest.mark.parametrize('form', ['qkk', 'qqq', 'qkv', 'qkq'])
@pytest.mark.parametrize('b,C,L,heads', [(5, 16, 8, 4), (3, 48, 16, 2), (7, 128, 8, 2)])
def test_live_dropout_matches_the_statement_under_the_exported_mask(b, C, L, heads, form):
    """Train mode with drpt = 0.25, every aliasing form of the projection plan (one, two and three GEMMs; q and v the
    same tensor with k another): the site recorded in K.DROP.record is exported and handed to the float64 statement."""
    from bmnas import lib
    seed = 1800 + b + C + L + heads
    p, t = mr.make_params(C, seed), mr.make_inputs(C, L, b, seed)
    m = build('Attention', C, L, heads, 0.25, p, True)
    q = leaf(t['q'])
    k = q if form == 'qqq' else leaf(t['k'])
    v = {'qkk': k, 'qqq': q, 'qkq': q}.get(form)
    if v is None:
        v = leaf(t['v'])
    with recorded_sites() as rec:
        out, dsrc, dpar = run(m, 'Attention', (q, k, v), t['g'].to(dev()))
    assert len(rec) == 1 and rec[0][1] == b * heads * L * L
    mask = lib.dropout_mask(rec[0][0], rec[0][1], dev()).cpu().view(b, heads, L, L)
    kept = float((mask > 0).float().mean())
    assert 0.63 < kept < 0.87 and abs(float(mask.max()) - 1.0 / 0.75) < 1e-6, kept
    cpu = {'q': t['q'], 'k': t['q'] if form == 'qqq' else t['k']}
    cpu['v'] = {'qkk': cpu['k'], 'qqq': cpu['q'], 'qkq': cpu['q'], 'qkv': t['v']}[form]
    ref = mr.mha_ref(cpu['q'], cpu['k'], cpu['v'], p, heads, t['g'], mask)
    want = {'qkk': [ref['dq'], ref['dk'] + ref['dv']], 'qqq': [ref['dq'] + ref['dk'] + ref['dv']],
            'qkv': [ref['dq'], ref['dk'], ref['dv']], 'qkq': [ref['dq'] + ref['dv'], ref['dk']]}[form]
    tag = f'b{b}C{C}L{L}h{heads} {form} drop'
    errs = {'out': mr.rel_err(out, ref['out'])}
    errs.update({f'dsrc{i}': mr.rel_err(a, w) for i, (a, w) in enumerate(zip(dsrc, want))})
    errs.update({n: mr.rel_err(dpar['attn.' + n], ref[n]) for n in mr.PARAM_KEYS})
    print(f'[{tag}] worst err / (|want| + max|want|): ' + ', '.join(f'{k_} {v_:.2e}' for k_, v_ in errs.items()))
    assert_close_scaled(tag + ' out', out, ref['out'], rel=FWD_REL)
    assert len(dsrc) == len(want)
    for i, (a, w) in enumerate(zip(dsrc, want)):
        assert_close_scaled(f'{tag} dsrc{i}', a, w, rel=BWD_REL)
    for n in mr.PARAM_KEYS:
        assert_close_scaled(f'{tag} d{n}', dpar['attn.' + n], ref[n], rel=BWD_REL)


# ------------------------------------------------------------------ native against composed, on the same module
@pytest.mark.parametrize('mode', ['train', 'eval'])
@pytest.mark.parametrize('form', ['qkk', 'qqq', 'qkv'])
@pytest.mark.parametrize('b,C,L,heads', [(6, 32, 8, 8), (5, 192, 16, 2), (7, 16, 4, 4)])
def test_native_equals_composed_on_the_same_module(b, C, L, heads, form, mode):
    import models.search.darts.operations as ops
    seed = 1900 + b + C + L + heads
    p, t = mr.make_params(C, seed), mr.make_inputs(C, L, b, seed)
    m = build('Attention', C, L, heads, 0.0, p, mode == 'train')
    q = leaf(t['q'])
    k = q if form == 'qqq' else leaf(t['k'])
    v = leaf(t['v']) if form == 'qkv' else k
    g = t['g'].to(dev())
    a = run(m, 'Attention', (q, k, v), g)
    a = (a[0], [x.clone() for x in a[1]], {n: x.clone() for n, x in a[2].items()})
    with forced_composed():
        assert ops.attention_route(m, q, k, v) == 'composed'
        c = run(m, 'Attention', (q, k, v), g)
    tag = f'b{b}C{C}L{L}h{heads} {form} {mode}'
    assert_close_scaled(tag + ' out', a[0], c[0], rel=FWD_REL)
    assert len(a[1]) == len(c[1]) == {'qkk': 2, 'qqq': 1, 'qkv': 3}[form]
    for i, (x, w) in enumerate(zip(a[1], c[1])):
        assert_close_scaled(f'{tag} dsrc{i}', x, w, rel=BWD_REL)
    for n, w in c[2].items():
        assert_close_scaled(f'{tag} d{n}', a[2][n], w, rel=BWD_REL)


def test_inputs_that_need_no_gradient_and_no_grad_mode():
    b, C, L, heads, seed = SHAPES[0]
    p, t = mr.make_params(C, seed), mr.make_inputs(C, L, b, seed)
    m = build('Attention', C, L, heads, 0.0, p, True)
    q, k = t['q'].to(dev()), leaf(t['k'])
    out, dsrc, dpar = run(m, 'Attention', (q, k, k), t['g'].to(dev()))
    ref = mr.mha_ref(t['q'], t['k'], t['k'], p, heads, t['g'])
    assert dsrc[0] is None
    assert_close_scaled('dk', dsrc[1], ref['dk'] + ref['dv'], rel=BWD_REL)
    assert_close_scaled('dW', dpar['attn.in_proj_weight'], ref['in_proj_weight'], rel=BWD_REL)
    with torch.no_grad():
        assert_close_scaled('out', m(q, k, k), ref['out'], rel=FWD_REL)


# ------------------------------------------------------------------ the core is bit-stable
@pytest.mark.parametrize('C,heads,L,b', [(192, 2, 16, 5), (16, 4, 4, 7)])
def test_two_backward_passes_of_the_core_are_bit_equal(C, heads, L, b):
    """dq / dk / dv through the kernel entry points (the weight gradients behind them are summed with atomics and are
    not compared): live dropout, two forward + backward passes into fresh NaN buffers."""
    from bmnas import lib
    t = {k: v.to(dev()) for k, v in mr.make_core_inputs(C, heads, L, b).items()}
    drop = lib.make_dropout(mr.DROP_P, mr.DROP_SEED, mr.DROP_OFFSET)
    U = torch.cat([t['Q'], t['K'], t['V']], 1)
    q, k, v = U[:, :C], U[:, C:2 * C], U[:, 2 * C:]
    runs = []
    for _ in range(2):
        pool = Pool()
        O, P, dU = pool.new(b, C, L), pool.new(b, heads, L, L), pool.new(b, 3 * C, L)
        lib.mha_core_fwd(q, k, v, O, P, b, C, L, heads, drop)
        lib.mha_core_bwd(t['dO'], q, k, v, P, dU[:, :C], dU[:, C:2 * C], dU[:, 2 * C:], b, C, L, heads, drop)
        pool.check()
        runs.append((O.clone(), P.clone(), dU.clone()))
    for x, y in zip(*runs):
        assert bool(torch.isfinite(x).all()) and torch.equal(x.view(torch.int32), y.view(torch.int32))
