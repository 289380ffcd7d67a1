"""CPU: tests/mha_ref.py — the float64 statement of the multi-head attention primitive that the GPU tests compare
against — pinned to torch.nn.MultiheadAttention in float64 (every shape of the kernel table, the output and all seven
gradients) and to the reference's own Attention class (tests/golden/mha.npz, written by
tests/golden/make_golden_r17_mha.py).  It also asserts that torch's fp32 result stays within a quarter of the two GPU
tolerances (1e-4 forward, 2e-4 gradients of |want| + max|want|) on these inputs: the GPU bounds are not hiding a
reference problem.  No kernel runs."""
import json
import os

import numpy as np
import pytest
import torch

import mha_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mha.npz')
FWD_REL, BWD_REL = 1e-4, 2e-4
GRADS = ('dq', 'dk', 'dv') + mr.PARAM_KEYS


def torch_mha(p, t, heads, dtype, p_drop=0.0, training=True):
    """nn.MultiheadAttention under the reference's transposes (operations.py:72-86) -> (out, the seven gradients)."""
    C = p['out_proj.weight'].shape[0]
    attn = torch.nn.MultiheadAttention(C, heads, p_drop).to(dtype)
    attn.load_state_dict({k: v.to(dtype) for k, v in p.items()})
    attn.train(training)
    q, k, v = (t[n].to(dtype).clone().requires_grad_(True) for n in ('q', 'k', 'v'))
    out = attn(*(x.transpose(0, 1).transpose(0, 2) for x in (q, k, v)), need_weights=False)[0]
    out = out.transpose(0, 2).transpose(0, 1)
    out.backward(t['g'].to(dtype))
    grads = {'dq': q.grad, 'dk': k.grad, 'dv': v.grad}
    grads.update({n: w.grad for n, w in attn.named_parameters()})
    return out.detach(), grads


@pytest.mark.parametrize('C,heads,L,b', mr.KERNEL_TABLE)
def test_statement_equals_torch_multihead_attention(C, heads, L, b):
    seed = mr.case_seed(C, heads, L, b)
    p, t = mr.make_params(C, seed), mr.make_inputs(C, L, b, seed)
    ref = mr.mha_ref(t['q'], t['k'], t['v'], p, heads, t['g'])
    out64, g64 = torch_mha(p, t, heads, torch.float64)
    assert mr.rel_err(ref['out'], out64) < 1e-12
    for n in GRADS:
        assert mr.rel_err(ref[n], g64[n]) < 1e-12, n
    # the softmax is not saturated: no row's largest probability is within 1e-3 of one
    assert float(ref['P'].max()) < 1.0 - 1e-3
    out32, g32 = torch_mha(p, t, heads, torch.float32)
    worst = {'out': mr.rel_err(out32, ref['out'])}
    worst.update({n: mr.rel_err(g32[n], ref[n]) for n in GRADS})
    print(f'C={C} h={heads} L={L} b={b}: torch fp32 vs float64 statement: ' +
          ', '.join(f'{k} {v:.1e}' for k, v in worst.items()))
    assert worst['out'] <= FWD_REL / 4
    for n in GRADS:
        assert worst[n] <= BWD_REL / 4, (n, worst[n])


@pytest.mark.parametrize('C,heads,L,b', [(16, 4, 4, 7), (48, 2, 16, 5)])
def test_core_and_whole_statement_agree_and_the_mask_multiplies_the_probabilities(C, heads, L, b):
    """core_ref with an explicit mask against autograd through the same formula (the kernels' tests hand it the exported
    dropout multipliers, which torch's own dropout cannot reproduce)."""
    t = mr.make_core_inputs(C, heads, L, b)
    g = mr.gen(5)
    mask = torch.from_numpy((g.random((b, heads, L, L)) >= mr.DROP_P).astype(np.float64) / (1.0 - mr.DROP_P))
    ref = mr.core_ref(t['Q'], t['K'], t['V'], heads, t['dO'], mask)
    Q, K, V = (t[n].double().clone().requires_grad_(True) for n in ('Q', 'K', 'V'))
    d = C // heads
    S = torch.einsum('bhci,bhcj->bhij', Q.view(b, heads, d, L), K.view(b, heads, d, L)) / d ** 0.5
    O = torch.einsum('bhij,bhcj->bhci', torch.softmax(S, -1) * mask, V.view(b, heads, d, L)).reshape(b, C, L)
    O.backward(t['dO'].double())
    assert mr.rel_err(ref['O'], O.detach()) < 1e-12
    for n, w in (('dQ', Q), ('dK', K), ('dV', V)):
        assert mr.rel_err(ref[n], w.grad) < 1e-12, n
    assert float(ref['P'].max()) < 1.0 - 1e-3


def test_statement_equals_the_reference_fixture():
    """The reference's Attention, both aliasing forms, train (drpt = 0) and eval: fp32 there, float64 here — within a
    quarter of the GPU tolerances, like torch's fp32 above."""
    z = np.load(GOLDEN)
    meta = json.loads(str(z['meta']))
    assert os.path.getsize(GOLDEN) < 1024 * 1024
    for (b, C, L, heads), seed in zip(meta['shapes'], meta['seeds']):
        p, t = mr.make_params(C, seed), mr.make_inputs(C, L, b, seed)
        for form in ('qkk', 'qqq'):
            q = t['q']
            k = q if form == 'qqq' else t['k']
            ref = mr.mha_ref(q, k, k, p, heads, t['g'])
            want = {'out': ref['out'], 'grad:q': ref['dq'] + (ref['dk'] + ref['dv'] if form == 'qqq' else 0.0)}
            if form == 'qkk':
                want['grad:k'] = ref['dk'] + ref['dv']
            want.update({'grad:attn.' + n: ref[n] for n in mr.PARAM_KEYS})
            for mode in ('train', 'eval'):
                tag = f'b{b}C{C}L{L}h{heads}:{form}:{mode}'
                for n, w in want.items():
                    bound = (FWD_REL if n == 'out' else BWD_REL) / 4
                    assert mr.rel_err(torch.from_numpy(z[f'{tag}:{n}']), w) <= bound, (tag, n)
                assert sum(key.startswith(tag + ':') for key in z.files) == len(want)
