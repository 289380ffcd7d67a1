"""CPU: the Attention / MultiHeadAttn module mirrors (reference models/search/darts/operations.py:67-86) and the host
logic in front of the attention-core kernels: state_dict keys and shapes, the attention_route decisions, the
lib.mha_ok table, the projection-GEMM plan of bmnas.functions.MhaFn.  No kernel runs."""
import inspect
import json
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

import mha_ref as mr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mha.npz')
C, L, B, HEADS = 16, 8, 4, 4
KEYS = ['attn.in_proj_weight', 'attn.in_proj_bias', 'attn.out_proj.weight', 'attn.out_proj.bias']


class Args:
    drpt = 0.2


def test_module_mirror_and_state_dict():
    import models.search.darts.node_operations as no
    from models.search.darts.operations import Attention
    assert list(inspect.signature(Attention.__init__).parameters) == ['self', 'embed_dim', 'num_heads', 'drpt']
    assert list(inspect.signature(Attention.forward).parameters) == ['self', 'q', 'k', 'v']
    m = Attention(C, HEADS, 0.3)
    assert type(m.attn) is nn.MultiheadAttention and m.attn.dropout == 0.3 and m.attn.num_heads == HEADS
    assert [k for k, _ in m.named_children()] == ['attn']
    assert list(m.state_dict()) == KEYS
    # ... which are the reference class's keys and shapes (the fixture holds its gradients under its parameter names)
    z = np.load(GOLDEN)
    b_, C_, L_, h_ = json.loads(str(z['meta']))['shapes'][0]
    tag = f'b{b_}C{C_}L{L_}h{h_}:qkk:train:grad:'
    ref_shapes = {k[len(tag):]: z[k].shape for k in z.files if k.startswith(tag + 'attn.')}
    assert ref_shapes == {k: tuple(v.shape) for k, v in Attention(C_, h_, 0.0).state_dict().items()}
    # both directions with a bare nn.MultiheadAttention
    bare = nn.MultiheadAttention(C, HEADS, 0.3)
    m.load_state_dict({'attn.' + k: v for k, v in bare.state_dict().items()})
    assert all(torch.equal(m.state_dict()['attn.' + k], v) for k, v in bare.state_dict().items())
    other = nn.MultiheadAttention(C, HEADS, 0.3)
    other.load_state_dict({k[len('attn.'):]: v for k, v in m.state_dict().items()})
    assert all(torch.equal(other.state_dict()[k], v) for k, v in bare.state_dict().items())

    assert list(inspect.signature(no.MultiHeadAttn.__init__).parameters) == ['self', 'C', 'L', 'args']
    assert list(inspect.signature(no.MultiHeadAttn.forward).parameters) == ['self', 'x', 'y']
    n = no.MultiHeadAttn(C, L, Args())
    assert isinstance(n, Attention) and list(n.state_dict()) == KEYS
    assert n.attn.num_heads == 2 and n.attn.dropout == Args.drpt and n.attn.embed_dim == C

    class WithHeads(Args):
        num_heads = 8
    assert no.MultiHeadAttn(C, L, WithHeads()).attn.num_heads == 8
    # not registered, as in the reference
    assert list(no.STEP_STEP_OPS) == ['Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC']
    assert not hasattr(n, 'forward_thru')


def test_cpu_tensors_raise():
    import models.search.darts.node_operations as no
    from models.search.darts.operations import Attention, attention_route
    x = torch.zeros(B, C, L)
    m = Attention(C, HEADS, 0.0)
    assert attention_route(m, x, x, x) == 'native'
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(x, x, x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        no.MultiHeadAttn(C, L, Args())(x, torch.ones(B, C, L))


def test_route_decisions(monkeypatch):
    import models.search.darts.node_operations as no
    import models.search.darts.operations as ops
    from bmnas import lib
    route = ops.attention_route
    x, y = torch.zeros(B, C, L), torch.ones(B, C, L)
    m = ops.Attention(C, HEADS, 0.1)
    assert route(m, x, y, y) == 'native' and route(m, x, x, x) == 'native' and route(m, x, y, x.clone()) == 'native'
    assert route(no.MultiHeadAttn(C, L, Args()), x, y, y) == 'native'
    # the switch
    monkeypatch.setattr(ops, 'MHA_NATIVE', False)
    assert route(m, x, y, y) == 'composed'
    monkeypatch.setattr(ops, 'MHA_NATIVE', True)
    # a shape that mha_ok refuses: asked of the library, and believed
    asked = []
    monkeypatch.setattr(lib, 'mha_ok', lambda *a: asked.append(a) or False)
    assert route(m, x, y, y) == 'composed' and asked == [(B, C, L, HEADS)]
    monkeypatch.undo()
    assert route(ops.Attention(C, 8, 0.0), x, y, y) == 'composed'                         # d = 2
    assert route(ops.Attention(1024, 2, 0.0), *[torch.zeros(2, 1024, L)] * 3) == 'composed'
    assert route(ops.Attention(C, HEADS, 0.0), *[torch.zeros(B, C, 32)] * 3) == 'composed'
    # non-fp32 or mismatched inputs
    assert route(m, x.double(), y.double(), y.double()) == 'composed'
    assert route(m, x, y.half(), y.half()) == 'composed'
    assert route(m, x, torch.zeros(B, C, 2 * L), torch.zeros(B, C, 2 * L)) == 'composed'
    assert route(m, x[0], y[0], y[0]) == 'composed'
    assert route(m, torch.zeros(B, 2 * C, L), torch.zeros(B, 2 * C, L), torch.zeros(B, 2 * C, L)) == 'composed'
    assert route(m, x, y, y.to('meta')) == 'composed'
    assert route(ops.Attention(C, HEADS, 0.1).double(), x, y, y) == 'composed'
    # an edited self.attn
    for kw in (dict(kdim=2 * C), dict(vdim=2 * C), dict(bias=False), dict(add_bias_kv=True), dict(add_zero_attn=True),
               dict(batch_first=True)):
        e = ops.Attention(C, HEADS, 0.1)
        e.attn = nn.MultiheadAttention(C, HEADS, 0.1, **kw)
        assert route(e, x, y, y) == 'composed', kw

    class MineAttn(nn.MultiheadAttention):
        pass
    e = ops.Attention(C, HEADS, 0.1)
    e.attn = MineAttn(C, HEADS, 0.1)
    assert route(e, x, y, y) == 'composed'

    # a subclass
    class Mine(ops.Attention):
        pass

    class MineToo(no.MultiHeadAttn):
        pass
    assert route(Mine(C, HEADS, 0.1), x, y, y) == 'composed'
    assert route(MineToo(C, L, Args()), x, y, y) == 'composed'


def test_composed_route_is_the_reference_composition():
    """MHA_NATIVE = False on the CPU: the module's own transposes around self.attn against the float64 statement."""
    import models.search.darts.operations as ops
    seed = 77
    p, t = mr.make_params(C, seed), mr.make_inputs(C, L, B, seed)
    m = ops.Attention(C, HEADS, 0.0)
    m.load_state_dict({'attn.' + k: v for k, v in p.items()})
    ops.MHA_NATIVE = False
    try:
        out = m(t['q'], t['k'], t['k'])
    finally:
        ops.MHA_NATIVE = True
    assert mr.rel_err(out, mr.mha_ref(t['q'], t['k'], t['k'], p, HEADS)['out']) < 2.5e-5


def test_mha_ok_table():
    from bmnas import lib
    for C_, heads, L_, b in mr.KERNEL_TABLE:
        assert lib.mha_ok(b, C_, L_, heads), (C_, heads, L_, b)
    for L_ in (4, 8, 16):
        for C_ in range(16, 513, 16):
            for heads in (1, 2, 4, 8):
                ok = C_ % heads == 0 and (C_ // heads) % 4 == 0
                assert lib.mha_ok(3, C_, L_, heads) == ok, (C_, L_, heads)
    assert lib.mha_ok(128, 192, 16, 2) and lib.mha_ok(64, 128, 8, 2) and lib.mha_ok(1, 16, 4, 4)
    for b, C_, L_, heads in ((0, 16, 8, 2), (2, 528, 8, 2), (2, 8, 8, 2), (2, 24, 8, 2), (2, 32, 2, 2), (2, 32, 12, 2),
                             (2, 32, 32, 2), (2, 32, 8, 0), (2, 32, 8, 3), (2, 32, 8, 16), (2, 48, 8, 5)):
        assert not lib.mha_ok(b, C_, L_, heads), (b, C_, L_, heads)


def test_projection_gemm_plan():
    from bmnas.functions import mha_runs
    assert mha_runs((0, 0, 0)) == [(0, 3, 0)]                      # q is k is v: one GEMM with M = 3C
    assert mha_runs((0, 1, 1)) == [(0, 1, 0), (1, 3, 1)]           # k is v: M = C and M = 2C
    assert mha_runs((0, 1, 2)) == [(0, 1, 0), (1, 2, 1), (2, 3, 2)]
    assert mha_runs((0, 1, 0)) == [(0, 1, 0), (1, 2, 1), (2, 3, 0)]   # q and v the same tensor, k another: three
    assert mha_runs((0, 0, 1)) == [(0, 2, 0), (2, 3, 1)]
