"""CPU: the CatConvMish step-node primitive (reference models/search/darts/node_operations.py:58-82) — the test-side
restatement against the reference's own numbers (tests/golden/cat_conv_mish.npz, written by
tests/golden/make_golden_r10_mish.py), the module mirror, and the host logic that puts the primitive into the mix
kernels' FC slot (node_operations.node_mix_route, the parameter / gradient bookkeeping of NodeMixedOp).  No kernel
runs."""
import inspect
import json
import os

import numpy as np
import pytest
import torch

import cat_conv_mish_util as cm
from cat_conv_mish_util import MISH, list_id
from oracle import fusion_oracle as fo
from test_node_prims_host import Args, C, L, fake, on_fake_device, predicate, route  # noqa: F401  (predicate: fixture)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'cat_conv_mish.npz')


def make_op(prims):
    from models.search.darts.node_operations import NodeMixedOp
    with cm.mish_list(prims):
        return NodeMixedOp(C, L, Args())


# --------------------------------------------------------------------------- restatement against the reference
def test_restatement_equals_the_reference_fixture():
    """fo._conv_bn -> u tanh(softplus(u)) -> fo._dropout is the reference's arithmetic: the class alone (train, eval)
    and inside the reference's NodeMixedOp over ['Sum', 'CatConvMish', 'LinearGLU'], output, every gradient and the
    BatchNorm buffers (fp32 on both sides, the same torch: 1e-6 of each tensor's scale)."""
    z = np.load(GOLDEN)
    meta = json.loads(str(z['meta']))
    b, C_, L_ = meta['b'], meta['C'], meta['L']
    assert os.path.getsize(GOLDEN) < 100 * 1024

    def close(name, got, want):
        want = torch.from_numpy(np.asarray(want))
        scale = max(float(want.abs().max()), 1e-30)
        assert tuple(got.shape) == tuple(want.shape), name
        assert float((got - want).abs().max()) <= 1e-6 * scale, (name, float((got - want).abs().max()), scale)

    for tag, prims, seed, training in (('alone_train', [MISH], meta['alone_seed'], True),
                                       ('alone_eval', [MISH], meta['alone_seed'], False),
                                       ('mix_train', meta['mix'], meta['mix_seed'], True)):
        p, x, y, gamma, g = cm.make_case(prims, b, C_, L_, False, seed)
        if tag != 'mix_train':
            gamma = torch.ones(1)
        out, dw, dx, dy, po = cm.oracle_op(prims, p, x, y, gamma, g, False, training)
        close(tag + ' out', out, z[tag + ':out'])
        close(tag + ' dx', dx, z[tag + ':grad:x'])
        close(tag + ' dy', dy, z[tag + ':grad:y'])
        strip = (lambda k: k[len(cm.PREFIX) + 3:]) if tag != 'mix_train' else (lambda k: k)
        seen = 0
        for k, v in po.items():
            if fo.is_buffer(k):
                want = z[f'{tag}:buf:{strip(k)}']
                if k.endswith('num_batches_tracked'):
                    # (the restated op leaves the counter alone, like fo.node_mixed_op: fo.node_cell counts one level up)
                    assert int(want) == (1 if training else 0), k
                else:
                    close(tag + ' ' + k, v, want)
            elif k.endswith('conv.bias') and training:
                # in front of a train-mode BatchNorm: mathematically zero, round-off on both sides
                assert float(v.grad.abs().max()) < 1e-4 and float(np.abs(z[f'{tag}:grad:{strip(k)}']).max()) < 1e-4, k
            else:
                close(tag + ' d' + k, v.grad, z[f'{tag}:grad:{strip(k)}'])
            seen += 1
        assert seen == (7 if tag != 'mix_train' else 14)
        if tag == 'mix_train':
            close(tag + ' dgamma', dw, z[tag + ':grad:gamma'])


# ------------------------------------------------------------------------------------------------ the modules
def test_module_mirror():
    import models.search.darts.node_operations as no
    from models.search.darts.node_operations import CatConvMish, Mish
    assert list(inspect.signature(CatConvMish.__init__).parameters) == ['self', 'C', 'args']
    assert list(inspect.signature(CatConvMish.forward).parameters) == ['self', 'x', 'y']
    assert list(inspect.signature(Mish.forward).parameters) == ['self', 'x']
    m = CatConvMish(C, Args())
    assert [k for k, _ in m.named_children()] == ['conv', 'bn', 'dropout', 'mish']
    assert isinstance(m.mish, Mish) and m.dropout.p == Args.drpt and m._act == 'mish'
    assert list(m.state_dict()) == list(no.ConcatFC(C, Args()).state_dict())
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == \
        {k[len('op._ops.0.'):]: s for k, s in cm.op_param_shapes([MISH], C, L, 'op._ops').items()}
    assert hasattr(m, 'forward_thru')
    u = torch.linspace(-30, 30, 41)
    assert torch.equal(Mish()(u), u * torch.tanh(torch.nn.functional.softplus(u)))
    # not registered, as in the reference: four keys
    assert list(no.STEP_STEP_OPS) == ['Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC']
    with cm.registered():
        assert type(no.STEP_STEP_OPS[MISH](C, L, Args())) is CatConvMish
    assert MISH not in no.STEP_STEP_OPS
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        m(torch.zeros(2, C, L), torch.zeros(2, C, L))


# -------------------------------------------------------------------------------------------------- routes
@pytest.mark.parametrize('prims', cm.SUBSETS + cm.PERMUTATIONS, ids=list_id)
def test_fc_slot_lists_route_selected(prims, predicate):
    op = on_fake_device(make_op(prims))
    assert op._prims == prims and not op._default
    assert route(op) == 'selected'
    # the library predicate sees ConcatFC's bit
    assert predicate == [(sum(1 << cm.BUILTIN4.index(p) for p in prims), 4, C, L)]
    assert route(op, y=fake(4, C, L)) == 'selected'


def test_both_fc_slot_primitives_and_foreign_modules_compose(predicate, monkeypatch):
    import models.search.darts.node_operations as no
    assert route(on_fake_device(make_op(['ConcatFC', MISH]))) == 'composed'
    assert route(on_fake_device(make_op(['Sum', MISH, 'LinearGLU', 'ConcatFC']))) == 'composed'
    assert route(on_fake_device(make_op([MISH, MISH]))) == 'composed'
    assert predicate == []

    class Mine(no.CatConvMish):
        pass
    monkeypatch.setitem(no.STEP_STEP_OPS, MISH, lambda C_, L_, a: Mine(C_, a))
    with cm.edited_step_prims(['Sum', MISH]):
        op = on_fake_device(no.NodeMixedOp(C, L, Args()))
    assert route(op) == 'composed'
    monkeypatch.undo()
    op = on_fake_device(make_op(['Sum', MISH]))
    assert route(op) == 'selected'
    no.NODE_PRIMS_NATIVE = False
    try:
        assert route(op) == 'composed'
    finally:
        no.NODE_PRIMS_NATIVE = True
    op._ops[1].bn.momentum = 0.05                           # every existing condition still holds for the new module
    assert route(op) == 'composed'


def test_default_list_is_still_the_default():
    import models.search.darts.node_operations as no
    with cm.registered():
        op = no.NodeMixedOp(C, L, Args())
    assert op._default and route(op, torch.zeros(4, C, L)) == 'default'
    assert not make_op(cm.BUILTIN4)._default


# --------------------------------------------------------------------------- parameter / gradient bookkeeping
@pytest.mark.parametrize('prims', [[MISH, 'ScaleDotAttn', 'LinearGLU'], [MISH], ['LinearGLU', MISH, 'ScaleDotAttn', 'Sum']],
                         ids=list_id)
def test_param_and_grad_order_follow_named_parameters(prims):
    """As test_node_prims_host's: the gradient pack's regions carry distinct values per (kind, tensor) and every
    parameter must receive its own, in named_parameters() order — the FC-slot rows sit behind the LinearGLU rows
    whatever the list order."""
    from bmnas.cell import Arena
    op = make_op(prims)
    named = list(op.named_parameters())
    assert [k for k, _ in named] == [k[len('op.'):] for k in cm.op_param_shapes(prims, C, L, 'op._ops')
                                     if not fo.is_buffer(k)]
    assert list(op.state_dict()) == [k[len('op.'):] for k in cm.op_param_shapes(prims, C, L, 'op._ops')]
    plist = op.param_list()
    assert len(plist) == len(named) and all(a is b for a, (_, b) in zip(plist, named))
    M = op.conv_rows()
    fo_ = 2 * C if 'LinearGLU' in prims else 0
    assert M == fo_ + C
    arena = Arena()
    h = op.plan_grads(arena)
    arena.buf = torch.zeros(max(arena.total, 1))
    G = op.bind_grads(arena, h)
    assert tuple(G.stack_dW.shape) == (M, 2 * C) and G.stack_bn_grad.numel() == 2 * M
    for kind, lo, hi in (('LinearGLU', 0, 2 * C), (MISH, fo_, fo_ + C)):
        if kind in prims:
            t = 1.0 if kind == 'LinearGLU' else 2.0
            G.stack_dW[lo:hi] = t + 0.1
            G.stack_dbias[lo:hi] = t + 0.2
            G.stack_bn_grad[lo:hi] = t + 0.3
            G.stack_bn_grad[M + lo:M + hi] = t + 0.4
    if G.dln_w is not None:
        G.dln_w.fill_(3.1)
        G.dln_b.fill_(3.2)
    grads = op.grads_in_param_order(G)
    assert len(grads) == len(named)
    tail = {'conv.weight': 0.1, 'conv.bias': 0.2, 'bn.weight': 0.3, 'bn.bias': 0.4, 'ln.weight': 0.1, 'ln.bias': 0.2}
    for (name, p), g in zip(named, grads):
        base = {'LinearGLU': 1.0, MISH: 2.0, 'ScaleDotAttn': 3.0}[prims[int(name.split('.')[1])]]
        want = base + tail[name.split('.', 2)[2]]
        assert tuple(g.shape) == tuple(p.shape), name
        assert torch.all(g == torch.tensor(want)), (name, float(g.reshape(-1)[0]), want)


def test_pack_names_the_slot_and_carries_the_activation():
    from bmnas import lib
    prims = ['LinearGLU', MISH, 'Sum']
    op = make_op(prims)
    # (CPU tensors: the stacked storage is plain tensor bookkeeping)
    P = op.pack()
    assert P.prims == ['LinearGLU', 'ConcatFC', 'Sum'] and P.fc_act == lib.FC_ACT_MISH and P.M == 3 * C
    assert P.fc_p == Args.drpt and P.glu_p == Args.drpt
    st = op._stack
    assert st is not None and op._ops[0].conv.weight.data_ptr() == st.W.data_ptr()      # GLU rows first
    assert op._ops[1].conv.weight.data_ptr() == st.W[2 * C:].data_ptr()
    sel = lib.make_node_sel(P.prims)
    assert list(sel.col) == [2, -1, 0, 1] and lib.node_sel_mask(sel) == 0b1101
    with cm.edited_step_prims(['LinearGLU', 'ConcatFC', 'Sum']):
        from models.search.darts.node_operations import NodeMixedOp
        assert NodeMixedOp(C, L, Args()).pack().fc_act == lib.FC_ACT_RELU


def test_selection_descriptor_still_refuses_the_name():
    from bmnas import lib
    assert lib.NODE_KINDS == ('Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC')
    with pytest.raises(ValueError):
        lib.make_node_sel(['Sum', MISH])
