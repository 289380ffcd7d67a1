"""CPU: the host logic behind an edited STEP_STEP_PRIMITIVES list — which path NodeMixedOp.forward takes
(node_operations.node_mix_route) and the per-kind parameter / gradient bookkeeping of NodeMixedOp.  No kernel runs."""
import pytest
import torch

from oracle import fusion_oracle as fo
from node_prims_util import KINDS, PERMUTATIONS, SUBSETS, edited_step_prims, list_id, op_param_shapes

C, L = 16, 8


class Args:
    C, L, drpt = C, L, 0.1


def make_op(prims):
    from models.search.darts.node_operations import NodeMixedOp
    with edited_step_prims(prims):
        return NodeMixedOp(C, L, Args())


class FakeCuda(torch.Tensor):
    """A CPU tensor that reports is_cuda: the route only looks at tensor metadata."""
    @property
    def is_cuda(self):
        return True


def fake(*shape):
    return torch.zeros(*shape).as_subclass(FakeCuda)


def on_fake_device(op):
    for name, p in list(op.named_parameters()):
        mod = op.get_submodule(name.rsplit('.', 1)[0])
        mod._parameters[name.rsplit('.', 1)[1]] = torch.nn.Parameter(p.data).as_subclass(FakeCuda)
    return op


@pytest.fixture
def predicate(monkeypatch):
    """The library predicate, stubbed: records its arguments, answers True."""
    from bmnas import lib
    calls = []
    monkeypatch.setattr(lib, 'node_mix_sel_ok', lambda mask, b, c, l: (calls.append((mask, b, c, l)), True)[1])
    return calls


def route(op, x=None, y=None, w=None):
    from models.search.darts.node_operations import node_mix_route
    x = fake(4, C, L) if x is None else x
    return node_mix_route(op, x, x if y is None else y, fake(len(op._prims)) if w is None else w)


def test_default_list_routes_default(predicate):
    import models.search.darts.node_operations as no
    op = make_op(KINDS)
    assert route(op, torch.zeros(4, C, L)) == 'default'        # today's path, whatever it is given
    no.NODE_PRIMS_NATIVE = False
    try:
        assert route(op) == 'default'
    finally:
        no.NODE_PRIMS_NATIVE = True
    assert predicate == []


@pytest.mark.parametrize('prims', [s for s in SUBSETS if s != KINDS] + PERMUTATIONS + [KINDS[::-1]], ids=list_id)
def test_subsets_and_permutations_route_selected(prims, predicate):
    op = on_fake_device(make_op(prims))
    assert op._prims == prims and not op._default
    assert route(op) == 'selected'
    assert predicate == [(sum(1 << KINDS.index(p) for p in prims), 4, C, L)]
    y = fake(4, C, L)
    assert route(op, y=y) == 'selected'


def test_everything_else_routes_composed(predicate, monkeypatch):
    import models.search.darts.node_operations as no
    prims = ['ConcatFC', 'Sum', 'ScaleDotAttn']
    assert route(on_fake_device(make_op(prims))) == 'selected'
    # a repeated name
    assert route(on_fake_device(make_op(['Sum', 'ConcatFC', 'Sum']))) == 'composed'
    # an unknown name (a primitive the user registered)
    monkeypatch.setitem(no.STEP_STEP_OPS, 'Mine', lambda C_, L_, a: no.Sum())
    assert route(on_fake_device(make_op(['Sum', 'Mine']))) == 'composed'
    # a subclassed op behind a built-in name (an edited registry)

    class MySum(no.Sum):
        pass
    monkeypatch.setitem(no.STEP_STEP_OPS, 'Sum', lambda C_, L_, a: MySum())
    assert route(on_fake_device(make_op(['Sum', 'ConcatFC']))) == 'composed'
    monkeypatch.undo()
    from bmnas import lib
    monkeypatch.setattr(lib, 'node_mix_sel_ok', lambda *a: True)
    op = on_fake_device(make_op(prims))
    assert route(op) == 'selected'
    # a CPU tensor, other dtypes / ranks / shapes
    assert route(op, torch.zeros(4, C, L)) == 'composed'
    assert route(op, y=torch.zeros(4, C, L)) == 'composed'
    assert route(op, fake(4, C, L).double().as_subclass(FakeCuda)) == 'composed'
    assert route(op, fake(4, C * L)) == 'composed'
    assert route(op, y=fake(5, C, L)) == 'composed'
    assert route(op, fake(4, 2 * C, L)) == 'composed'           # not the (C, L) the op was built for
    # the weight row
    assert route(op, w=fake(4)) == 'composed'
    assert route(op, w=fake(1, 3)) == 'composed'
    # mixed train / eval submodules
    op._ops[0].bn.eval()
    assert route(op) == 'composed'
    op.train()
    assert route(op) == 'selected'
    op.eval()
    assert route(op) == 'selected'
    # BatchNorm away from its defaults
    op._ops[0].bn.momentum = 0.05
    assert route(op) == 'composed'
    op._ops[0].bn.momentum = 0.1
    op._ops[0].bn.eps = 1e-3
    assert route(op) == 'composed'
    op._ops[0].bn.eps = 1e-5
    assert route(op) == 'selected'
    # the switch
    no.NODE_PRIMS_NATIVE = False
    try:
        assert route(op) == 'composed'
    finally:
        no.NODE_PRIMS_NATIVE = True
    # the library's own limits
    monkeypatch.setattr(lib, 'node_mix_sel_ok', lambda *a: False)
    assert route(op) == 'composed'


def test_composed_forward_is_the_reference_sum_on_cpu():
    """Off the selected route the forward is still `sum(w * op(x, y))`: with a stand-in primitive list that needs no
    kernel it runs on the CPU and equals the weighted sum."""
    import models.search.darts.node_operations as no

    class Twice(torch.nn.Module):
        def forward(self, x, y):
            return 2 * x + y

    class Diff(torch.nn.Module):
        def forward(self, x, y):
            return x - y
    no.STEP_STEP_OPS['Twice'] = lambda C_, L_, a: Twice()
    no.STEP_STEP_OPS['Diff'] = lambda C_, L_, a: Diff()
    try:
        op = make_op(['Twice', 'Diff'])
        x, y, w = torch.randn(3, C, L), torch.randn(3, C, L), torch.tensor([0.25, 0.75])
        assert no.node_mix_route(op, x, y, w) == 'composed'
        assert torch.equal(op(x, y, w), 0.25 * (2 * x + y) + 0.75 * (x - y))
    finally:
        del no.STEP_STEP_OPS['Twice'], no.STEP_STEP_OPS['Diff']


@pytest.mark.parametrize('prims', SUBSETS + [PERMUTATIONS[1], KINDS[::-1]], ids=list_id)
def test_param_and_grad_order_follow_named_parameters(prims):
    """param_list() is named_parameters() order, and grads_in_param_order() hands every parameter the slice of the
    gradient pack that belongs to it: the pack's regions are filled with distinct values per (kind, tensor) and each
    parameter must receive its own, in its own shape — for all 15 subsets and two permutations."""
    from bmnas.cell import Arena
    op = make_op(prims)
    named = list(op.named_parameters())
    assert [k for k, _ in named] == [k[len('op.'):] for k in op_param_shapes(prims, C, L, 'op._ops')
                                     if not fo.is_buffer(k)]
    plist = op.param_list()
    assert len(plist) == len(named) and all(a is b for a, (_, b) in zip(plist, named))
    M = op.conv_rows()
    assert M == (2 * C if 'LinearGLU' in prims else 0) + (C if 'ConcatFC' in prims else 0)
    arena = Arena()
    h = op.plan_grads(arena)
    arena.buf = torch.zeros(max(arena.total, 1))
    G = op.bind_grads(arena, h)
    assert (G.stack_dW is None) == (M == 0) and (G.dln_w is None) == ('ScaleDotAttn' not in prims)
    # tag: rows of LinearGLU 1.x, rows of ConcatFC 2.x; x = 1 dW, 2 dbias, 3 dBN.weight, 4 dBN.bias; LayerNorm 3.1 / 3.2
    fo_ = 2 * C if 'LinearGLU' in prims else 0
    if M:
        assert tuple(G.stack_dW.shape) == (M, 2 * C) and G.stack_bn_grad.numel() == 2 * M
        for kind, lo, hi in (('LinearGLU', 0, 2 * C), ('ConcatFC', fo_, fo_ + C)):
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
        kind = prims[int(name.split('.')[1])]
        base = {'LinearGLU': 1.0, 'ConcatFC': 2.0, 'ScaleDotAttn': 3.0}[kind]
        want = base + tail[name.split('.', 2)[2]]
        assert tuple(g.shape) == tuple(p.shape), name
        assert torch.all(g == torch.tensor(want)), (name, float(g.reshape(-1)[0]), want)


def test_state_dict_keys_follow_list_position():
    prims = ['ConcatFC', 'ScaleDotAttn', 'Sum', 'LinearGLU']
    op = make_op(prims)
    assert list(op.state_dict()) == [k[len('op.'):] for k in op_param_shapes(prims, C, L, 'op._ops')]


def test_selection_descriptor():
    from bmnas import lib
    sel = lib.make_node_sel(['ConcatFC', 'Sum'])
    assert list(sel.col) == [1, -1, -1, 0] and sel.n == 2 and lib.node_sel_mask(sel) == 0b1001
    for bad in ([], ['Sum', 'Sum'], ['Sum', 'CatConvMish']):
        with pytest.raises(ValueError):
            lib.make_node_sel(bad)
