"""-m gpu: the MultiHeadAttn step-node primitive (the two-input form of the reference's Attention,
models/search/darts/operations.py:67-86) inside NodeMixedOp and whole networks.

The primitive is registered the way a user registers it (STEP_STEP_OPS['MultiHeadAttn'] = ...).  In an edited
STEP_STEP_PRIMITIVES list NodeMixedOp keeps its composed sum with this term on its own kernels inside it: checked
against the reference's NodeMixedOp over ['Sum', 'MultiHeadAttn', 'LinearGLU'] (tests/golden/mha.npz), and as a search
hypernet step against the same network with the attention forced onto the composed route.  A found network whose
genotype names the primitive: an eager step, the captured step (bmnas.graph.GraphedTrainStep) against its eager twin,
and live attention dropout across replays.  Tolerances are the project's: 1e-4 of scale forward, 2e-4 gradients."""
import contextlib
import json
import os

import numpy as np
import pytest
import torch

import mha_ref as mr
import node_prims_util as npu
from gpu_util import Args, assert_close_scaled, dev, set_mode
from oracle import fusion_oracle as fo
from oracle import synth

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'mha.npz')
MHA = 'MultiHeadAttn'
SEED = 41


@contextlib.contextmanager
def registered():
    """STEP_STEP_OPS['MultiHeadAttn'] for the duration, the one line a user adds."""
    import models.search.darts.node_operations as no
    assert MHA not in no.STEP_STEP_OPS
    no.STEP_STEP_OPS[MHA] = lambda C, L, args: no.MultiHeadAttn(C, L, args)
    try:
        yield
    finally:
        del no.STEP_STEP_OPS[MHA]


@contextlib.contextmanager
def forced_composed():
    import models.search.darts.operations as ops
    ops.MHA_NATIVE = False
    try:
        yield
    finally:
        ops.MHA_NATIVE = True


def attention_modules(net):
    import models.search.darts.node_operations as no
    return [m for m in net.modules() if type(m) is no.MultiHeadAttn]


def load_synthetic(net, shapes, cfg, seed):
    """synth parameters for every key of `shapes`, mha_ref.make_params for the attention modules (the only other
    keys)."""
    sd = synth.make_params(cfg, seed, shapes)
    rest = [k for k in net.state_dict() if k not in sd]
    assert rest and all('.attn.' in k for k in rest), rest
    for i, pre in enumerate(sorted({k[:k.index('.attn.') + len('.attn.')] for k in rest})):
        sd.update({pre + k: v for k, v in mr.make_params(cfg.C, seed + 100 + i).items()})
    assert set(sd) == set(net.state_dict())
    net.load_state_dict(sd)


def native_launches(fn):
    """fn() -> (its result, how many attention-core forward launches it issued)."""
    from bmnas import lib
    calls = []
    plain = lib.mha_core_fwd

    def counted(*a, **k):
        calls.append(1)
        return plain(*a, **k)
    lib.mha_core_fwd = counted
    try:
        return fn(), len(calls)
    finally:
        lib.mha_core_fwd = plain


# ------------------------------------------------------------------ one NodeMixedOp, against the reference's
def test_node_mixed_op_matches_the_reference_fixture():
    import models.search.darts.node_operations as no
    z = np.load(GOLDEN)
    meta = json.loads(str(z['meta']))
    prims, b, C, L = meta['mix'], meta['mix_b'], meta['mix_C'], meta['mix_L']
    cfg = fo.make_cfg(N=2, C=C, L=L, S=1, M=1, ns=1, nm=1, drpt=0.1)
    with registered(), npu.edited_step_prims(prims):
        op = no.NodeMixedOp(C, L, Args(cfg, 1e-12))
    assert type(op._ops[1]) is no.MultiHeadAttn and op._ops[1].attn.num_heads == meta['mix_heads']
    p, x, y, gamma, g = npu.make_case(prims, b, C, L, False, seed=meta['mix_seed'])
    sd = {k[len('op.'):]: v.clone() for k, v in p.items()}
    sd.update({f'_ops.1.attn.{k}': v.clone() for k, v in mr.make_params(C, meta['mix_seed']).items()})
    assert set(sd) == set(op.state_dict())
    op.load_state_dict(sd)
    op.to(dev()).train()
    xd, yd = x.to(dev()).requires_grad_(True), y.to(dev()).requires_grad_(True)
    wd = gamma.to(dev()).requires_grad_(True)
    assert no.node_mix_route(op, xd, yd, wd) == 'composed'
    out, n = native_launches(lambda: op(xd, yd, wd))
    assert n == 1                                               # ... with the attention term on its own kernels
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    assert_close_scaled('out', out, z['mix_train:out'], rel=1e-4)
    assert_close_scaled('dx', xd.grad, z['mix_train:grad:x'], rel=2e-4)
    assert_close_scaled('dy', yd.grad, z['mix_train:grad:y'], rel=2e-4)
    assert_close_scaled('dgamma', wd.grad, z['mix_train:grad:gamma'], rel=2e-4)
    seen = 0
    for k, v in op.named_parameters():
        want = z[f'mix_train:grad:op.{k}']
        if k.endswith('conv.bias'):
            assert float(v.grad.abs().max()) < 1e-4 and float(np.abs(want).max()) < 1e-4, k
        else:
            assert_close_scaled('d' + k, v.grad, want, rel=2e-4)
        seen += '.attn.' in k
    assert seen == 4
    for k, v in op.state_dict().items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == int(z[f'mix_train:buf:op.{k}']) == 1
        elif fo.is_buffer(k):
            assert_close_scaled('buf:' + k, v.float(), z[f'mix_train:buf:op.{k}'])


# ------------------------------------------------------------------ the search hypernet
def test_search_step_native_attention_equals_composed_attention(monkeypatch):
    """One step (forward + backward) of the hypernet at N3 C16 L8 with STEP_STEP_PRIMITIVES = ['Sum', 'MultiHeadAttn',
    'LinearGLU'], on the same weights: the attention terms native against composed.  Weight, architecture and input
    gradients."""
    from models.search.darts.model_search import FusionNetwork
    prims = ['Sum', MHA, 'LinearGLU']
    monkeypatch.setattr(fo, 'STEP_STEP_PRIMITIVES', list(prims))          # (arch shapes of synth.make_arch)
    cfg = fo.make_cfg(N=3, C=16, L=8, S=2, M=2, ns=2, nm=2, drpt=0.0)
    batch, nout = 5, 7
    with registered(), npu.edited_step_prims(prims):
        net = FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), criterion=None)
    load_synthetic(net, npu.net_param_shapes(cfg, prims), cfg, SEED)
    for dst, src in zip(net.arch_parameters(), synth.make_arch(cfg, SEED, 0.5)):
        assert dst.shape == src.shape
        dst.data.copy_(src)
    net.to(dev())
    set_mode(net, 'train')
    assert len(attention_modules(net)) == cfg.S * cfg.ns
    cls = torch.nn.Linear(cfg.M * cfg.C * cfg.L, nout)
    cw, cb = synth.make_classifier(cfg, nout, SEED)
    cls.weight.data.copy_(cw)
    cls.bias.data.copy_(cb)
    cls.to(dev())
    labels = synth.make_labels('ce', batch, nout, SEED).to(dev())

    def step():
        xs = [x.to(dev()).requires_grad_(True) for x in synth.make_inputs(cfg, batch, SEED)]
        for q in list(net.parameters()) + list(net.arch_parameters()) + list(cls.parameters()):
            q.grad = None
        with npu.edited_step_prims(prims):
            logits = cls(net(xs))
        loss = torch.nn.functional.cross_entropy(logits, labels)
        loss.backward()
        torch.cuda.synchronize()
        grads = {'w:' + k: v.grad.clone() for k, v in net.named_parameters()}
        grads.update({f'arch:{i}': a.grad.clone() for i, a in enumerate(net.arch_parameters())})
        grads.update({f'input:{i}': x.grad.clone() for i, x in enumerate(xs)})
        return logits.detach().clone(), loss.detach().clone(), grads

    (la, sa, ga), n = native_launches(step)
    assert n == cfg.S * cfg.ns
    with forced_composed():
        (lb, sb, gb), n = native_launches(step)
    assert n == 0
    assert_close_scaled('logits', la, lb, rel=1e-4)
    assert_close_scaled('loss', sa, sb, rel=1e-4)
    assert set(ga) == set(gb) and any('.attn.' in k for k in ga) and 'arch:2' in ga
    for k, v in ga.items():
        if k.endswith('conv.bias'):
            assert float(v.abs().max()) < 1e-4 and float(gb[k].abs().max()) < 1e-4, k
        else:
            assert_close_scaled('grad ' + k, v, gb[k], rel=2e-4)


# ------------------------------------------------------------------ found networks
def _skip(*idx):
    return [('skip', i) for i in idx]


FOUND = {
    'two_steps': (fo.make_cfg(N=2, C=32, L=16, S=2, M=2, ns=2, nm=2, drpt=0.0), 5,
                  [_skip(0, 1, 1, 2), _skip(1, 0, 0, 2)], [MHA, 'LinearGLU'], [2, 3]),
    'one_step': (fo.make_cfg(N=2, C=16, L=8, S=2, M=2, ns=1, nm=1, drpt=0.0), 4,
                 [_skip(0, 1), _skip(1, 0)], [MHA], [2]),
}


def build_found(key, seed, drpt=None, linear=None, nout=8):
    """-> (model: fusion net + classifier, cfg, batch).  The genotype names the primitive; Found_NodeCell.compile looks
    it up in STEP_STEP_OPS (node.py:52), where it is registered while the network is constructed."""
    from models.search.darts.genotypes import Genotype, StepGenotype
    from models.search.darts.model import Found_FusionNetwork
    cfg, batch, inner_edges, inner_steps, inner_concat = FOUND[key]
    if drpt is not None:
        cfg = fo.make_cfg(N=cfg.N, C=cfg.C, L=cfg.L, S=cfg.S, M=cfg.M, ns=cfg.ns, nm=cfg.nm, drpt=drpt)
    steps = lambda names: [StepGenotype(inner_edges=[tuple(e) for e in ed], inner_steps=list(names),
                                        inner_concat=list(inner_concat)) for ed in inner_edges]
    gg = Genotype(edges=[tuple(e) for e in _skip(0, 1, 1, 0)], steps=steps(inner_steps), concat=[2, 3])
    with registered():
        net = Found_FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), None, gg)
    # the other parameters' shapes: the genotype with the parameter-free Sum where the attention is
    plain = fo.Genotype(edges=_skip(0, 1, 1, 0), concat=[2, 3],
                        steps=[fo.StepGenotype(e, ['Sum' if n == MHA else n for n in inner_steps], list(inner_concat))
                               for e in inner_edges])
    load_synthetic(net, fo.found_param_shapes(cfg, plain), cfg, seed)
    assert len(attention_modules(net)) == cfg.S
    cls = (linear or torch.nn.Linear)(cfg.M * cfg.C * cfg.L, nout)
    cw, cb = synth.make_classifier(cfg, nout, seed)
    cls.weight.data.copy_(cw)
    cls.bias.data.copy_(cb)
    return _FoundStep(net, cls).to(dev()), cfg, batch


class _FoundStep(torch.nn.Module):
    """fusion_net -> central_classifier, wired like the reference's Found_*_Net minus backbones and reshape layers."""
    def __init__(self, net, cls):
        super().__init__()
        self.fusion_net, self.central_classifier = net, cls

    def forward(self, xs):
        return self.fusion_net.forward_classified(list(xs), self.central_classifier)


def _batch(cfg, batch, seed, nout=8):
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, batch, seed)]
    return xs, synth.make_labels('bce', batch, nout, seed).to(dev())


@pytest.mark.parametrize('key', list(FOUND))
def test_found_network_eager_step_native_equals_composed(key):
    model, cfg, batch = build_found(key, 57)
    set_mode(model, 'train')
    xs, y = _batch(cfg, batch, 57)

    def step():
        model.zero_grad()
        ins = [x.clone().requires_grad_(True) for x in xs]
        logits = model(ins)
        torch.nn.functional.binary_cross_entropy_with_logits(logits, y).backward()
        torch.cuda.synchronize()
        return logits.detach().clone(), {k: v.grad.clone() for k, v in model.named_parameters()}, [i.grad for i in ins]

    (la, ga, ia), n = native_launches(step)
    assert n == cfg.S
    with forced_composed():
        (lb, gb, ib), n = native_launches(step)
    assert n == 0
    assert_close_scaled('logits', la, lb, rel=1e-4)
    assert sum('.attn.' in k for k in ga) == 4 * cfg.S
    for k, v in ga.items():
        if k.endswith('conv.bias'):                              # in front of a train-mode BatchNorm: zero
            assert float(v.abs().max()) < 1e-4 and float(gb[k].abs().max()) < 1e-4, k
        else:
            assert_close_scaled('grad ' + k, v, gb[k], rel=2e-4)
    for i, (a, b_) in enumerate(zip(ia, ib)):
        assert_close_scaled(f'grad input.{i}', a, b_, rel=2e-4)


@pytest.mark.parametrize('key', list(FOUND))
def test_captured_found_step_matches_its_eager_twin(key):
    """GraphedTrainStep (forward, criterion, backward, Adam as one replay) with dropout off: the loss and every
    gradient of replay 1 against an eager twin built from the same parameters."""
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    crit = bnn.BCEWithLogitsLoss()
    models = []
    for _ in range(2):
        model, cfg, batch = build_found(key, 57, linear=bnn.Linear)
        set_mode(model, 'train')
        models.append(model)
    xs, y = _batch(cfg, batch, 57)
    opts = [Adam(list(m.parameters()), lr=1e-3, weight_decay=1e-4) for m in models]
    (g, n) = native_launches(lambda: GraphedTrainStep(models[0], crit, opts[0], xs, y))
    assert n >= cfg.S                                           # the attention core is inside the capture
    loss1 = float(g(xs, y)[0])
    torch.cuda.synchronize()
    grads1 = {k: v.grad.detach().clone() for k, v in models[0].named_parameters() if v.grad is not None}
    opts[1].zero_grad()
    loss_e = crit(models[1](xs), y)
    loss_e.backward()
    torch.cuda.synchronize()
    loss_e = float(loss_e.detach())
    assert abs(loss1 - loss_e) <= 1e-4 * max(1.0, abs(loss_e)), (loss1, loss_e)
    seen = 0
    for k, v in models[1].named_parameters():
        assert v.grad is not None and k in grads1, k
        if k.endswith('conv.bias'):
            assert float(grads1[k].abs().max()) < 1e-4, k
        else:
            assert_close_scaled('grad:' + k, grads1[k], v.grad, rel=2e-4)
            seen += '.attn.' in k
    assert seen == 4 * cfg.S


def test_captured_found_step_draws_fresh_attention_masks():
    """Live attention dropout (every nn.Dropout of the network an identity, so the attention's is the only site) and a
    learning rate of zero: two replays run on the same weights and batch, differ, and every output is finite."""
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    from fc_edges_util import recorded_sites
    model, cfg, batch = build_found('two_steps', 57, drpt=0.3, linear=bnn.Linear)
    set_mode(model, 'train_nodrop')
    assert all(m.attn.dropout == 0.3 for m in attention_modules(model))
    xs, y = _batch(cfg, batch, 57)
    opt = Adam(list(model.parameters()), lr=0.0, weight_decay=0.0)
    before = [p.detach().clone() for p in model.parameters()]
    with recorded_sites() as rec:
        g = GraphedTrainStep(model, bnn.BCEWithLogitsLoss(), opt, xs, y)
    sites = [r for r in rec if r[0].step]
    assert sites and len(sites) % cfg.S == 0 and all(n == batch * 2 * cfg.L * cfg.L for _, n in sites)
    outs = []
    for _ in range(2):
        r = g(xs, y)
        torch.cuda.synchronize()
        outs.append([t.detach().clone() for t in r[:2]])
    for loss, logits in outs:
        assert bool(torch.isfinite(loss).all()) and bool(torch.isfinite(logits).all())
    assert not torch.equal(outs[0][1], outs[1][1])
    assert all(torch.equal(a, b) for a, b in zip(before, model.parameters()))
    assert all(bool(torch.isfinite(p.grad).all()) for p in model.parameters() if p.grad is not None)
