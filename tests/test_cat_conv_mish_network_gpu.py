"""-m gpu: whole networks with the CatConvMish step-node primitive (reference
models/search/darts/node_operations.py:58-82).

The search hypernet with STEP_STEP_PRIMITIVES = ['Sum', 'ScaleDotAttn', 'LinearGLU', 'CatConvMish'] — a four-entry list
that is not the default, every NodeMixedOp on the selected-term kernels with the Mish activation in the FC slot — as a
whole step against the CPU restatement swapped into the oracle (cat_conv_mish_util.patch_oracle) through
gpu_util.match_step, against the forced composed sum, and captured as a hipGraph.  Found networks whose genotype names
the primitive (Found_NodeCell.compile looks it up in STEP_STEP_OPS; the standalone conv GEMM + bn_mish tail, through
forward_thru) against fo.found_cell with fo._found_node_op taught the name.

The pattern is tests/test_node_prims_network_gpu.py's; tolerances are the project's (1e-4 of scale for outputs and
buffers, 2e-4 for gradients)."""
import contextlib

import numpy as np
import pytest
import torch

import cat_conv_mish_util as cm
from cat_conv_mish_util import BUILTIN4, MISH, list_id
from fc_edges_util import recorded_sites
from gpu_util import Args, assert_close_scaled, dev, match_step, set_mode
from oracle import fusion_oracle as fo
from oracle import synth

pytestmark = pytest.mark.gpu

HEADS = {'mmimdb': (23, 'bce'), 'ntu': (60, 'ce')}
SEED = 31


@contextlib.contextmanager
def forced_composed():
    import models.search.darts.node_operations as no
    saved = no.NODE_PRIMS_NATIVE
    no.NODE_PRIMS_NATIVE = False
    try:
        yield
    finally:
        no.NODE_PRIMS_NATIVE = saved


def make_arch(cfg, prims, seed=SEED):
    """synth.make_arch with gammas of len(prims) columns (fo.arch_shapes reads fo.STEP_STEP_PRIMITIVES: patched)."""
    assert fo.STEP_STEP_PRIMITIVES == prims
    return synth.make_arch(cfg, seed, 0.5)


def build(cfg, nout, mode, prims, seed=SEED, linear=None):
    from models.search.darts.model_search import FusionNetwork
    with cm.mish_list(prims):
        net = FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), criterion=None)
    shapes = cm.net_param_shapes(cfg, prims)
    assert set(net.state_dict().keys()) == set(shapes.keys())
    net.load_state_dict(synth.make_params(cfg, seed, shapes))
    arch = make_arch(cfg, prims, seed)
    for i, (dst, src) in enumerate(zip(net.arch_parameters(), arch)):
        assert dst.shape == src.shape
        if i and i % 2 == 0:
            assert dst.shape == (cfg.ns, len(prims))        # gammas: one column per listed primitive
        dst.data.copy_(src)
    net.to(dev())
    set_mode(net, mode)
    cls = (linear or torch.nn.Linear)(cfg.M * cfg.C * cfg.L, nout)
    cw, cb = synth.make_classifier(cfg, nout, seed)
    cls.weight.data.copy_(cw)
    cls.bias.data.copy_(cb)
    cls.to(dev())
    return net, cls


def run_step(cfg, batch, nout, loss_kind, mode, prims, seed=SEED):
    net, cls = build(cfg, nout, mode, prims, seed)
    xs = [x.to(dev()).requires_grad_(True) for x in synth.make_inputs(cfg, batch, seed)]
    y = synth.make_labels(loss_kind, batch, nout, seed).to(dev())
    crit = torch.nn.BCEWithLogitsLoss() if loss_kind == 'bce' else torch.nn.CrossEntropyLoss()
    with cm.edited_step_prims(prims):                       # genotype() reads the list
        logits = cls(net(xs))
        loss = crit(logits, y)
        loss.backward()
        geno = fo.genotype_to_jsonable(net.genotype())
    torch.cuda.synchronize()
    return net, cls, xs, logits, loss, geno


def compare_step(cfg, batch, nout, loss_kind, prims, net, cls, xs, logits, loss, geno, label, seed=SEED):
    """Every tensor of the step against the patched oracle, over the edited list's parameter shapes."""
    shapes = cm.net_param_shapes(cfg, prims)

    def evaluate(double, flips, near):
        f = (lambda t: t.double() if t.is_floating_point() else t) if double else (lambda t: t)
        p = {k: f(v) for k, v in synth.make_params(cfg, seed, shapes).items()}
        cw, cb = synth.make_classifier(cfg, nout, seed)
        with fo.relu_decisions(near, flips) as rd:           # (the reshape-free hypernet's other ReLUs: the cell's tail)
            lg, ls, grads = fo.search_step([f(x) for x in synth.make_inputs(cfg, batch, seed)],
                                           synth.make_labels(loss_kind, batch, nout, seed),
                                           [f(a) for a in make_arch(cfg, prims, seed)], p, f(cw), f(cb), cfg, loss_kind,
                                           training=True, attn_drop=0.0)
        want = {'logits': lg, 'loss': ls, '_params': p}
        for k, v in grads.items():
            want['grad:' + k] = v
        return want, rd.ambiguous

    got, specs = {'logits': logits, 'loss': loss}, {'logits': (1e-4, True), 'loss': (1e-4, True)}
    for k, v in net.named_parameters():
        assert v.grad is not None, k
        if k.endswith('conv.bias'):
            assert float(v.grad.abs().max()) < 1e-4, k       # mathematically zero (BN removes the mean)
        else:
            got['grad:' + k] = v.grad
    for i, a in enumerate(net.arch_parameters()):
        got[f'grad:arch.{i}'] = a.grad
    for i, x in enumerate(xs):
        got[f'grad:input.{i}'] = x.grad
    for k in ('weight', 'bias'):
        got['grad:central_classifier.' + k] = getattr(cls, k).grad
    for k in got:
        specs.setdefault(k, (2e-4, False))
    how = match_step(got, specs, evaluate, label)
    p32 = evaluate(False, (), 0.0)[0]['_params']
    for k, v in net.state_dict().items():
        if fo.is_buffer(k):
            assert_close_scaled('buf:' + k, v.float(), p32[k].float())
    assert geno == fo.genotype_to_jsonable(fo.network_genotype(make_arch(cfg, prims, seed), cfg))
    return how


def assert_routes(net, want):
    import models.search.darts.node_operations as no
    seen = 0
    for n in net.cell._step_nodes:
        for op in n.node_cell.node_ops:
            z = torch.zeros(2, op.C, op.L, device=dev())
            assert no.node_mix_route(op, z, z, torch.zeros(len(op._prims), device=dev())) == want
            assert not op._default and type(op._ops[3]) is no.CatConvMish
            seen += 1
    assert seen


# ------------------------------------------------------------------------------------------ the search hypernet
@pytest.mark.parametrize('name,batch', [('mmimdb', 32), ('ntu', 8)])
def test_whole_step_matches_restatement(name, batch, monkeypatch):
    from bmnas import lib
    prims = BUILTIN4
    cm.patch_oracle(monkeypatch, prims)
    cfg = fo.Cfg({**fo.CONFIGS[name], 'drpt': 0.0})          # dropout as identity, in the modules and in the oracle
    nout, loss_kind = HEADS[name]
    before = dict(lib.NODE_SEL_LAUNCHES)
    net, cls, xs, logits, loss, geno = run_step(cfg, batch, nout, loss_kind, 'train_nodrop', prims)
    assert not net.cell._fusable or not all(op._default for n in net.cell._step_nodes for op in n.node_cell.node_ops)
    assert_routes(net, 'selected')
    assert lib.NODE_SEL_LAUNCHES['fwd'] - before['fwd'] == cfg.S * cfg.ns
    assert lib.NODE_SEL_LAUNCHES['bwd'] - before['bwd'] == cfg.S * cfg.ns
    compare_step(cfg, batch, nout, loss_kind, prims, net, cls, xs, logits, loss, geno,
                 f'catconvmish {list_id(prims)}: {name} b{batch}')


def test_native_path_and_forced_composed_agree(monkeypatch):
    from bmnas import lib
    prims = BUILTIN4
    cm.patch_oracle(monkeypatch, prims)
    name, batch = 'ntu', 8
    cfg = fo.Cfg({**fo.CONFIGS[name], 'drpt': 0.0})
    nout, loss_kind = HEADS[name]
    a = run_step(cfg, batch, nout, loss_kind, 'train_nodrop', prims)
    before = dict(lib.NODE_SEL_LAUNCHES)
    with forced_composed():
        b = run_step(cfg, batch, nout, loss_kind, 'train_nodrop', prims)
        assert_routes(b[0], 'composed')
    assert lib.NODE_SEL_LAUNCHES == before                     # the composed sum issued none of the mix launches
    assert_close_scaled('logits', a[3], b[3], rel=1e-4)
    assert_close_scaled('loss', a[4], b[4], rel=1e-4)
    ga, gb = dict(a[0].named_parameters()), dict(b[0].named_parameters())
    for k, v in ga.items():
        if k.endswith('conv.bias'):
            assert float(v.grad.abs().max()) < 1e-4 and float(gb[k].grad.abs().max()) < 1e-4, k
        else:
            assert_close_scaled('grad:' + k, v.grad, gb[k].grad, rel=2e-4)
    for pa, pb in zip(a[0].arch_parameters(), b[0].arch_parameters()):
        assert_close_scaled('grad:arch', pa.grad, pb.grad, rel=2e-4)
    for xa, xb in zip(a[2], b[2]):
        assert_close_scaled('grad:input', xa.grad, xb.grad, rel=2e-4)
    for k, v in a[0].state_dict().items():
        if fo.is_buffer(k):
            assert_close_scaled('buf:' + k, v.float(), b[0].state_dict()[k].float())
    assert a[5] == b[5]


class _Step(torch.nn.Module):
    def __init__(self, net, cls):
        super().__init__()
        self.net, self.cls = net, cls

    def arch_parameters(self):
        return self.net.arch_parameters()

    def forward(self, xs):
        return self.cls(self.net(xs))


def test_captured_step_replay_matches_its_eager_twin(monkeypatch):
    """bmnas.graph.GraphedTrainStep over the hypernet (forward, criterion, backward, Adam as one replay; the mix
    kernels with the Mish FC slot inside the capture), live dropout.  Replay 1 against an eager twin that draws the
    SAME masks (its host-side Philox offset is set to the step-counter value the replay's sites read), gradient by
    gradient."""
    from bmnas import cell as K
    from bmnas import lib
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    prims = BUILTIN4
    cm.patch_oracle(monkeypatch, prims)                      # (arch shapes of make_arch)
    name, batch = 'mmimdb', 32
    cfg = fo.CONFIGS[name]
    assert cfg.drpt > 0
    nout, loss_kind = HEADS[name]
    crit = bnn.BCEWithLogitsLoss()
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, batch, SEED)]
    y = synth.make_labels(loss_kind, batch, nout, SEED).to(dev())
    models = [_Step(*build(cfg, nout, 'train', prims, linear=bnn.Linear)) for _ in range(2)]
    opts = [Adam(list(m.parameters()), lr=1e-3, weight_decay=1e-4) for m in models]
    before = dict(lib.NODE_SEL_LAUNCHES)
    with cm.edited_step_prims(prims), recorded_sites() as rec:
        g = GraphedTrainStep(models[0], crit, opts[0], xs, y)
    assert lib.NODE_SEL_LAUNCHES['fwd'] > before['fwd'] and lib.NODE_SEL_LAUNCHES['bwd'] > before['bwd']
    rec = [r for r in rec if r[0].step]                  # the captured step's sites (warm-up passes are eager)
    owners = sum(q != 'Sum' for q in prims)
    assert len(rec) >= cfg.S * cfg.ns * owners and len(rec) % owners == 0, (len(rec), owners)
    loss1 = float(g(xs, y)[0])
    torch.cuda.synchronize()
    step1 = g._g.site_step_value()
    grads1 = {k: v.grad.detach().clone() for k, v in models[0].named_parameters() if v.grad is not None}
    masks1 = lib.dropout_mask(rec[0][0], rec[0][1], dev(), step1).cpu()
    assert 0.03 < float((masks1 == 0).float().mean()) < 0.3
    saved = K.DROP.offset
    K.DROP.offset = step1
    try:
        opts[1].zero_grad()
        loss_e = crit(models[1](xs), y)
        loss_e.backward()
    finally:
        K.DROP.offset = saved
    torch.cuda.synchronize()
    assert type(models[1].net.cell._step_nodes[0].node_cell.node_ops[0]._ops[3]).__name__ == MISH
    assert abs(loss1 - float(loss_e)) <= 1e-4 * max(1.0, abs(float(loss_e))), (loss1, float(loss_e))
    seen = 0
    for k, v in models[1].named_parameters():
        assert v.grad is not None, k
        if k.endswith('conv.bias'):
            assert float(grads1[k].abs().max()) < 1e-4, k
        else:
            assert_close_scaled('grad:' + k, grads1[k], v.grad, rel=2e-4)
            seen += '.node_ops.' in k
    assert seen > 0


# ------------------------------------------------------------------------------------------ found networks
def _skip(*idx):
    return [('skip', i) for i in idx]


# two step nodes, both reading the two inputs; the cell's tail concatenates both
FOUND = {
    'two_steps': (fo.make_cfg(N=2, C=32, L=16, S=2, M=2, ns=2, nm=2, drpt=0.0), 5,
                  [_skip(0, 1, 1, 2), _skip(1, 0, 0, 2)], [MISH, 'ScaleDotAttn'], [2, 3]),
    'one_step': (fo.make_cfg(N=2, C=16, L=8, S=2, M=2, ns=1, nm=1, drpt=0.0), 4,
                 [_skip(0, 1), _skip(1, 0)], [MISH], [2]),
}


def found_genotype(key):
    cfg, batch, inner_edges, inner_steps, inner_concat = FOUND[key]
    g = fo.Genotype(edges=_skip(0, 1, 1, 0), concat=[2, 3],
                    steps=[fo.StepGenotype(inner_edges=e, inner_steps=list(inner_steps), inner_concat=list(inner_concat))
                           for e in inner_edges])
    return cfg, batch, g


def build_found(cfg, g, seed, mode):
    """gpu_util.build_found_net with the name registered while the network is constructed and the parameter shapes of
    the substituted genotype."""
    from models.search.darts.genotypes import Genotype, StepGenotype
    from models.search.darts.model import Found_FusionNetwork
    import models.search.darts.node_operations as no
    gg = Genotype(edges=[tuple(e) for e in g.edges],
                  steps=[StepGenotype(inner_edges=[tuple(e) for e in s.inner_edges], inner_steps=list(s.inner_steps),
                                      inner_concat=list(s.inner_concat)) for s in g.steps],
                  concat=list(g.concat))
    with cm.registered():
        net = Found_FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), None, gg)
    shapes = fo.found_param_shapes(cfg, cm.substituted_genotype(g))
    assert set(net.state_dict()) == set(shapes)
    net.load_state_dict(synth.make_params(cfg, seed, shapes))
    assert all(type(n.node_cell.node_ops[0]) is no.CatConvMish for n in net.cell._step_nodes)
    net.to(dev())
    set_mode(net, mode)
    return net, shapes


@pytest.mark.parametrize('mode', ['train_nodrop', 'eval'])
@pytest.mark.parametrize('key', list(FOUND))
def test_found_network_matches_restatement(key, mode, monkeypatch):
    cm.patch_found_oracle(monkeypatch)
    cfg, batch, g = found_genotype(key)
    seed, training = 57, mode != 'eval'
    net, shapes = build_found(cfg, g, seed, mode)
    xs = [x.to(dev()).requires_grad_(True) for x in synth.make_inputs(cfg, batch, seed)]
    feat = net(xs)
    w = torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(tuple(feat.shape))
                         .astype(np.float32))
    feat.backward(w.to(dev()))
    torch.cuda.synchronize()
    p = synth.make_params(cfg, seed, shapes)
    pp = {k: (v if fo.is_buffer(k) else v.requires_grad_(True)) for k, v in p.items()}
    xo = [x.requires_grad_(True) for x in synth.make_inputs(cfg, batch, seed)]
    ofeat = fo.found_cell(xo, g, pp, cfg, training, attn_drop=0.0)
    ofeat.backward(w)
    assert_close_scaled('feat', feat, ofeat)
    for i, (a, b_) in enumerate(zip(xs, xo)):
        assert_close_scaled(f'grad:input.{i}', a.grad, b_.grad, rel=2e-4)
    seen = 0
    for k, v in net.named_parameters():
        want = pp[k].grad
        assert want is not None and v.grad is not None, k
        if k.endswith('conv.bias') and training:
            assert float(v.grad.abs().max()) < 1e-4, k
        else:
            assert_close_scaled('grad:' + k, v.grad, want, rel=2e-4)
        seen += '.node_ops.0.' in k
    assert seen == 4 * cfg.S
    for k, v in net.state_dict().items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == int(p[k]) == (1 if training else 0), k
        elif fo.is_buffer(k):
            assert_close_scaled('buf:' + k, v.float(), p[k].float())


class _FoundStep(torch.nn.Module):
    """fusion_net -> central_classifier, wired like the reference's Found_*_Net minus backbones and reshape layers."""
    def __init__(self, net, cls):
        super().__init__()
        self.fusion_net, self.central_classifier = net, cls

    def forward(self, xs):
        return self.fusion_net.forward_classified(list(xs), self.central_classifier)


@pytest.mark.parametrize('key', list(FOUND))
def test_found_step_holds_no_aten_kernel(key):
    """No aten kernel among the device events of the found network's forward and backward, where the project makes
    that claim for every found network (tests/test_graph_forward_gpu.py): in the captured step, whose zero-filled
    accumulators come from the step's arena (an eager pass fills them with torch.zeros, whatever the genotype).  One
    replay is forward, criterion, backward and Adam."""
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    from torch.profiler import ProfilerActivity, profile
    cfg, batch, g = found_genotype(key)
    seed, nout = 57, 8
    net, _ = build_found(cfg, g, seed, 'train_nodrop')
    cls = bnn.Linear(cfg.M * cfg.C * cfg.L, nout)
    cw, cb = synth.make_classifier(cfg, nout, seed)
    cls.weight.data.copy_(cw)
    cls.bias.data.copy_(cb)
    model = _FoundStep(net, cls.to(dev())).train()
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, batch, seed)]
    y = synth.make_labels('bce', batch, nout, seed).to(dev())
    opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
    step = GraphedTrainStep(model, bnn.BCEWithLogitsLoss(), opt, xs, y)
    ref = [q.detach().clone() for q in model.parameters()]
    step(xs, y)
    torch.cuda.synchronize()
    assert any(not torch.equal(a, b) for a, b in zip(ref, model.parameters()))     # the replays do train
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss = step(xs, y)[0]
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    aten = [n for n in names if 'at::native' in n]
    print(f'{key}: {len(names)} device events, aten: {aten}')
    assert any('bn_mish_fwd_k' in n for n in names) and any('bn_mish_bwd_k' in n for n in names), names
    assert not aten, aten
    assert torch.isfinite(loss).all()


@pytest.mark.parametrize('b,C,L', [(5, 32, 16), (7, 16, 8)])
def test_attention_forward_thru_gives_the_gradients_of_forward(b, C, L):
    """ScaledDotAttn.forward_thru (what keeps the two-step genotype above free of engine adds) hands both inputs back;
    later torch readers of both aliases see their gradient accumulated by the attention's backward launch: the same
    input and LayerNorm gradients as forward with the readers on x and y.  Also with one alias unread (its gradient
    slot arrives empty) and with the op's own output unread."""
    from models.search.darts.node_operations import ScaledDotAttn
    rng = np.random.Generator(np.random.PCG64(900 + b + C))
    r = lambda *s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
    x, y, g, lw, lb = r(b, C, L), r(b, C, L), r(b, C, L), 1.0 + 0.1 * r(C, L), 0.1 * r(C, L)
    readers = {'both': lambda s, ax, ay: s * 1.5 + ax * ay + ax.sin(),
               'x only': lambda s, ax, ay: s * 1.5 + ax.sin(),
               'aliases only': lambda s, ax, ay: ax * ay + ay.cos()}
    for name, read in readers.items():
        res = []
        for thru in (False, True):
            m = ScaledDotAttn(C, L)
            m.ln.weight.data.copy_(lw)
            m.ln.bias.data.copy_(lb)
            m.to(dev()).train()
            m.dropout.p = 0.0
            xd, yd = x.to(dev()).requires_grad_(True), y.to(dev()).requires_grad_(True)
            if thru:
                s, ax, ay = m.forward_thru(xd, yd)
                assert type(s.grad_fn).__name__ == 'SdpaLnThruFnBackward'
            else:
                s, ax, ay = m(xd, yd), xd, yd
            read(s, ax, ay).backward(g.to(dev()))
            torch.cuda.synchronize()
            res.append([s.detach(), xd.grad, yd.grad, m.ln.weight.grad, m.ln.bias.grad])
        for i, (a, b_) in enumerate(zip(*res)):
            if a is None:
                assert b_ is None or float(b_.abs().max()) == 0.0, (name, i)
            else:
                assert_close_scaled(f'{name}: tensor {i}', b_, a, rel=2e-4 if i else 1e-4)
