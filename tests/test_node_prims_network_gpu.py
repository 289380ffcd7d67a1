"""-m gpu: the search hypernet with STEP_STEP_PRIMITIVES edited — its NodeMixedOps on the selected-term kernels
(csrc/nodemix_sel.hip) — as a whole step: against the CPU oracle through gpu_util.match_step (the edited list swapped
into the oracle with monkeypatch, node_prims_util.patch_oracle), against the forced composed sum, and captured as a
hipGraph."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import fusion_oracle as fo
from oracle import synth
from fc_edges_util import recorded_sites
from gpu_util import Args, assert_close_scaled, dev, match_step, set_mode
from node_prims_util import edited_step_prims, list_id, net_param_shapes, patch_oracle

pytestmark = pytest.mark.gpu

LISTS = [['Sum', 'ScaleDotAttn'], ['ConcatFC', 'Sum', 'LinearGLU']]
HEADS = {'mmimdb': (23, 'bce'), 'ntu': (60, 'ce'), 'ego': (83, 'ce')}
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
    with edited_step_prims(prims):
        net = FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), criterion=None)
    shapes = net_param_shapes(cfg, prims)
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
    with edited_step_prims(prims):                          # genotype() reads the list
        logits = cls(net(xs))
        loss = crit(logits, y)
        loss.backward()
        geno = fo.genotype_to_jsonable(net.genotype())
    torch.cuda.synchronize()
    return net, cls, xs, logits, loss, geno


def compare_step(cfg, batch, nout, loss_kind, prims, net, cls, xs, logits, loss, geno, label, seed=SEED):
    """gpu_util.compare_search_step over the patched oracle and the edited list's parameter shapes."""
    shapes = net_param_shapes(cfg, prims)

    def evaluate(double, flips, near):
        f = (lambda t: t.double() if t.is_floating_point() else t) if double else (lambda t: t)
        p = {k: f(v) for k, v in synth.make_params(cfg, seed, shapes).items()}
        cw, cb = synth.make_classifier(cfg, nout, seed)
        with fo.relu_decisions(near, flips) as rd:
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
    for n in net.cell._step_nodes:
        for op in n.node_cell.node_ops:
            z = torch.zeros(2, op.C, op.L, device=dev())
            assert no.node_mix_route(op, z, z, torch.zeros(len(op._prims), device=dev())) == want


@pytest.mark.parametrize('name,batch', [('mmimdb', 32), ('ntu', 8), ('ntu', 7), ('ego', 6)])
@pytest.mark.parametrize('prims', LISTS, ids=list_id)
def test_whole_step_matches_oracle(prims, name, batch, monkeypatch):
    from bmnas import lib
    patch_oracle(monkeypatch, prims)
    cfg = fo.Cfg({**fo.CONFIGS[name], 'drpt': 0.0})          # dropout as identity, in the modules and in the oracle
    nout, loss_kind = HEADS[name]
    before = dict(lib.NODE_SEL_LAUNCHES)
    net, cls, xs, logits, loss, geno = run_step(cfg, batch, nout, loss_kind, 'train_nodrop', prims)
    assert not net.cell._fusable or not all(op._default for n in net.cell._step_nodes for op in n.node_cell.node_ops)
    assert_routes(net, 'selected')
    assert lib.NODE_SEL_LAUNCHES['fwd'] - before['fwd'] == cfg.S * cfg.ns
    assert lib.NODE_SEL_LAUNCHES['bwd'] - before['bwd'] == cfg.S * cfg.ns
    compare_step(cfg, batch, nout, loss_kind, prims, net, cls, xs, logits, loss, geno,
                 f'nodeprims {list_id(prims)}: {name} b{batch}')


@pytest.mark.parametrize('prims', LISTS, ids=list_id)
def test_native_path_and_forced_composed_agree(prims, monkeypatch):
    from bmnas import lib
    patch_oracle(monkeypatch, prims)
    name, batch = 'ntu', 8
    cfg = fo.Cfg({**fo.CONFIGS[name], 'drpt': 0.0})
    nout, loss_kind = HEADS[name]
    a = run_step(cfg, batch, nout, loss_kind, 'train_nodrop', prims)
    before = dict(lib.NODE_SEL_LAUNCHES)
    with forced_composed():
        b = run_step(cfg, batch, nout, loss_kind, 'train_nodrop', prims)
        assert_routes(b[0], 'composed')
    assert lib.NODE_SEL_LAUNCHES == before                     # the composed sum issued none of the new launches
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
    assert a[5] == b[5]


class _Step(torch.nn.Module):
    def __init__(self, net, cls):
        super().__init__()
        self.net, self.cls = net, cls

    def arch_parameters(self):
        return self.net.arch_parameters()

    def forward(self, xs):
        return self.cls(self.net(xs))


@pytest.mark.parametrize('prims', LISTS, ids=list_id)
def test_captured_step_replays_with_fresh_masks_and_matches_eager(prims, monkeypatch):
    """bmnas.graph.GraphedTrainStep over the edited-list hypernet (forward, criterion, backward, Adam as one replay),
    live dropout.  Replay 1 against an eager twin that draws the SAME masks (its host-side Philox offset is set to the
    step-counter value the replay's sites read: same seed, same counters), gradient by gradient; replay 2 draws
    other masks."""
    from bmnas import cell as K
    from bmnas import lib
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    patch_oracle(monkeypatch, prims)                         # (arch shapes of make_arch)
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
    with recorded_sites() as rec:
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
    # the eager twin under the same masks
    saved = K.DROP.offset
    K.DROP.offset = step1
    try:
        opts[1].zero_grad()
        loss_e = crit(models[1](xs), y)
        loss_e.backward()
    finally:
        K.DROP.offset = saved
    torch.cuda.synchronize()
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
    loss2 = float(g(xs, y)[0])
    torch.cuda.synchronize()
    step2 = g._g.site_step_value()
    masks2 = lib.dropout_mask(rec[0][0], rec[0][1], dev(), step2).cpu()
    assert step2 != step1 and not torch.equal(masks1, masks2)
    assert np.isfinite(loss2) and loss2 != loss1
