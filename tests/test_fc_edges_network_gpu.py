"""-m gpu: the search hypernet with PRIMITIVES edited to ['none', 'fc_relu', 'fc_mish', 'skip'] — its mixed-edge sums
on the grouped FC-edge kernels (csrc/fcedge.hip) — as a whole step: against the CPU oracle through
gpu_util.match_step, with live dropout under exported masks, against the composed fallback, captured as a hipGraph,
and against the reference's own outputs at the production sizes (tests/golden/fcedge_*.npz)."""
import contextlib
import json

import numpy as np
import pytest
import torch

from oracle import fusion_oracle as fo
from oracle import synth
from fc_edges_util import device_kernels, edited_primitives, recorded_sites
from gpu_util import Args, assert_close_scaled, assert_summary_scaled, dev, match_step, set_mode
from util import case_id, cfg_of, golden_files, load_npz

pytestmark = pytest.mark.gpu

PRIMS = ['none', 'fc_relu', 'fc_mish', 'skip']
HEADS = {'mmimdb': (23, 'bce'), 'ntu': (60, 'ce'), 'ego': (83, 'ce')}
SEED = 31


@contextlib.contextmanager
def forced_fallback():
    from models.search.darts import operations as ops_mod
    saved = ops_mod.FC_EDGES_NATIVE
    ops_mod.FC_EDGES_NATIVE = False
    try:
        yield
    finally:
        ops_mod.FC_EDGES_NATIVE = saved


def build(cfg, nout, mode, seed=SEED, prims=PRIMS, linear=None):
    from models.search.darts.model_search import FusionNetwork
    with edited_primitives(prims):
        net = FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), criterion=None)
        shapes = fo.param_shapes(cfg, prims)
        assert set(net.state_dict().keys()) == set(shapes.keys())
        net.load_state_dict(synth.make_params(cfg, seed, shapes))
        for dst, src in zip(net.arch_parameters(), synth.make_arch(cfg, seed, 0.5, prims)):
            assert dst.shape == src.shape
            dst.data.copy_(src)
    net.to(dev())
    set_mode(net, mode)
    cls = (linear or torch.nn.Linear)(cfg.M * cfg.C * cfg.L, nout)
    cw, cb = synth.make_classifier(cfg, nout, seed)
    cls.weight.data.copy_(cw)
    cls.bias.data.copy_(cb)
    cls.to(dev())
    return net, cls


def run_step(cfg, batch, nout, loss_kind, mode, seed=SEED):
    net, cls = build(cfg, nout, mode, seed)
    xs = [x.to(dev()).requires_grad_(True) for x in synth.make_inputs(cfg, batch, seed)]
    y = synth.make_labels(loss_kind, batch, nout, seed).to(dev())
    crit = torch.nn.BCEWithLogitsLoss() if loss_kind == 'bce' else torch.nn.CrossEntropyLoss()
    with edited_primitives(PRIMS):              # genotype() reads the list
        logits = cls(net(xs))
        loss = crit(logits, y)
        loss.backward()
        geno = fo.genotype_to_jsonable(net.genotype())
    torch.cuda.synchronize()
    return net, cls, xs, logits, loss, geno


def compare_step(cfg, batch, nout, loss_kind, net, cls, xs, logits, loss, geno, masks, attn_drop, label, seed=SEED):
    """gpu_util.compare_search_step with the edited list handed to the oracle (that helper has no such argument)."""
    def evaluate(double, flips, near):
        f = (lambda t: t.double() if t.is_floating_point() else t) if double else (lambda t: t)
        p = {k: f(v) for k, v in synth.make_params(cfg, seed, fo.param_shapes(cfg, PRIMS)).items()}
        cw, cb = synth.make_classifier(cfg, nout, seed)
        inj = fo.injected_masks(masks) if masks is not None else contextlib.nullcontext()
        with inj, fo.relu_decisions(near, flips) as rd:
            lg, ls, grads = fo.search_step([f(x) for x in synth.make_inputs(cfg, batch, seed)],
                                           synth.make_labels(loss_kind, batch, nout, seed),
                                           [f(a) for a in synth.make_arch(cfg, seed, 0.5, PRIMS)], p, f(cw), f(cb), cfg,
                                           loss_kind, training=True, attn_drop=attn_drop, primitives=PRIMS)
        if masks is not None:
            assert inj.used == len(masks)
        want = {'logits': lg, 'loss': ls, '_params': p, '_none': [k for k, v in grads.items() if v is None]}
        for k, v in grads.items():
            if v is not None:
                want['grad:' + k] = v
        return want, rd.ambiguous

    got, specs = {'logits': logits, 'loss': loss}, {'logits': (1e-4, True), 'loss': (1e-4, True)}
    unreached = []
    for k, v in net.named_parameters():
        if v.grad is None:
            unreached.append(k)              # the inner edges' third / fourth primitive (zip quirk)
        elif k.endswith('conv.bias'):
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
    w32 = evaluate(False, (), 0.0)[0]
    assert sorted(unreached) == sorted(w32['_none']) and unreached, (unreached, w32['_none'])
    for k, v in net.state_dict().items():
        if fo.is_buffer(k):
            assert_close_scaled('buf:' + k, v.float(), w32['_params'][k].float())
    arch = synth.make_arch(cfg, seed, 0.5, PRIMS)
    assert geno == fo.genotype_to_jsonable(fo.network_genotype(arch, cfg, PRIMS))
    return how


def assert_native(net, want=True):
    """The cell-level sums of this net take the FC-edge kernels (or, want=False, do not)."""
    from models.search.darts import operations as ops_mod
    cell = net.cell
    x = torch.zeros(2, cell.C, cell.L, device=dev())
    w = torch.zeros(len(cell._ops), len(PRIMS), device=dev())
    route = ops_mod.edge_sum_route(cell._ops, [x] * cell.num_input_nodes, w, 0)[0]
    assert (route == 'fc') == want, route


@pytest.mark.parametrize('name,batch', [('mmimdb', 32), ('mmimdb', 37), ('ntu', 64), ('ntu', 8), ('ntu', 7), ('ego', 48),
                                        ('ego', 6)])
def test_whole_step_matches_oracle(name, batch):
    cfg = fo.Cfg({**fo.CONFIGS[name], 'drpt': 0.0})          # dropout as identity, in the modules and in the oracle
    nout, loss_kind = HEADS[name]
    from bmnas import lib
    before = dict(lib.FC_EDGE_LAUNCHES)
    net, cls, xs, logits, loss, geno = run_step(cfg, batch, nout, loss_kind, 'train_nodrop')
    assert_native(net)
    sums = cfg.S * (1 + cfg.ns)                    # mixed-edge sums of the step: per cell step one + one per inner step
    assert lib.FC_EDGE_LAUNCHES['fwd'] - before['fwd'] == 3 * sums
    assert lib.FC_EDGE_LAUNCHES['bwd'] - before['bwd'] == 4 * sums
    compare_step(cfg, batch, nout, loss_kind, net, cls, xs, logits, loss, geno, None, 0.0, f'fcedge: {name} b{batch}')


def test_whole_step_with_live_dropout_matches_oracle():
    from bmnas import lib
    name, batch = 'mmimdb', 32
    cfg = fo.Cfg({**fo.CONFIGS[name], 'drpt': 0.1})
    nout, loss_kind = HEADS[name]
    with recorded_sites() as rec:
        net, cls, xs, logits, loss, geno = run_step(cfg, batch, nout, loss_kind, 'train')
    # per cell step: (N + i) edges x 2 FC sites, 2 inner edges x 1 (none + fc_relu), attention + GLU + ConcatFC
    want_sites = sum((cfg.N + i) * 2 + cfg.ns * (2 + 3) for i in range(cfg.S))
    assert len(rec) == want_sites, (len(rec), want_sites)
    masks = [lib.dropout_mask(d, n, dev()).cpu() for d, n in rec]
    compare_step(cfg, batch, nout, loss_kind, net, cls, xs, logits, loss, geno, masks, fo.ATTN_DROP,
                 f'fcedge drop: {name} b{batch}')


def test_native_path_and_forced_fallback_agree():
    name, batch = 'mmimdb', 32
    cfg = fo.Cfg({**fo.CONFIGS[name], 'drpt': 0.0})
    nout, loss_kind = HEADS[name]
    from bmnas import lib
    a = run_step(cfg, batch, nout, loss_kind, 'train_nodrop')
    before = dict(lib.FC_EDGE_LAUNCHES)
    with forced_fallback():
        b = run_step(cfg, batch, nout, loss_kind, 'train_nodrop')
        assert_native(b[0], False)
    assert lib.FC_EDGE_LAUNCHES == before                       # the fallback issued none of the new launches
    assert_close_scaled('logits', a[3], b[3], rel=1e-4)
    assert_close_scaled('loss', a[4], b[4], rel=1e-4)
    for (net, cls, xs, logits, loss, geno), label in ((a, 'native'), (b, 'fallback')):
        compare_step(cfg, batch, nout, loss_kind, net, cls, xs, logits, loss, geno, None, 0.0,
                     f'fcedge {label}: {name} b{batch}')


class _Step(torch.nn.Module):
    def __init__(self, net, cls):
        super().__init__()
        self.net, self.cls = net, cls

    def arch_parameters(self):
        return self.net.arch_parameters()

    def forward(self, xs):
        return self.cls(self.net(xs))


def test_captured_step_replays_with_fresh_masks_and_matches_eager():
    """bmnas.graph.GraphedTrainStep over the edited-list hypernet (forward, criterion, backward, Adam as one replay),
    live dropout.  Replay 1 against an eager twin that draws the SAME masks (its host-side Philox offset is set to the
    step-counter value the replay's sites read: same seed, same counters), gradient by gradient; replay 2 draws
    other masks."""
    from bmnas import cell as K
    from bmnas import lib
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    name, batch = 'ntu', 8
    cfg = fo.CONFIGS[name]
    nout, loss_kind = HEADS[name]
    crit = bnn.CrossEntropyLoss()
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, batch, SEED)]
    y = synth.make_labels(loss_kind, batch, nout, SEED).to(dev())
    models = [_Step(*build(cfg, nout, 'train', linear=bnn.Linear)) for _ in range(2)]
    opts = [Adam(list(m.parameters()), lr=1e-3, weight_decay=1e-4) for m in models]
    with recorded_sites() as rec:
        g = GraphedTrainStep(models[0], crit, opts[0], xs, y)
    rec = [r for r in rec if r[0].step]                  # the captured step's sites (warm-up passes are eager)
    assert len(rec) >= sum((cfg.N + i) * 2 + cfg.ns * 3 for i in range(cfg.S))
    loss1 = float(g(xs, y)[0])
    torch.cuda.synchronize()
    step1 = g._g.site_step_value()
    grads1 = {k: v.grad.detach().clone() for k, v in models[0].named_parameters() if v.grad is not None}
    masks1 = lib.dropout_mask(rec[0][0], rec[0][1], dev(), step1).cpu()
    assert 0.1 < float((masks1 == 0).float().mean()) < 0.3
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
        if v.grad is None:
            assert k not in grads1 or float(grads1[k].abs().max()) == 0.0, k
        elif k.endswith('conv.bias'):
            assert float(grads1[k].abs().max()) < 1e-4, k
        else:
            assert_close_scaled('grad:' + k, grads1[k], v.grad, rel=2e-4)
            seen += k.endswith('linear.weight')
    assert seen > 0
    loss2 = float(g(xs, y)[0])
    torch.cuda.synchronize()
    step2 = g._g.site_step_value()
    masks2 = lib.dropout_mask(rec[0][0], rec[0][1], dev(), step2).cpu()
    assert step2 != step1 and not torch.equal(masks1, masks2)
    assert np.isfinite(loss2) and loss2 != loss1


@pytest.mark.parametrize('path', golden_files('fcedge_*.npz'), ids=case_id)
def test_module_path_matches_reference_at_production_size(path):
    meta, z = load_npz(path)
    cfg = cfg_of(meta)
    assert meta['primitives'] == PRIMS
    seed, batch, nout = meta['seed'], meta['batch'], meta['num_outputs']
    net, cls = build(cfg, nout, meta['mode'], seed)
    assert_native(net)
    xs = [x.to(dev()).requires_grad_(True) for x in synth.make_inputs(cfg, batch, seed)]
    y = synth.make_labels(meta['loss'], batch, nout, seed).to(dev())
    crit = torch.nn.BCEWithLogitsLoss() if meta['loss'] == 'bce' else torch.nn.CrossEntropyLoss()
    with edited_primitives(PRIMS), torch.set_grad_enabled(meta['has_grads']):
        feat = net(xs)
        logits = cls(feat)
        loss = crit(logits, y)
        if meta['has_grads']:
            loss.backward()
        assert fo.genotype_to_jsonable(net.genotype()) == json.loads(str(z['genotype']))
    assert_summary_scaled('feat', feat, z['feat'])
    assert_close_scaled('logits', logits, z['logits'])
    assert_close_scaled('loss', loss, z['loss'])
    if meta['has_grads']:
        params = dict(net.named_parameters())
        for k in z.files:
            if not k.startswith('grad:'):
                continue
            nm = k[5:]
            if nm.startswith('arch.'):
                assert_close_scaled(k, net.arch_parameters()[int(nm.split('.')[1])].grad, z[k], rel=2e-4)
                continue
            if nm.startswith('input.'):
                got = xs[int(nm.split('.')[1])].grad
            elif nm.startswith('central_classifier.'):
                got = getattr(cls, nm.split('.')[1]).grad
            else:
                got = params[nm].grad
            if got is None:
                assert float(z[k][1]) == 0.0, k                     # never reached in the reference either
            elif nm.endswith('conv.bias') and meta['mode'] != 'eval':
                assert float(got.abs().max()) < 1e-4, k
            else:
                assert_summary_scaled(k, got, z[k])
    for k, v in net.state_dict().items():
        if fo.is_buffer(k):
            if v.dim() == 0:
                assert int(v) == int(z['buf:' + k]), k
            else:
                assert_summary_scaled('buf:' + k, v.float(), z['buf:' + k])
