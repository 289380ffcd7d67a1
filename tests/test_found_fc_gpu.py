"""-m gpu: Found_FusionNetwork over genotypes with fc_relu / fc_mish edges — the edges on the grouped kernels of
csrc/fcedge.hip (bmnas.functions.FoundFcEdgesFn) — against the reference's own outputs (tests/golden/fcfound_*.npz),
against the composed route, with shared and gradient-free sources, with live dropout under exported masks, as device
events, and captured as a hipGraph."""
import contextlib

import numpy as np
import pytest
import torch

import found_fc_util as fu
from fc_edges_util import device_kernels, recorded_sites
from gpu_util import assert_close_scaled, dev
from oracle import fusion_oracle as fo
from oracle import synth
from util import case_id

pytestmark = pytest.mark.gpu

FILES = fu.fixture_files()


@contextlib.contextmanager
def forced_composed():
    from models.search.darts import operations as ops_mod
    saved = ops_mod.FC_EDGES_NATIVE
    ops_mod.FC_EDGES_NATIVE = False
    try:
        yield
    finally:
        ops_mod.FC_EDGES_NATIVE = saved


def fixture(name):
    meta, z = fu.load([p for p in FILES if case_id(p) == name][0])
    cfg = fo.Cfg(meta['cfg'])
    g = fo.genotype_from_jsonable(meta['genotype'])
    params = synth.make_params(cfg, meta['seed'], fu.found_fc_param_shapes(cfg, g))
    xs = [torch.from_numpy(z[f'input.{i}']) for i in range(cfg.N)]
    return meta, z, cfg, g, params, xs


def fc_launches():
    from bmnas import lib
    return lib.FC_EDGE_LAUNCHES['fwd'] + lib.FC_EDGE_LAUNCHES['bwd']


def run(net, xs, seed, grads=True, need=None):
    """forward (+ backward under the PCG64(seed) cotangent) -> feat, input gradients."""
    xd = [x.to(dev()).requires_grad_(grads and (need is None or need[i])) for i, x in enumerate(xs)]
    with torch.set_grad_enabled(grads):
        feat = net(xd)
    if grads:
        (feat * fu.cotangent(seed, feat.shape).to(dev())).sum().backward()
    torch.cuda.synchronize()
    return feat, xd


@pytest.mark.parametrize('path', FILES, ids=case_id)
def test_found_network_with_fc_edges_matches_reference_golden(path):
    """Compared exactly the way test_found_network_matches_reference_golden (tests/test_network_gpu.py) compares."""
    meta, z, cfg, g, params, xs = fixture(case_id(path))
    net = fu.build_mirror(cfg, g, params, meta['mode'], dev())
    before = fc_launches()
    feat, xd = run(net, xs, meta['seed'], meta['has_grads'])
    n_groups = 1 + sum(i >= cfg.N for name, i in g.edges if name in fu.FC)
    kinds = len({name for name, i in g.edges if name in fu.FC and i < cfg.N})
    training = meta['mode'] != 'eval'
    want_launches = n_groups * (int(training) + 1) + kinds + (n_groups - 1) + (4 * n_groups if meta['has_grads'] else 0)
    assert fc_launches() - before == want_launches            # the grouped route ran, within its launch budget
    assert_close_scaled('feat', feat, z['feat'])
    if meta['has_grads']:
        named = dict(net.named_parameters())
        zero = fu.roundoff_zero_gradients(cfg, g, params, xs, meta['mode'], meta['seed'])
        for k in z.files:
            if k.startswith('grad:input.'):
                x = xd[int(k.split('.')[-1])]
                got = x.grad if x.grad is not None else torch.zeros_like(x)
                assert_close_scaled(k, got, z[k], rel=2e-4)
            elif k.startswith('grad:'):
                t = named[k[5:]]
                got = t.grad if t.grad is not None else torch.zeros_like(t)
                fu.assert_gradient(k, got, z[k], zero, meta['mode'], assert_close_scaled)
    for k, v in net.state_dict().items():
        if fo.is_buffer(k):
            assert_close_scaled('buf:' + k, v.float(), z['buf:' + k])


@pytest.mark.parametrize('name', ['fcfound_a_m_train_nodrop', 'fcfound_a_m_eval', 'fcfound_d_s_train_nodrop',
                                  'fcfound_c_s_train_nodrop'])
def test_native_and_forced_composed_agree(name):
    meta, z, cfg, g, params, xs = fixture(name)
    res = []
    for native in (True, False):
        net = fu.build_mirror(cfg, g, params, meta['mode'], dev())
        before = fc_launches()
        with contextlib.nullcontext() if native else forced_composed():
            feat, xd = run(net, xs, meta['seed'])
        assert (fc_launches() > before) == native                       # the composed route issues none of the launches
        res.append((net, feat, xd))
    (na, fa, xa), (nb, fb, xb) = res
    assert_close_scaled('feat', fa, fb, rel=1e-4)
    for i, (a, b) in enumerate(zip(xa, xb)):
        assert_close_scaled(f'grad:input.{i}', a.grad, b.grad, rel=2e-4)
    pb = dict(nb.named_parameters())
    zero = fu.roundoff_zero_gradients(cfg, g, params, xs, meta['mode'], meta['seed'])
    seen = 0
    for k, v in na.named_parameters():
        if pb[k].grad is None:
            assert v.grad is None or float(v.grad.abs().max()) == 0.0, k
        else:
            fu.assert_gradient('grad:' + k, v.grad, pb[k].grad, zero, meta['mode'], assert_close_scaled)
            seen += k.startswith('cell._ops.')
    assert seen == 4 * sum(name in fu.FC for name, _ in g.edges)
    for (k, a), (_, b) in zip(na.state_dict().items(), nb.state_dict().items()):
        if fo.is_buffer(k):
            assert_close_scaled('buf:' + k, a.float(), b.float())


def _fc_ops(training, kinds=('FC_Relu', 'FC_Mish', 'FC_Mish'), C=32, L=8, seed=5):
    from models.search.darts import operations as ops

    class A:
        drpt = 0.0
    torch.manual_seed(seed)
    mods = [getattr(ops, k)(C, L, A()).to(dev()).train(training) for k in kinds]
    for m in mods:
        with torch.no_grad():
            m.bn.weight.uniform_(0.5, 1.5)
            m.bn.bias.uniform_(-0.2, 0.2)
            m.bn.running_mean.uniform_(-0.2, 0.2)
            m.bn.running_var.uniform_(0.8, 1.5)
    return mods


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
def test_shared_source_gradient_is_returned_once_and_is_the_sum_of_its_edges_parts(training):
    """Edges 0 and 2 read the same tensor object: one gradient for it (the dx tiles of both edges share the
    destination), equal to the sum of what each edge alone sends back.  The single-edge calls run the same kernels over
    the same pre-activations, so no ReLU decision can differ."""
    from models.search.darts.operations import found_fc_apply, found_fc_route
    b, C, L = 6, 32, 8
    mods = _fc_ops(training)
    g = torch.Generator().manual_seed(3)
    x0, x1 = (torch.randn(b, C, L, generator=g).relu().to(dev()).requires_grad_(True) for _ in range(2))
    ws = [torch.randn(b, C, L, generator=g).to(dev()) for _ in range(3)]
    srcs = [x0, x1, x0]
    assert found_fc_route(mods, srcs) == 'fc'
    state = [{k: v.clone() for k, v in m.state_dict().items()} for m in mods]
    outs = found_fc_apply(mods, srcs)
    assert len(outs) == 3 and outs[0].grad_fn is outs[2].grad_fn
    assert tuple(outs[0].grad_fn.fc_U.shape) == (3, b, C, L)
    d0, d1 = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, ws)), [x0, x1])
    parts = []
    for e in range(3):
        mods[e].load_state_dict(state[e])                      # (the running statistics moved in training mode)
        (o,) = found_fc_apply([mods[e]], [srcs[e]])
        parts.append(torch.autograd.grad((o * ws[e]).sum(), srcs[e])[0])
        assert_close_scaled(f'out[{e}]', o, outs[e], rel=1e-5)
    assert_close_scaled('dx0', d0, parts[0] + parts[2], rel=2e-4)
    assert_close_scaled('dx1', d1, parts[1], rel=2e-4)
    assert float((parts[0] - parts[2]).abs().max()) > 1e-3 * float(d0.abs().max())


def test_source_without_requires_grad_and_no_grad_forward():
    meta, z, cfg, g, params, xs = fixture('fcfound_a_m_train_nodrop')
    net = fu.build_mirror(cfg, g, params, meta['mode'], dev())
    feat, xd = run(net, xs, meta['seed'])
    full = {k: v.grad.clone() for k, v in net.named_parameters() if v.grad is not None}
    # input 0 (read by two FC edges) and input 2 without a gradient
    net2 = fu.build_mirror(cfg, g, params, meta['mode'], dev())
    feat2, xd2 = run(net2, xs, meta['seed'], need=[False, True, False])
    assert xd2[0].grad is None and xd2[2].grad is None
    assert_close_scaled('feat', feat2, feat, rel=1e-6)
    assert_close_scaled('grad:input.1', xd2[1].grad, xd[1].grad, rel=1e-5)
    for k, v in net2.named_parameters():
        if k in full:
            assert_close_scaled('grad:' + k, v.grad, full[k], rel=1e-5)
    # no input needs a gradient at all: no data-gradient tile, the parameters' gradients are what they were
    net3 = fu.build_mirror(cfg, g, params, meta['mode'], dev())
    run(net3, xs, meta['seed'], need=[False] * cfg.N)
    for k, v in net3.named_parameters():
        if k in full:
            assert_close_scaled('grad:' + k, v.grad, full[k], rel=1e-5)
    # torch.no_grad(): forward only, same output, buffers updated as in any training forward
    net4 = fu.build_mirror(cfg, g, params, meta['mode'], dev())
    before = fc_launches()
    feat4, _ = run(net4, xs, meta['seed'], grads=False)
    assert fc_launches() - before == 1 + 2 + 1 and feat4.grad_fn is None
    assert_close_scaled('feat', feat4, z['feat'])
    for (k, a), (_, b) in zip(net4.state_dict().items(), net.state_dict().items()):
        if fo.is_buffer(k):
            assert_close_scaled('buf:' + k, a.float(), b.float(), rel=1e-6)


def test_num_batches_tracked_advances_by_one_per_training_forward():
    meta, z, cfg, g, params, xs = fixture('fcfound_d_s_train_nodrop')
    net = fu.build_mirror(cfg, g, params, 'train_nodrop', dev())
    fcs = [op for op in net.cell._ops if hasattr(op, 'bn')]
    assert len(fcs) == 2
    for n in (1, 2, 3):
        run(net, xs, meta['seed'], grads=n != 2)
        assert [int(op.bn.num_batches_tracked) for op in fcs] == [n, n]
    net.eval()
    run(net, xs, meta['seed'], grads=False)
    assert [int(op.bn.num_batches_tracked) for op in fcs] == [3, 3]


@pytest.mark.parametrize('name', ['fcfound_a_s_train_nodrop', 'fcfound_c_s_train_nodrop', 'fcfound_d_s_train_nodrop',
                                  'fcfound_a_n_train_nodrop'])
def test_live_dropout_under_exported_masks(name):
    """Train mode, every dropout live.  The recorded sites: one per FC edge of group 0 in genotype order, then per step
    a late FC edge's and the step node's.  The exported masks, permuted into the reference's execution order (step i's
    edge sites, then step i's node sites), are injected into the restatement."""
    from bmnas import lib
    meta, z, cfg0, g, params, xs = fixture(name)
    cfg = fo.Cfg({**cfg0, 'drpt': 0.15})
    net = fu.build_mirror(cfg, g, params, 'train', dev())
    with recorded_sites() as rec:
        feat, xd = run(net, xs, meta['seed'])
    b = meta['batch']
    names, idx = zip(*g.edges)
    group0 = [e for e in range(len(names)) if names[e] in fu.FC and idx[e] < cfg.N]
    late = [e for e in range(len(names)) if names[e] in fu.FC and idx[e] >= cfg.N]
    node_sites = [fu.node_live_sites(s, cfg) for s in g.steps]
    assert len(rec) == len(group0) + len(late) + sum(node_sites), (len(rec), group0, late, node_sites)
    assert all(n == b * cfg.C * cfg.L and d.thr == rec[0][0].thr for d, n in rec[:len(group0)])
    offs = [d.offset for d, _ in rec]
    assert offs == sorted(offs) and len(set(offs)) == len(offs)              # issued in this order, no site twice
    masks = [lib.dropout_mask(d, n, dev()).cpu() for d, n in rec]
    assert 0.05 < float((masks[0] == 0).float().mean()) < 0.3
    order = fu.reference_site_order(g, cfg)(node_sites)
    if name.startswith('fcfound_a_'):
        assert order[:2] == [0, 1] and order[2 + node_sites[0]:4 + node_sites[0]] == [2, 3]
        assert (order != sorted(order)) == (node_sites[0] > 0)
    want_feat, want, after, _ = fu.restate(cfg, g, params, xs, 'train', meta['seed'], [masks[i] for i in order])
    assert_close_scaled('feat', feat, want_feat)
    for i, x in enumerate(xd):
        assert_close_scaled(f'grad:input.{i}', x.grad, want[f'grad:input.{i}'], rel=2e-4)
    zero = fu.roundoff_zero_gradients(cfg, g, params, xs, 'train', meta['seed'], [masks[i] for i in order])
    for k, v in net.named_parameters():
        got = v.grad if v.grad is not None else torch.zeros_like(v)
        fu.assert_gradient('grad:' + k, got, want['grad:' + k], zero, 'train', assert_close_scaled)
    for k, v in net.state_dict().items():
        if fo.is_buffer(k):
            assert_close_scaled('buf:' + k, v.float(), after[k].float())


def _is_foreign(name):
    return 'at::' in name or 'Memcpy' in name or 'Memset' in name or 'rocclr' in name


FC_KERNELS = ('fc_gemm_fwd_k', 'fc_sep_fwd_k', 'fc_sep_bwd_reduce_k', 'fc_sep_bwd_du_k', 'fc_bwd_gemm_k')


def _short(name):
    return next((s for s in FC_KERNELS + ('prologue',) if s in name), name)


def test_function_runs_only_library_kernels():
    """torch.profiler over forward + backward of the Function alone, genotype (a)'s four edges (both kinds, input 0 read
    twice) at (C, L, b) = (32, 16, 5) in training mode with dropout live: every device event is one of
    libbmnas_hip.so's — no aten kernel, no memcpy, no memset — and the launches are exactly the budget: zero-fill, one
    GEMM per kind, apply; zero-fill, reductions, dU, GEMMs."""
    from models.search.darts.operations import found_fc_apply
    b, C, L = 5, 32, 16
    mods = _fc_ops(True, ('FC_Relu', 'FC_Mish', 'FC_Mish', 'FC_Relu'), C, L)
    for m in mods:
        m.dropout.p = 0.1
    gen = torch.Generator().manual_seed(4)
    xs = [torch.randn(b, C, L, generator=gen).relu().to(dev()).requires_grad_(True) for _ in range(3)]
    ws = [torch.randn(b, C, L, generator=gen).to(dev()) for _ in range(4)]
    leaves = xs + [p for m in mods for p in m.parameters()]

    def go():
        outs = found_fc_apply(mods, [xs[0], xs[0], xs[1], xs[2]])
        return torch.autograd.grad(outs, leaves, ws)
    assert all(g is not None for g in go())
    torch.cuda.synchronize()
    names = device_kernels(go)
    foreign = [k for k in names if _is_foreign(k) or _short(k) == k]
    assert not foreign, foreign
    assert [_short(k) for k in names] == ['prologue', 'fc_gemm_fwd_k', 'fc_gemm_fwd_k', 'fc_sep_fwd_k', 'prologue',
                                          'fc_sep_bwd_reduce_k', 'fc_sep_bwd_du_k', 'fc_bwd_gemm_k'], names


def test_device_events_of_the_fc_part():
    """Forward + backward of the whole network at (C, L, b) = (32, 16, 5), genotype (a) — both kinds, every cell input
    feeds FC edges only — in training mode with dropout live.  The FC part is exactly zero-fill, GEMM per kind, apply in
    front of everything else, and zero-fill, reductions, dU, GEMMs behind everything else: no foreign event in or
    between them, no autograd add behind them.  (The step nodes between the two parts are the ones every found network
    has; in an eager pass theirs include the fills of the BatchNorm pools and the add of a Sum node's residual.)  The
    device sees strictly fewer events than with the edges composed."""
    meta, z, cfg0, g, params, xs = fixture('fcfound_a_m_train_nodrop')
    cfg = fo.Cfg({**cfg0, 'drpt': 0.1})
    cot = fu.cotangent(meta['seed'], (meta['batch'], cfg.M * cfg.C * cfg.L)).to(dev())

    def runner(net):
        xd = [x.to(dev()).requires_grad_(True) for x in xs]
        leaves = xd + [p for p in net.parameters()]

        def go():
            return torch.autograd.grad(net(xd), leaves, cot, allow_unused=True)
        go()
        torch.cuda.synchronize()
        return go
    native = device_kernels(runner(fu.build_mirror(cfg, g, params, 'train', dev())))
    with forced_composed():
        composed = device_kernels(runner(fu.build_mirror(cfg, g, params, 'train', dev())))
    short = [_short(k) for k in native]
    print(f'found net, genotype (a) at C32 L16 b5: native {len(native)} device events, composed {len(composed)}')
    assert short[:4] == ['prologue', 'fc_gemm_fwd_k', 'fc_gemm_fwd_k', 'fc_sep_fwd_k'], short
    assert short[-4:] == ['prologue', 'fc_sep_bwd_reduce_k', 'fc_sep_bwd_du_k', 'fc_bwd_gemm_k'], short
    assert [short.count(k) for k in FC_KERNELS] == [2, 1, 1, 1, 1], short
    assert not any(s in k for k in composed for s in FC_KERNELS)
    # the rest of the network is the same in both runs: the FC edges are 8 events here, 8 + (what composing adds) there
    assert len(native) < len(composed), (len(native), len(composed))


class _Step(torch.nn.Module):
    def __init__(self, net, cls):
        super().__init__()
        self.net, self.cls = net, cls

    def forward(self, xs):
        return self.cls(self.net(list(xs)))


def test_captured_step_replays_with_fresh_masks_and_matches_eager():
    """bmnas.graph.GraphedTrainStep over a found network with FC edges (forward, criterion, backward, Adam as one
    replay), live dropout.  Replay 1 against an eager twin that draws the SAME masks (its host-side Philox offset is set
    to the step-counter value the replay's sites read), gradient by gradient; replay 2 draws other masks."""
    from bmnas import cell as K
    from bmnas import lib
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    meta, z, cfg0, g, params, xs = fixture('fcfound_a_m_train_nodrop')
    cfg = fo.Cfg({**cfg0, 'drpt': 0.1})
    nout, batch, seed = 7, meta['batch'], meta['seed']
    crit = bnn.CrossEntropyLoss()
    xs = [x.to(dev()) for x in xs]
    y = synth.make_labels('ce', batch, nout, seed).to(dev())

    def model():
        cls = bnn.Linear(cfg.M * cfg.C * cfg.L, nout)
        cw, cb = synth.make_classifier(cfg, nout, seed)
        cls.weight.data.copy_(cw)
        cls.bias.data.copy_(cb)
        return _Step(fu.build_mirror(cfg, g, params, 'train', dev()), cls.to(dev())).train()
    models = [model() for _ in range(2)]
    opts = [Adam(list(m.parameters()), lr=1e-3, weight_decay=1e-4) for m in models]
    with recorded_sites() as rec:
        gr = GraphedTrainStep(models[0], crit, opts[0], xs, y)
    rec = [r for r in rec if r[0].step]                  # the captured step's sites (warm-up passes are eager)
    assert len(rec) == 4 + sum(fu.node_live_sites(s, cfg) for s in g.steps)
    assert rec[0][1] == batch * cfg.C * cfg.L and rec[0][0].offset == 0
    loss1 = float(gr(xs, y)[0])
    torch.cuda.synchronize()
    step1 = gr._g.site_step_value()
    grads1 = {k: v.grad.detach().clone() for k, v in models[0].named_parameters() if v.grad is not None}
    masks1 = lib.dropout_mask(rec[0][0], rec[0][1], dev(), step1).cpu()
    assert 0.03 < float((masks1 == 0).float().mean()) < 0.2
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
    assert seen == 4
    loss2 = float(gr(xs, y)[0])
    torch.cuda.synchronize()
    step2 = gr._g.site_step_value()
    masks2 = lib.dropout_mask(rec[0][0], rec[0][1], dev(), step2).cpu()
    assert step2 != step1 and not torch.equal(masks1, masks2)
    assert np.isfinite(loss2) and loss2 != loss1
