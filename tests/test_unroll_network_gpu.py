"""-m gpu: DARTS' unrolled architecture step through the drivers — models.search._common.search_setup with args.unrolled on the
small MM-IMDB hypernet of tests/helpers/dp_child.py (fusion cell + classifier, C = 32, batch 8, dropout an identity) —
against the same algorithm written over oracle.fusion_oracle.search_step in float64 on the CPU: the virtual step, the
validation gradients at w', the +-R finite difference with the same r = 1e-2, and the combine; BatchNorm buffers cloned
per pass.  Train batch from seed SEED, validation batch from SEED + 1.

The weight optimizer is bmnas.optim.SGD (momentum 0.9, weight_decay 1e-4, lr 1e-2) after one real weight step, so that
the momentum buffers exist and enter the virtual step; the run is repeated with the default bmnas.optim.Adam, whose state
plays no part (the plain step).  The reference starts from the GPU's state after that weight step — weights, BatchNorm
buffers and momentum buffers read back and widened to float64 —: the weight step is not what is tested here.

alpha.grad, captured in front of optimizer.step(), is held to the project's gradient tolerance, assert_close_scaled(rel =
2e-4).  That tolerance is neither vacuous nor too tight at eta = 1e-2 (measured on the CPU in this configuration, without
momentum buffers or with random ones scaled to max|g|): an fp32 CPU run of the reference algorithm sits 0.12-0.23 x the
tolerance from the float64 run (the implicit term alone: 1.5e-3 relative), while the second-order term eta * ig is >= 10 x
the tolerance on 24 of the 42 alpha entries (largest about 200 x) — the first-order dalpha cannot pass.  At eta = 1e-3 only
4 entries clear 10 x; at eta = 1e-1 the fp32 CPU run itself exceeds the tolerance (1.7-2.3 x).  The test recomputes the
second figure in float64 and asserts >= 10 entries at >= 10 x; it prints the GPU's worst error over tolerance."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn as nn

from gpu_util import assert_close_scaled, dev, scale_tol, set_mode

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))

GRAD_REL = 2e-4
ETA, R0 = 1e-2, 1e-2


def _build(mode='train_nodrop', **extra):
    """tests/test_sgd_loop_gpu.py's recipe: dp_child's hypernet through search_setup, single process
    -> model, criterion, weight optimizer, architect, args"""
    import dp_child as base
    from oracle import synth
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase, search_setup
    cfg = base.cfg_small()
    args = base.make_args(cfg)
    args.use_dataparallel = False
    for k, v in extra.items():
        setattr(args, k, v)

    class Net(HyperNetBase):
        def __init__(self, criterion):
            super().__init__()
            self._build_head(args, criterion, nn.ModuleList([nn.Identity() for _ in range(cfg.N)]), cfg.N, 2)

        def forward(self, feats):
            return self.fuse(feats)

    crit = bnn.BCEWithLogitsLoss()
    model = Net(crit)
    model.fusion_net.load_state_dict(synth.make_params(cfg, base.SEED))
    for dst, src in zip(model.arch_parameters(), synth.make_arch(cfg, base.SEED, 0.5)):
        dst.data.copy_(src)
    cw, cb = synth.make_classifier(cfg, base.NOUT, base.SEED)
    model.central_classifier.weight.data.copy_(cw)
    model.central_classifier.bias.data.copy_(cb)
    optimizer, _, architect, _ = search_setup(model, args, crit, dev(), 1.0, args.weight_decay)
    set_mode(model, mode)
    return model, crit, optimizer, architect, args


def _batch(seed, device=None):
    import dp_child as base
    from oracle import synth
    cfg = base.cfg_small()
    xs = synth.make_inputs(cfg, base.GLOBAL_BATCH, seed)
    y = synth.make_labels('bce', base.GLOBAL_BATCH, base.NOUT, seed)
    if device is not None:
        xs, y = [x.to(device) for x in xs], y.to(device)
    return xs, y


def _weight_names(model):
    """name (the oracle's keys) -> parameter, for every tensor of the weight optimizer"""
    out = {k: v for k, v in model.fusion_net.named_parameters()}
    out['central_classifier.weight'] = model.central_classifier.weight
    out['central_classifier.bias'] = model.central_classifier.bias
    return out


def _reference(model, optimizer, eta, r):
    """The unrolled step in float64 over the oracle, from the model's CURRENT state
    -> (alpha.grad per arch tensor, eta * ig per arch tensor)"""
    import dp_child as base
    from oracle import fusion_oracle as fo
    cfg = base.cfg_small()
    f64 = lambda t: t.detach().cpu().double() if t.is_floating_point() else t.detach().cpu().clone()
    state = {k: f64(v) for k, v in model.fusion_net.state_dict().items()}
    names = _weight_names(model)
    W = {k: f64(p) for k, p in names.items()}
    arch = [f64(a) for a in model.arch_parameters()]
    group_of = {id(p): g for g in optimizer.param_groups for p in g['params']}
    train = _batch(base.SEED)
    valid = _batch(base.SEED + 1)

    def grads_at(Wx, batch):
        p = {k: (v.clone() if fo.is_buffer(k) else Wx[k]) for k, v in state.items()}       # buffers cloned per pass
        xs, y = batch
        _, _, g = fo.search_step([x.double() for x in xs], y, arch, p, Wx['central_classifier.weight'],
                                 Wx['central_classifier.bias'], cfg, 'bce', training=True, attn_drop=0.0)
        return g

    g = grads_at(W, train)
    W1 = {}
    for k, p in names.items():
        grp = group_of[id(p)]
        d = g[k] + grp['weight_decay'] * W[k]
        buf = optimizer.state.get(p, {}).get('momentum_buffer')
        if buf is not None:
            d = f64(buf) * grp['momentum'] + d
        W1[k] = W[k] - eta * d
    gv = grads_at(W1, valid)
    dalpha = [gv[f'arch.{i}'] for i in range(len(arch))]
    v = {k: gv[k] for k in names}
    R = r / float(torch.sqrt(sum((t ** 2).sum() for t in v.values())))
    gp = grads_at({k: W[k] + R * v[k] for k in names}, train)
    gn = grads_at({k: W[k] - R * v[k] for k in names}, train)
    second = [eta * (gp[f'arch.{i}'] - gn[f'arch.{i}']) / (2 * R) for i in range(len(arch))]
    return [d - s for d, s in zip(dalpha, second)], second


def _one_weight_step(model, crit, optimizer, xs, y):
    optimizer.zero_grad()
    crit(model(xs), y).backward()
    optimizer.step()
    optimizer.zero_grad()
    torch.cuda.synchronize()


def _state_tensors(optimizer):
    return [(k, t) for p, st in optimizer.state.items() for k, t in st.items() if torch.is_tensor(t)]


def _nbt(model):
    return [int(v) for k, v in model.state_dict().items() if k.endswith('num_batches_tracked')]


@pytest.mark.parametrize('kind', ['sgd', 'adam'])
def test_unrolled_step_matches_the_float64_algorithm(monkeypatch, kind):
    import dp_child as base
    from bmnas.optim import SGD, Adam
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    extra = dict(optimizer='sgd', momentum=0.9) if kind == 'sgd' else {}
    model, crit, opt, architect, args = _build(unrolled=True, eta_max=ETA, weight_decay=1e-4, **extra)
    assert type(opt) is (SGD if kind == 'sgd' else Adam) and architect.unrolled and architect.network_optimizer is opt
    assert all(g['lr'] == ETA and g['weight_decay'] == 1e-4 for g in opt.param_groups)
    xt, yt = _batch(base.SEED, dev())
    xv, yv = _batch(base.SEED + 1, dev())
    # one real weight step: the momentum buffers (Adam: the moments and step counts) exist.  Adam's first step moves every
    # element by its whole learning rate, whatever the gradient: at 1e-2 that is another model (eta * ig then clears 10 x
    # the tolerance on 2 entries only), so ITS weight step runs at 1e-5 and the rate is put back for the architecture step
    for g in opt.param_groups:
        g['lr'] = ETA if kind == 'sgd' else 1e-5
    _one_weight_step(model, crit, opt, xt, yt)
    for g in opt.param_groups:
        g['lr'] = ETA
    names = _weight_names(model)
    if kind == 'sgd':
        assert all(torch.is_tensor(opt.state[p].get('momentum_buffer')) for p in names.values())
    want, second = _reference(model, opt, ETA, R0)

    # the comparison below cannot pass vacuously: the second-order term, in float64, against the tolerance
    far, most = 0, 0.0
    for w, s in zip(want, second):
        w, s = w.numpy(), s.numpy()
        tol = GRAD_REL * np.abs(w) + scale_tol(w, GRAD_REL)        # assert_close_scaled's
        far += int((np.abs(s) >= 10 * tol).sum())
        most = max(most, float((np.abs(s) / tol).max()))
    total = sum(w.numel() for w in want)
    print(f'{kind}: eta * ig >= 10 x tolerance on {far} of {total} alpha entries (largest {most:.0f} x)')
    assert far >= 10

    w_list = [p for p in model.parameters() if not any(p is a for a in model.arch_parameters())]
    w_before = [p.detach().clone() for p in w_list]
    st_before = [(k, t.clone()) for k, t in _state_tensors(opt)]
    a_before = [a.detach().clone() for a in model.arch_parameters()]
    nbt0 = _nbt(model)
    seen = []
    step = architect.optimizer.step

    def recording_step(*a, **k):
        seen.append([None if p.grad is None else p.grad.detach().clone() for p in model.arch_parameters()])
        return step(*a, **k)

    monkeypatch.setattr(architect.optimizer, 'step', recording_step)
    assert architect.step(xv, yv, None, input_train=xt, target_train=yt) is None
    torch.cuda.synchronize()
    assert len(seen) == 1 and architect.unrolled_steps == 1 and architect.graph_replays == 0
    got = seen[0]
    worst = 0.0
    for g_, w in zip(got, want):
        w_ = w.numpy()
        tol = GRAD_REL * np.abs(w_) + scale_tol(w_, GRAD_REL)
        worst = max(worst, float((np.abs(g_.cpu().double().numpy() - w_) / tol).max()))
    print(f'{kind}: worst |alpha.grad - float64| / tolerance on the GPU: {worst:.3f}')
    for i, (g_, w) in enumerate(zip(got, want)):
        assert_close_scaled(f'{kind} alpha.grad {i}', g_, w, rel=GRAD_REL)

    # the weights are back bit for bit, no `.grad` of a weight was written, the weight optimizer's state was only read
    assert all(torch.equal(p, q) for p, q in zip(w_list, w_before))
    assert all(p.grad is None for p in w_list)
    st_after = _state_tensors(opt)
    assert len(st_after) == len(st_before) > 0
    assert all(k == k2 and torch.equal(t, t2) for (k, t), (k2, t2) in zip(st_after, st_before))
    # four passes on the live model
    assert _nbt(model) == [n + 4 for n in nbt0] and len(nbt0) > 0
    # alpha: an eager bmnas.optim.Adam step on that dalpha, on a twin
    twin = [a.clone().requires_grad_(True) for a in a_before]
    g0 = architect.optimizer.param_groups[0]
    twin_opt = Adam(twin, lr=g0['lr'], betas=g0['betas'], eps=g0['eps'], weight_decay=g0['weight_decay'])
    for t, g_ in zip(twin, got):
        t.grad = g_
    twin_opt.step()
    torch.cuda.synchronize()
    for a, t, a0 in zip(model.arch_parameters(), twin, a_before):
        assert torch.equal(a.detach(), t.detach()) and not torch.equal(a.detach(), a0)

    # a second step synchronises nothing with the host
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        architect.step(xv, yv, None, input_train=xt, target_train=yt)
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    torch.cuda.synchronize()
    assert architect.unrolled_steps == 2 and len(seen) == 2
    assert all(torch.equal(p, q) for p, q in zip(w_list, w_before))
    assert all(bool(torch.isfinite(g_).all()) for g_ in seen[1])


def test_plus_and_minus_passes_share_their_dropout_masks(monkeypatch):
    """Live dropout (drpt 0.1, train mode): the sites the + pass and the - pass issue have pairwise equal
    (seed, offset, thr) — the same masks —, and the next step's sites repeat none of them."""
    import dp_child as base
    from bmnas import cell as K
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    model, crit, opt, architect, args = _build(mode='train', unrolled=True, eta_max=ETA, drpt=0.1)
    xt, yt = _batch(base.SEED, dev())
    xv, yv = _batch(base.SEED + 1, dev())
    site = lambda rec: [(d.seed, d.offset, d.thr) for d, _ in rec]
    steps = []
    try:
        for _ in range(2):
            K.DROP.record = []
            architect.step(xv, yv, None, input_train=xt, target_train=yt)
            steps.append(site(K.DROP.record))
    finally:
        K.DROP.record = None
    torch.cuda.synchronize()
    for rec in steps:
        assert len(rec) > 0 and len(rec) % 4 == 0                    # four passes over the same sites
        n = len(rec) // 4
        virt, val, plus, minus = rec[:n], rec[n:2 * n], rec[2 * n:3 * n], rec[3 * n:]
        assert plus == minus
        assert len({o for _, o, _ in virt + val + plus}) == 3 * n    # ... and no other pass shares a site's offset
    assert not {o for _, o, _ in steps[0]} & {o for _, o, _ in steps[1]}
    assert min(o for _, o, _ in steps[1]) > max(o for _, o, _ in steps[0])
    assert all(bool(torch.isfinite(a).all()) for a in model.arch_parameters())
