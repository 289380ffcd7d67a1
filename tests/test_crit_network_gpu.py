"""-m gpu: class-weighted / label-smoothed criteria (bmnas.nn.BCEWithLogitsLoss, CrossEntropyLoss with weight,
pos_weight, label_smoothing, ignore_index, reduction='sum') on whole networks: eager on the kernels of csrc/linear.hip,
deferred into the head's backward launch (csrc/head.hip) of a search cell and of a found network, captured as a
hipGraph with the weight tensors read by address, and under bmnas.cell.DETERMINISTIC."""
import warnings

import pytest
import torch

import crit_ref
from oracle import fusion_oracle as fo
from oracle import synth
from fc_edges_util import device_kernels
from gpu_util import assert_close_scaled, build_found_net, build_search_net, dev

pytestmark = pytest.mark.gpu

SEED = 31
SMALL_PLAIN = dict(N=3, C=32, L=16, S=2, M=2, ns=2, nm=2, drpt=0.0)      # the head's plain backward (bmnas_head_bwd_crit)
SMALL_LAZY = dict(N=3, C=64, L=16, S=2, M=2, ns=1, nm=1, drpt=0.0)       # node_multiplier 1: bmnas_head_bwd_lazy_crit


class _Step(torch.nn.Module):
    """fusion_net -> central_classifier, wired like the reference's hypernets minus backbones and reshape layers."""

    def __init__(self, net, cls):
        super().__init__()
        self.fusion_net, self.central_classifier = net, cls

    def arch_parameters(self):
        return self.fusion_net.arch_parameters() if hasattr(self.fusion_net, 'arch_parameters') else []

    def forward(self, xs):
        return self.fusion_net.forward_classified(list(xs), self.central_classifier)


def _model(cfg, nout, found=False, seed=SEED):
    from bmnas import nn as bnn
    if found:
        net = build_found_net(cfg, fo.network_genotype(synth.make_arch(cfg, seed), cfg), seed, 'train_nodrop')
    else:
        net = build_search_net(cfg, seed, 'train_nodrop')
    cls = bnn.Linear(cfg.M * cfg.C * cfg.L, nout)
    cw, cb = synth.make_classifier(cfg, nout, seed)
    cls.weight.data.copy_(cw)
    cls.bias.data.copy_(cb)
    return _Step(net, cls.to(dev())).train()


def _vec(n, seed):
    return (0.25 + 2.0 * torch.rand(n, generator=torch.Generator().manual_seed(seed))).to(dev())


def _criterion(kind, nout):
    """-> criterion, the labels' loss kind, ignore_index"""
    from bmnas import nn as bnn
    if kind == 'bce':
        return bnn.BCEWithLogitsLoss(weight=_vec(nout, 1), pos_weight=_vec(nout, 2)).to(dev()), 'bce', None
    if kind == 'bce_sum':
        return bnn.BCEWithLogitsLoss(pos_weight=_vec(nout, 2), reduction='sum').to(dev()), 'bce', None
    return bnn.CrossEntropyLoss(weight=_vec(nout, 3), label_smoothing=0.1, ignore_index=2).to(dev()), 'ce', 2


def _batch(cfg, batch, nout, loss_kind, ign, seed=SEED):
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, batch, seed)]
    y = synth.make_labels(loss_kind, batch, nout, seed)
    if ign is not None:
        y[1] = ign                                                # at least one ignored row
    return xs, y.to(dev())


def _grads(model, xs):
    out = {'p.' + k: v.grad for k, v in model.named_parameters() if v.grad is not None}
    for i, x in enumerate(xs):
        if x.grad is not None:
            out[f'input.{i}'] = x.grad
    for i, a in enumerate(model.arch_parameters()):
        if a.grad is not None:
            out[f'arch.{i}'] = a.grad
    return out


def _same_grads(got, want, label):
    assert set(got) == set(want), (label, set(got) ^ set(want))
    seen = 0
    for k in want:
        if k.endswith('conv.bias'):
            assert float(got[k].abs().max()) < 1e-4, k            # mathematically zero (BatchNorm removes the mean)
        else:
            assert_close_scaled(f'{label} {k}', got[k], want[k], rel=2e-4)
            seen += 1
    assert seen > 4


def test_weighted_criteria_run_on_the_kernels_not_on_torch():
    """No off-path warning (an error here), and torch's own numbers on the CPU in float64."""
    from bmnas import lib
    from bmnas import nn as bnn
    g = torch.Generator().manual_seed(3)
    z = (2.0 * torch.randn(37, 23, generator=g)).to(dev()).requires_grad_(True)
    y = (torch.rand(37, 23, generator=g) < 0.3).float().to(dev())
    zc = (2.0 * torch.randn(64, 60, generator=g)).to(dev()).requires_grad_(True)
    yc = torch.randint(0, 60, (64,), generator=g).to(dev())
    yc[::5] = 7
    w23, p23, w60 = _vec(23, 1), _vec(23, 2), _vec(60, 3)
    lib._NOTED.clear()
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        cases = [(bnn.BCEWithLogitsLoss(pos_weight=p23), z, y, 'BCEWithLogitsCritFnBackward'),
                 (bnn.BCEWithLogitsLoss(weight=w23, pos_weight=p23, reduction='sum'), z, y, 'BCEWithLogitsCritFnBackward'),
                 (bnn.CrossEntropyLoss(weight=w60, label_smoothing=0.1, ignore_index=7), zc, yc, 'CrossEntropyCritFnBackward'),
                 (bnn.CrossEntropyLoss(reduction='sum', ignore_index=7), zc, yc, 'CrossEntropyCritFnBackward'),
                 (bnn.BCEWithLogitsLoss(), z, y, 'BCEWithLogitsFnBackward'),                   # the bare forms: as before
                 (bnn.CrossEntropyLoss(), zc, yc, 'CrossEntropyFnBackward')]
        for crit, zz, yy, fn in cases:
            assert bnn.criterion_route(crit, zz, yy) == 'native'
            zz.grad = None
            loss = crit(zz, yy)
            assert type(loss.grad_fn).__name__ == fn
            loss.backward()
            if isinstance(crit, bnn.BCEWithLogitsLoss):
                want, dwant = crit_ref.bce(zz, yy, crit.weight, crit.pos_weight, crit.reduction)
            else:
                want, dwant = crit_ref.ce(zz, yy, crit.weight, crit.label_smoothing, crit.ignore_index, crit.reduction)
            assert_close_scaled('loss', loss.reshape(1), want.reshape(1))
            assert_close_scaled('dz', zz.grad, dwant)
    # what stays with torch still says so
    with pytest.warns(RuntimeWarning, match='stock torch ops'):
        bnn.BCEWithLogitsLoss(reduction='none')(z, y)


@pytest.mark.parametrize('shape,found,kind', [(SMALL_PLAIN, False, 'bce'), (SMALL_LAZY, False, 'ce'),
                                              (SMALL_LAZY, False, 'bce_sum'), (SMALL_PLAIN, True, 'ce'),
                                              (SMALL_PLAIN, True, 'bce')])
def test_deferred_weighted_criterion_equals_the_eager_one(shape, found, kind):
    """The criterion evaluated by the head's backward launch against the same criterion as a launch of its own (which
    materialises dlogits): the loss and every gradient."""
    from bmnas import cell as K
    from bmnas import nn as bnn
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg, batch, nout = fo.make_cfg(**shape), 17, 23
    crit, loss_kind, ign = _criterion(kind, nout)
    res = []
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        for deferred in (True, False):
            model = _model(cfg, nout, found)
            xs, y = _batch(cfg, batch, nout, loss_kind, ign)
            xs = [x.requires_grad_(True) for x in xs]
            with bnn.fused_criterion(deferred):
                logits = model(xs)
                assert getattr(logits, '_bmnas_head', None) is not None
                loss = crit(logits, y)
            want_fn = 'DeferredLossFnBackward' if deferred else \
                ('CrossEntropyCritFnBackward' if loss_kind == 'ce' else 'BCEWithLogitsCritFnBackward')
            assert type(loss.grad_fn).__name__ == want_fn
            loss.backward()
            torch.cuda.synchronize()
            res.append((float(loss.detach()), logits.detach(), _grads(model, xs)))
    (l_d, z_d, g_d), (l_e, z_e, g_e) = res
    if loss_kind == 'bce':
        want, _ = crit_ref.bce(z_e, y, crit.weight, crit.pos_weight, crit.reduction)
    else:
        want, _ = crit_ref.ce(z_e, y, crit.weight, crit.label_smoothing, crit.ignore_index, crit.reduction)
    assert_close_scaled('eager loss', torch.tensor([l_e]), want.reshape(1))
    assert_close_scaled('deferred loss', torch.tensor([l_d]), want.reshape(1))
    _same_grads(g_d, g_e, f'{kind} deferred vs eager')


def _captured_and_twin(cfg, batch, nout, kind, found):
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    crit, loss_kind, ign = _criterion(kind, nout)
    xs, y = _batch(cfg, batch, nout, loss_kind, ign)
    models = [_model(cfg, nout, found) for _ in range(2)]
    # lr = 0: the replays leave the parameters where the eager twin's are (the update itself is tests/test_optim_gpu.py's)
    opts = [Adam(list(m.parameters()), lr=0.0, weight_decay=1e-4) for m in models]
    step = GraphedTrainStep(models[0], crit, opts[0], xs, y)
    return crit, xs, y, models, opts, step


def _eager(model, opt, crit, xs, y):
    opt.zero_grad()
    loss = crit(model(xs), y)
    loss.backward()
    torch.cuda.synchronize()
    return float(loss), {'p.' + k: v.grad.detach().clone() for k, v in model.named_parameters() if v.grad is not None}


@pytest.mark.parametrize('shape,found,kind', [(SMALL_LAZY, False, 'bce'), (SMALL_LAZY, False, 'ce'),
                                              (SMALL_PLAIN, True, 'bce'), (SMALL_PLAIN, True, 'ce')])
def test_captured_step_matches_eager_and_follows_in_place_weight_edits(shape, found, kind):
    from bmnas import cell as K
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg, batch, nout = fo.make_cfg(**shape), 17, 23
    with warnings.catch_warnings():
        warnings.simplefilter('error', RuntimeWarning)
        crit, xs, y, models, opts, step = _captured_and_twin(cfg, batch, nout, kind, found)
        edited = crit.pos_weight if kind == 'bce' else crit.weight
        address = edited.data_ptr()
        losses = []
        for rnd in range(2):
            loss_g = float(step(xs, y)[0])
            torch.cuda.synchronize()
            grads_g = {'p.' + k: v.grad.detach().clone() for k, v in models[0].named_parameters() if v.grad is not None}
            loss_e, grads_e = _eager(models[1], opts[1], crit, xs, y)
            assert abs(loss_g - loss_e) <= 1e-4 * max(1.0, abs(loss_e)), (rnd, loss_g, loss_e)
            _same_grads(grads_g, grads_e, f'replay {rnd} vs eager')
            losses.append(loss_g)
            edited.mul_(torch.linspace(0.5, 4.0, nout, device=dev()))     # in place, between two replays
            assert edited.data_ptr() == address
    # the edit did move the loss, by ten times the bound the replay was held to against the eager twin (a replay that
    # still read the old weights could not have passed round 1); the weighted CE mean renormalises, so it moves less
    assert abs(losses[1] - losses[0]) > 1e-3 * abs(losses[0]), losses


@pytest.mark.parametrize('shape,found', [(SMALL_LAZY, False), (SMALL_PLAIN, True)], ids=['search', 'found'])
def test_weighted_captured_step_has_the_unweighted_step_launches(shape, found):
    """Same number of device events as the unweighted captured step, none of them an aten kernel: the criterion has no
    launch of its own and no dlogits tensor.  A search cell (the head's lazy backward) and a found network (FoundHeadFn,
    the plain backward), BCE and CE on each."""
    from bmnas import cell as K
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg, batch = fo.make_cfg(**shape), 17
    names = {}
    for label, nout, make in [('bce', 23, lambda: bnn.BCEWithLogitsLoss()),
                              ('bce weighted', 23, lambda: _criterion('bce', 23)[0]),
                              ('ce', 23, lambda: bnn.CrossEntropyLoss()),
                              ('ce weighted', 23, lambda: _criterion('ce', 23)[0])]:
        crit = make()
        loss_kind = 'bce' if 'bce' in label else 'ce'
        xs, y = _batch(cfg, batch, nout, loss_kind, None)
        model = _model(cfg, nout, found)
        step = GraphedTrainStep(model, crit, Adam(list(model.parameters()), lr=1e-3), xs, y)
        step(xs, y)
        torch.cuda.synchronize()
        names[label] = device_kernels(lambda: step(xs, y))
        assert torch.isfinite(step(xs, y)[0]).all()
        del step
    for kind in ('bce', 'ce'):
        plain, weighted = names[kind], names[kind + ' weighted']
        print(f'{kind}: {len(plain)} device events unweighted, {len(weighted)} weighted')
        assert len(weighted) == len(plain), (plain, weighted)
        assert not [n for n in weighted if 'at::native' in n]
        assert any('head_bwd_k' in n for n in weighted)


@pytest.fixture
def deterministic():
    from bmnas import cell as K
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0 (switch matrix): the deterministic mode covers the fused-head path only')
    prev = K.DETERMINISTIC
    K.DETERMINISTIC = True
    K.apply_deterministic()
    yield K
    K.DETERMINISTIC = prev
    K.apply_deterministic()


def test_deterministic_mode_with_pos_weight_is_bit_identical(deterministic):
    """Two MM-IMDB-configuration steps at b = 37 (a ragged last chunk) with pos_weight: the loss shares leave through
    loss_part, and every tensor of the step is bit-identical between the runs."""
    from bmnas import nn as bnn
    cfg, batch, nout = fo.Cfg({**fo.CONFIGS['mmimdb'], 'drpt': 0.0}), 37, 23
    runs = []
    for _ in range(2):
        model = _model(cfg, nout, seed=11)
        crit = bnn.BCEWithLogitsLoss(pos_weight=_vec(nout, 2))
        xs, y = _batch(cfg, batch, nout, 'bce', None, seed=11)
        xs = [x.requires_grad_(True) for x in xs]
        with bnn.fused_criterion():
            logits = model(xs)
            loss = crit(logits, y)
        assert type(loss.grad_fn).__name__ == 'DeferredLossFnBackward'
        loss.backward()
        torch.cuda.synchronize()
        out = {'logits': logits.detach().clone(), 'loss': loss.detach().clone()}
        out.update({k: v.clone() for k, v in _grads(model, xs).items()})
        for i, a in enumerate(model.arch_parameters()):
            out[f'arch.{i}'] = a.grad.clone()
        runs.append(out)
    a, b = runs
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, (len(diff), diff[:6])
    want, _ = crit_ref.bce(a['logits'], y, None, _vec(nout, 2), 'mean')
    assert_close_scaled('loss', a['loss'].reshape(1), want.reshape(1))
