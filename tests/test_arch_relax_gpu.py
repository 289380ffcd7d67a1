"""-m gpu: the temperature / Gumbel-softmax relaxation of the architecture tensors — the two launches of csrc/relax.hip
against the numpy restatement (tests/arch_relax_ref.py), the device counter eagerly and under hipGraph replay, the search
hypernet with a relaxation set against a twin whose RAW arch tensors hold the relaxed values, captured steps against
eager ones, and the default path (no relaxation: not one launch or bit different).

Bit comparisons of whole network steps run in deterministic mode (bmnas.cell.DETERMINISTIC) where that mode covers the
route — the fused cell under the fused head; the default mode sums its batch reductions with fp32 atomics and two runs
of ONE network already differ in their last bits (tests/test_deterministic_gpu.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import arch_relax_ref as ref
from gpu_util import Pool, assert_close_scaled, build_search_net, dev, set_mode
from oracle import fusion_oracle as fo
from oracle import synth

pytestmark = pytest.mark.gpu

TAUS = [1.0, 0.3, 5.0]
SEED = 0x1234ABCD5678EF01
SHAPES = {
    'one': [(1, 1)],
    'straddle': [(3, 3), (2, 2)],                                      # 13 elements: no multiple of 4
    'mixed': [(3, 2), (2, 3), (5, 4), (1, 7)],                         # cols 2 / 3 / 4 / 7 in one launch, 39 elements
    'n16': [(i % 3 + 1, (2, 3, 4, 7)[i % 4]) for i in range(16)],      # the most tensors of one launch
    'big': [(70, 4)],                                                  # 280 elements: more than the workgroup
}
STEPS = {'one': 0, 'straddle': 2, 'mixed': 7, 'n16': (1 << 32) + 3, 'big': 41}     # (n16: step << 32 wraps in 64 bits)


def _bits(t):
    a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(name, got, want):
    g, w = _bits(got), _bits(want)
    assert g.shape == w.shape, (name, g.shape, w.shape)
    if not np.array_equal(g, w):
        i = int(np.flatnonzero(g.reshape(-1) != w.reshape(-1))[0])
        raise AssertionError(f'{name}: bits differ at flat {i} of {g.size}: got '
                             f'{np.asarray(got.detach().cpu() if torch.is_tensor(got) else got).reshape(-1)[i]!r} want '
                             f'{np.asarray(want.detach().cpu() if torch.is_tensor(want) else want).reshape(-1)[i]!r}')


def _state(tau, seed=SEED, step=0):
    from bmnas.nn import ArchRelaxation
    r = ArchRelaxation(tau=tau, gumbel=True, seed=seed).to(dev())
    r.counter.fill_(step)
    return r


def _logits(shapes, salt=0):
    rng = np.random.Generator(np.random.PCG64(1000 + salt))
    return [torch.from_numpy(rng.standard_normal(s).astype(np.float32)).to(dev()) for s in shapes]


def _check_noise(name, noise, shapes, seed, step, e0=0):
    want = ref.noise64(shapes, seed, step, e0)
    worst = 0.0
    for t, (g, w) in enumerate(zip(noise, want)):
        g = g.detach().cpu().numpy().astype(np.float64)
        assert np.isfinite(g).all(), (name, t)
        err = np.abs(g - w) / np.maximum(1.0, np.abs(w))
        worst = max(worst, float(err.max()))
        assert (np.abs(g - w) <= ref.gumbel_bound(w)).all(), (name, t, float(err.max()), 8 * 2.0 ** -23)
    return worst


# ---- kernels against the reference -------------------------------------------------------------------------------------
@pytest.mark.parametrize('tau', TAUS)
@pytest.mark.parametrize('case', list(SHAPES))
def test_forward_and_backward_against_the_reference(case, tau):
    from bmnas import lib
    shapes, step = SHAPES[case], STEPS[case]
    r = _state(tau, step=step)
    a = _logits(shapes)
    pool = Pool()
    z = [pool.new(*s) for s in shapes]
    noise = [pool.new(*s) for s in shapes]
    before = dict(lib.RELAX_LAUNCHES)
    lib.arch_relax_fwd(a, z, noise, r.state, True, False)
    pool.check()
    assert lib.RELAX_LAUNCHES['fwd'] - before['fwd'] == 1
    assert int(r.counter) == step                                      # advance = 0
    worst = _check_noise(case, noise, shapes, SEED, step)
    print(f'{case} tau {tau}: max |G - G64| / max(1, |G64|) = {worst:.3e} (bound {8 * 2.0 ** -23:.3e})')
    a_np, g_np = [t.cpu().numpy() for t in a], [t.cpu().numpy() for t in noise]
    for t, (got, want) in enumerate(zip(z, ref.relax(a_np, g_np, tau))):
        _same_bits(f'{case} z[{t}]', got, want)
    # gumbel = 0: z = a / tau, no noise written, the counter is not read
    pool0 = Pool()
    z0 = [pool0.new(*s) for s in shapes]
    n0 = [pool0.new(*s) for s in shapes]
    lib.arch_relax_fwd(a, z0, n0, r.state, False, False)
    pool0.check()
    for t, (got, want) in enumerate(zip(z0, ref.relax(a_np, None, tau))):
        _same_bits(f'{case} z0[{t}]', got, want)
        assert bool(torch.isnan(n0[t]).all())
    # backward: da = dz / tau
    dz = _logits(shapes, salt=5)
    poolb = Pool()
    da = [poolb.new(*s) for s in shapes]
    lib.arch_relax_bwd(dz, da, r.state)
    poolb.check()
    assert lib.RELAX_LAUNCHES['bwd'] - before['bwd'] == 1
    for t, (got, want) in enumerate(zip(da, ref.relax_bwd([g.cpu().numpy() for g in dz], tau))):
        _same_bits(f'{case} da[{t}]', got, want)
    assert int(r.counter) == step


@pytest.mark.parametrize('tau', TAUS)
def test_two_launches_with_e0_give_the_bits_of_one(tau):
    from bmnas import lib
    shapes, step = SHAPES['mixed'], 9
    a = _logits(shapes)
    r = _state(tau, step=step)
    z1, n1 = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in a]
    lib.arch_relax_fwd(a, z1, n1, r.state, True, True)
    assert int(r.counter) == step + 1
    r.counter.fill_(step)
    z2, n2 = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in a]
    cut = 2
    e0 = sum(t.numel() for t in a[:cut])                               # 12: the second launch starts on a fresh counter ...
    lib.arch_relax_fwd(a[:cut], z2[:cut], n2[:cut], r.state, True, False, e0=0)
    assert int(r.counter) == step
    lib.arch_relax_fwd(a[cut:], z2[cut:], n2[cut:], r.state, True, True, e0=e0)
    assert int(r.counter) == step + 1
    for t in range(len(a)):
        _same_bits(f'noise[{t}]', n2[t], n1[t])
        _same_bits(f'z[{t}]', z2[t], z1[t])
    # ... and a cut inside a counter (after 6 elements: words 2, 3 of counter 1 belong to the second launch)
    r.counter.fill_(step)
    z3, n3 = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in a]
    lib.arch_relax_fwd(a[:1], z3[:1], n3[:1], r.state, True, False, e0=0)
    lib.arch_relax_fwd(a[1:], z3[1:], n3[1:], r.state, True, True, e0=6)
    for t in range(len(a)):
        _same_bits(f'noise3[{t}]', n3[t], n1[t])
        _same_bits(f'z3[{t}]', z3[t], z1[t])
    _check_noise('split', n3[1:], shapes[1:], SEED, step, e0=6)


def test_more_than_sixteen_tensors_are_several_launches_and_one_draw():
    from bmnas import lib
    shapes = [(i % 4 + 1, (2, 4, 3)[i % 3]) for i in range(20)]
    a = _logits(shapes)
    r = _state(0.3, step=4)
    z, n = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in a]
    before = dict(lib.RELAX_LAUNCHES)
    lib.arch_relax_fwd(a, z, n, r.state, True, True)
    assert lib.RELAX_LAUNCHES['fwd'] - before['fwd'] == 2
    assert int(r.counter) == 5                                         # advanced once, by the last launch
    _check_noise('twenty', n, shapes, SEED, 4)
    for t, (got, want) in enumerate(zip(z, ref.relax([x.cpu().numpy() for x in a], [g.cpu().numpy() for g in n], 0.3))):
        _same_bits(f'z[{t}]', got, want)
    dz = _logits(shapes, salt=3)
    da = [torch.empty_like(t) for t in dz]
    lib.arch_relax_bwd(dz, da, r.state)
    assert lib.RELAX_LAUNCHES['bwd'] - before['bwd'] == 2
    for t, (got, want) in enumerate(zip(da, ref.relax_bwd([g.cpu().numpy() for g in dz], 0.3))):
        _same_bits(f'da[{t}]', got, want)


# ---- the counter -------------------------------------------------------------------------------------------------------
def test_counter_moves_by_one_per_advancing_launch():
    from bmnas import lib
    shapes = SHAPES['big']
    a = _logits(shapes)
    r = _state(1.0, step=100)
    z, n = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in a]
    seen = []
    for i in range(3):
        lib.arch_relax_fwd(a, z, n, r.state, True, True)
        assert int(r.counter) == 101 + i
        seen.append(n[0].clone())
        _check_noise(f'launch {i}', n, shapes, SEED, 100 + i)
    assert not torch.equal(seen[0], seen[1]) and not torch.equal(seen[1], seen[2])
    lib.arch_relax_fwd(a, z, n, r.state, True, False)                  # advance = 0
    lib.arch_relax_fwd(a, z, n, r.state, False, False)
    assert int(r.counter) == 103
    lib.arch_relax_fwd(a, z, n, r.state, False, True)                  # the counter moves without noise too, when asked
    assert int(r.counter) == 104
    saved = r.save_counter()
    lib.arch_relax_fwd(a, z, n, r.state, True, True)
    r.restore_counter(saved)
    assert int(r.counter) == 104
    # the seed and tau words were not touched
    assert r.state_dict()['seed'] == SEED and int(r.state[1]) & 0xFFFFFFFFFFFFFFFF == SEED
    assert float(r.state.view(torch.float32)[0]) == 1.0


def test_captured_launch_draws_fresh_noise_and_honours_tau():
    from bmnas import lib
    shapes = SHAPES['mixed']
    a = _logits(shapes)
    c = 50
    r = _state(2.0, step=c)
    z, n = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in a]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        lib.arch_relax_fwd(a, z, n, r.state, True, True)               # warm-up (module load) outside the capture
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    r.counter.fill_(c)
    block = r.state.data_ptr()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        lib.arch_relax_fwd(a, z, n, r.state, True, True)
    assert int(r.counter) == c                                         # a capture executes nothing
    a_np = [t.cpu().numpy() for t in a]
    taus = [2.0, 0.5, 0.5]
    for i in range(3):
        if r.tau != taus[i]:
            r.tau = taus[i]                                            # one device fill between two replays
        graph.replay()
        torch.cuda.synchronize()
        assert int(r.counter) == c + i + 1
        got_n, got_z = [t.clone() for t in n], [t.clone() for t in z]
        _check_noise(f'replay {i}', got_n, shapes, SEED, c + i)
        # the bits of an eager launch at that counter value
        e = _state(taus[i], step=c + i)
        ze, ne = [torch.empty_like(t) for t in a], [torch.empty_like(t) for t in a]
        lib.arch_relax_fwd(a, ze, ne, e.state, True, False)
        for t in range(len(a)):
            _same_bits(f'replay {i} noise[{t}]', got_n[t], ne[t])
            _same_bits(f'replay {i} z[{t}]', got_z[t], ze[t])
        for t, want in enumerate(ref.relax(a_np, [g.cpu().numpy() for g in got_n], taus[i])):
            _same_bits(f'replay {i} z[{t}] (reference)', got_z[t], want)
    assert r.state.data_ptr() == block


def test_refusals_launch_nothing():
    from bmnas import lib
    r = _state(1.0, step=7)
    a = _logits([(2, 2)])
    pool = Pool()
    z = [pool.new(2, 2)]
    with pytest.raises(lib.BmnasError, match='state'):
        lib.arch_relax_fwd(a, z, None, r.state.float(), True, True)
    with pytest.raises(lib.BmnasError, match='noise_list'):
        lib.arch_relax_fwd(a, z, [], r.state, True, True)
    with pytest.raises(lib.BmnasError, match='limit exceeded'):
        big = [torch.empty(257, 256, device=dev())]
        lib.arch_relax_fwd(big, [torch.empty_like(big[0])], None, r.state, True, True)
    with pytest.raises(lib.BmnasError, match='bad argument'):
        lib.arch_relax_fwd(a, z, None, r.state, True, True, e0=-4)
    with pytest.raises(lib.BmnasError, match='one output'):
        lib.arch_relax_bwd(a, [], r.state)
    pool.check()
    assert bool(torch.isnan(z[0]).all()) and int(r.counter) == 7


# ---- the network -------------------------------------------------------------------------------------------------------
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


BATCH, NOUT, NET_SEED = 4, 23, 11


def _classifier(cfg, linear):
    cw, cb = synth.make_classifier(cfg, NOUT, NET_SEED)
    cls = linear(cfg.M * cfg.C * cfg.L, NOUT).to(dev())
    cls.weight.data.copy_(cw)
    cls.bias.data.copy_(cb)
    return cls


def _step(net, cfg, fused_head=True):
    """One search step of `net` (built by the caller) from Philox offset 0 -> every tensor of it + the dropout sites."""
    from bmnas import cell as K, nn as bnn
    cls = _classifier(cfg, bnn.Linear if fused_head else torch.nn.Linear)
    xs = [x.to(dev()).requires_grad_(True) for x in synth.make_inputs(cfg, BATCH, NET_SEED)]
    y = synth.make_labels('bce', BATCH, NOUT, NET_SEED).to(dev())
    torch.manual_seed(1234)
    K.DROP.offset = 0
    K.DROP.record = rec = []
    try:
        if fused_head:
            with bnn.fused_criterion():
                logits = net.forward_classified(xs, cls)
                loss = bnn.BCEWithLogitsLoss()(logits, y)
        else:
            logits = cls(net(xs))
            loss = torch.nn.BCEWithLogitsLoss()(logits, y)
        loss.backward()
    finally:
        K.DROP.record = None
    out = {'logits': logits.detach().clone(), 'loss': loss.detach().clone()}
    for i, x in enumerate(xs):
        out[f'input.{i}'] = x.grad.clone()
    for n, p in net.named_parameters():
        out['p.' + n] = p.grad.clone()
    out['cls.w'], out['cls.b'] = cls.weight.grad.clone(), cls.bias.grad.clone()
    arch = [a.grad.clone() for a in net.arch_parameters()]
    torch.cuda.synchronize()
    return out, arch, rec


def _twin_check(make_net, cfg, tau, gumbel, fused_head, label):
    from bmnas import lib
    from bmnas.nn import ArchRelaxation
    net = make_net()
    relax = ArchRelaxation(tau=tau, gumbel=gumbel, seed=77)
    net.set_relaxation(relax)
    relax.counter.fill_(5)
    raw = [a.detach().clone() for a in net.arch_parameters()]
    z, noise = relax.peek(*net.arch_parameters())
    assert int(relax.counter) == 5                                      # peek leaves the counter
    raw_np = [t.cpu().numpy() for t in raw]
    if gumbel:
        _check_noise(label, noise, [tuple(t.shape) for t in raw], 77, 5)
        want_z = ref.relax(raw_np, [g.cpu().numpy() for g in noise], tau)
    else:
        assert all(not bool(g.any()) for g in noise)
        want_z = ref.relax(raw_np, None, tau)
    for t in range(len(z)):
        _same_bits(f'{label} peek z[{t}]', z[t], want_z[t])
    before = dict(lib.RELAX_LAUNCHES)
    got, got_arch, got_rec = _step(net, cfg, fused_head)
    assert lib.RELAX_LAUNCHES['fwd'] - before['fwd'] == 1               # ONE launch over alpha and every beta / gamma
    assert lib.RELAX_LAUNCHES['bwd'] - before['bwd'] == 1
    assert int(relax.counter) == (6 if gumbel else 5)
    for a, r0 in zip(net.arch_parameters(), raw):
        assert torch.equal(a.detach(), r0)                              # the raw tensors are what genotype() reads
    twin = make_net()
    for dst, src in zip(twin.arch_parameters(), z):
        dst.data.copy_(src)
    assert twin.relaxation is None
    want, want_arch, want_rec = _step(twin, cfg, fused_head)
    assert lib.RELAX_LAUNCHES['fwd'] - before['fwd'] == 1               # the twin issued none
    diff = [k for k in want if not torch.equal(got[k], want[k])]
    assert not diff, (label, len(diff), diff[:6])
    for t, (g, w) in enumerate(zip(got_arch, want_arch)):
        _same_bits(f'{label} arch grad {t}', g, ref.relax_bwd([w.cpu().numpy()], tau)[0])
    # the dropout stream does not know of the relaxation: same sites, same masks
    assert len(got_rec) == len(want_rec)
    for (da, na), (db, nb) in zip(got_rec, want_rec):
        assert (da.thr, da.seed, da.offset, na) == (db.thr, db.seed, db.offset, nb)
        assert torch.equal(lib.dropout_mask(da, na, dev()), lib.dropout_mask(db, nb, dev()))
    return got_rec


@pytest.mark.parametrize('tau,gumbel', [(0.3, True), (5.0, True), (1.0, True), (0.3, False)])
def test_fused_route_against_the_twin(deterministic, tau, gumbel):
    cfg = fo.Cfg({**fo.CONFIGS['mmimdb'], 'drpt': 0.0})
    rec = _twin_check(lambda: build_search_net(cfg, NET_SEED, 'train_nodrop'), cfg, tau, gumbel, True, f'fused tau {tau}')
    assert not rec


def test_fused_route_with_live_dropout_against_the_twin(deterministic):
    cfg = fo.Cfg({**fo.CONFIGS['mmimdb'], 'drpt': 0.1})
    rec = _twin_check(lambda: build_search_net(cfg, NET_SEED, 'train'), cfg, 0.3, True, True, 'fused, dropout')
    assert len(rec) > 0 and all(d.thr != 0 for d, _ in rec)


def test_composed_route_against_the_twin(monkeypatch):
    """An edited STEP_STEP_PRIMITIVES list: FusionCell.forward composes per-op autograd nodes and the step nodes softmax
    the relaxed tensors themselves (arch_softmax(z) in FusionCell.forward / FusionNode.forward).

    This route has no deterministic mode: its per-op backward launches add their edge-weight dot products with fp32
    atomics, one add per workgroup.  The MM-IMDB-like small configuration of tests/helpers/dp_child.py (C = 32) at b = 4
    gives those launches b C L / 4 = 512 float4 = two workgroups, i.e. at most two adds onto a zeroed address — a sum
    that does not depend on their order —, so the twin is a bit-exact reference here.  (At C = 192 the launches have 12
    workgroups and two runs of the TWIN ALONE differ in the last bits of the alpha gradient: measured, first row
    4.0323922e-04 / -4.0323989e-04 where the columns of a softmax gradient are exact negatives.)"""
    from node_prims_util import patch_oracle
    from test_node_prims_network_gpu import build as build_prims
    prims = ['Sum', 'ScaleDotAttn']
    patch_oracle(monkeypatch, prims)
    cfg = fo.Cfg({**fo.CONFIGS['mmimdb'], 'C': 32, 'drpt': 0.0})

    def make_net():
        net, _ = build_prims(cfg, NOUT, 'train_nodrop', prims, seed=NET_SEED)
        assert not all(op._default for n in net.cell._step_nodes for op in n.node_cell.node_ops)
        return net
    _twin_check(make_net, cfg, 0.3, True, False, 'composed')


def test_eval_mode_draws_no_noise_and_leaves_the_counter():
    from bmnas import lib
    from bmnas.nn import ArchRelaxation
    cfg = fo.Cfg({**fo.CONFIGS['mmimdb'], 'drpt': 0.1})
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, BATCH, NET_SEED)]
    net = build_search_net(cfg, NET_SEED, 'eval')
    relax = ArchRelaxation(tau=0.3, gumbel=True, seed=77)
    net.set_relaxation(relax)
    relax.counter.fill_(9)
    z, noise = relax.peek(*net.arch_parameters(), training=False)
    for t, (a, got) in enumerate(zip(net.arch_parameters(), z)):
        _same_bits(f'eval z[{t}]', got, ref.relax([a.detach().cpu().numpy()], None, 0.3)[0])
        assert not bool(noise[t].any())
    before = dict(lib.RELAX_LAUNCHES)
    with torch.no_grad():
        out = net(xs)
    assert lib.RELAX_LAUNCHES['fwd'] - before['fwd'] == 1 and int(relax.counter) == 9
    twin = build_search_net(cfg, NET_SEED, 'eval')
    for dst, src in zip(twin.arch_parameters(), z):
        dst.data.copy_(src)
    with torch.no_grad():
        want = twin(xs)
    assert_close_scaled('eval output', out, want, rel=1e-5)            # (default mode: batch sums are atomics)
    # ... and in training mode the same network does draw
    net.train()
    with torch.no_grad():
        net(xs)
    assert int(relax.counter) == 10


def test_weight_step_issues_no_relax_backward():
    from bmnas import cell as K, lib
    from bmnas.nn import ArchRelaxation
    cfg = fo.Cfg({**fo.CONFIGS['mmimdb'], 'drpt': 0.0})
    net = build_search_net(cfg, NET_SEED, 'train_nodrop')
    net.set_relaxation(ArchRelaxation(tau=0.5, gumbel=True, seed=3))
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, BATCH, NET_SEED)]
    before = dict(lib.RELAX_LAUNCHES)
    loss = net(xs).square().mean()
    with K.weight_grads_only(True):
        grads = torch.autograd.grad(loss, list(net.parameters()), allow_unused=True)
    torch.cuda.synchronize()
    assert lib.RELAX_LAUNCHES['fwd'] - before['fwd'] == 1 and lib.RELAX_LAUNCHES['bwd'] == before['bwd']
    assert any(g is not None for g in grads)


# ---- the default path: must pass on a tree that has no relaxation at all ------------------------------------------------
class _CountingLib:
    """Stands in for the loaded library: counts every C-ABI call (each is at most one launch)."""

    def __init__(self, real):
        self.real, self.calls = real, []

    def __getattr__(self, name):
        fn = getattr(self.real, name)

        def call(*a):
            self.calls.append(name)
            return fn(*a)
        return call


def test_default_path_is_the_network_that_never_heard_of_it(deterministic, monkeypatch):
    from bmnas import lib
    cfg = fo.Cfg({**fo.CONFIGS['mmimdb'], 'drpt': 0.1})
    counting = _CountingLib(lib.load())
    runs = []
    for reset in (False, True):
        net = build_search_net(cfg, NET_SEED, 'train')
        if reset and hasattr(net, 'set_relaxation'):
            from bmnas.nn import ArchRelaxation
            net.set_relaxation(ArchRelaxation(tau=0.3, gumbel=True))
            net.set_relaxation(None)
        monkeypatch.setattr(lib, '_lib', counting)
        counting.calls = []
        try:
            out, arch, _ = _step(net, cfg, True)
        finally:
            monkeypatch.setattr(lib, '_lib', counting.real)
        runs.append((out, arch, list(counting.calls)))
    (a, aa, ca), (b, ab, cb) = runs
    assert ca == cb and len(ca) > 4
    assert not any('relax' in c for c in ca)
    diff = [k for k in a if not torch.equal(a[k], b[k])]
    assert not diff, diff[:6]
    for x, y in zip(aa, ab):
        assert torch.equal(x, y)


# ---- captured steps -----------------------------------------------------------------------------------------------------
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))


def _hypernet(tau, gumbel, counter, lr, arch_lr):
    import torch.nn as nn
    import dp_child as ch
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase, search_setup
    cfg = ch.cfg_small()
    args = ch.make_args(cfg)
    args.use_dataparallel = False
    args.arch_learning_rate = arch_lr

    class Net(HyperNetBase):
        def __init__(self, criterion):
            super().__init__()
            self._build_head(args, criterion, nn.ModuleList([nn.Identity() for _ in range(cfg.N)]), cfg.N, 2)

        def forward(self, feats):
            return self.fuse(feats)

    crit = bnn.BCEWithLogitsLoss()
    model = Net(crit)
    model.fusion_net.load_state_dict(synth.make_params(cfg, ch.SEED))
    for dst, src in zip(model.arch_parameters(), synth.make_arch(cfg, ch.SEED, 0.5)):
        dst.data.copy_(src)
    cw, cb = synth.make_classifier(cfg, ch.NOUT, ch.SEED)
    model.central_classifier.weight.data.copy_(cw)
    model.central_classifier.bias.data.copy_(cb)
    optimizer, _, architect, _ = search_setup(model, args, crit, dev(), 1.0, args.weight_decay)
    set_mode(model, 'train_nodrop')
    for g in optimizer.param_groups:
        g['lr'] = lr
    relax = bnn.ArchRelaxation(tau=tau, gumbel=gumbel, seed=2024)
    model.fusion_net.set_relaxation(relax)
    relax.counter.fill_(counter)
    X = [x.to(dev()) for x in synth.make_inputs(cfg, BATCH, ch.SEED)]
    Y = synth.make_labels('bce', BATCH, ch.NOUT, ch.SEED).to(dev())
    return model, crit, optimizer, architect, relax, X, Y


@pytest.mark.parametrize('which', ['weight', 'arch'])
def test_three_replays_match_three_eager_steps(which):
    """GraphedTrainStep over the weight optimizer, and over the Architect's optimizer (the graph Architect.step builds),
    with Gumbel noise: replay i draws the noise of counter c + i — the warm-up passes of the build are undone — and
    the three losses are those of three eager steps of a twin started from the same state and counter (eager against
    replay: 1e-4 of the loss, the rule of tests/test_node_prims_network_gpu.py's captured step)."""
    from bmnas import lib
    from bmnas.graph import GraphedTrainStep
    c = 1000
    lr, arch_lr = 1e-2, 5e-2
    model, crit, optimizer, architect, relax, X, Y = _hypernet(0.7, True, c, lr, arch_lr)
    opt = optimizer if which == 'weight' else architect.optimizer
    step = GraphedTrainStep(model, crit, opt, X, Y)
    assert step.in_graph_step and (step.no_arch if which == 'weight' else step.arch_only)
    assert int(relax.counter) == c                                      # the build used up no draw
    block = relax.state.data_ptr()
    launches = dict(lib.RELAX_LAUNCHES)
    got = []
    for i in range(3):
        if i == 2:
            relax.tau = 0.4                                             # edited between two replays
        loss, _ = step(X, Y)
        torch.cuda.synchronize()
        got.append(float(loss))
        assert int(relax.counter) == c + i + 1
    assert lib.RELAX_LAUNCHES == launches and relax.state.data_ptr() == block      # replays: no Python launch
    del step
    # the same three steps eagerly
    model2, crit2, optimizer2, architect2, relax2, _, _ = _hypernet(0.7, True, c, lr, arch_lr)
    opt2 = optimizer2 if which == 'weight' else architect2.optimizer
    want = []
    for i in range(3):
        if i == 2:
            relax2.tau = 0.4
        opt2.zero_grad()
        loss = crit2(model2(X), Y)
        loss.backward()
        opt2.step()
        want.append(float(loss.detach()))
    torch.cuda.synchronize()
    assert int(relax2.counter) == c + 3
    print(which, 'replays', got, 'eager', want)
    for g, w in zip(got, want):
        assert abs(g - w) <= 1e-4 * max(1.0, abs(w)), (which, got, want)
    assert len({round(v, 7) for v in want}) == 3                        # real steps: the loss moved
    # the noise is part of those losses: a twin one draw behind does not reproduce them
    model3, crit3, _, _, _, _, _ = _hypernet(0.7, True, c + 1, lr, arch_lr)
    with torch.no_grad():
        other = float(crit3(model3(X), Y))
    assert abs(other - want[0]) > 1e-4 * max(1.0, abs(want[0])), (other, want[0])


def test_captured_forward_draws_fresh_noise_in_training_mode():
    from bmnas.graph import GraphedForward
    model, crit, _, _, relax, X, Y = _hypernet(0.7, True, 300, 0.0, 0.0)
    g = GraphedForward(model, crit, X, Y)
    assert int(relax.counter) == 300
    losses = []
    for i in range(3):
        loss, _ = g(X, Y)
        torch.cuda.synchronize()
        losses.append(float(loss))
        assert int(relax.counter) == 301 + i
    assert len({round(v, 7) for v in losses}) == 3                      # three draws
    # eager, from the same counter
    relax.counter.fill_(300)
    with torch.no_grad():
        want = float(crit(model(X), Y))
    assert abs(losses[0] - want) <= 1e-4 * max(1.0, abs(want)), (losses, want)
