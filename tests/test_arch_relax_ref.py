"""CPU: the numpy restatement of the architecture relaxation (tests/arch_relax_ref.py) pinned against the definitions of
include/bmnas_hip.h, the schedule and refusals of bmnas.nn.ArchRelaxation, the trainers' argument reader, and the C ABI of
the two entry points (exported, bound, and refusing bad arguments without a launch — no GPU is touched)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import arch_relax_ref as ref
from oracle.philox import philox4x32_10


# ---- the noise ---------------------------------------------------------------------------------------------------------
def test_range_of_u_and_G():
    lo, hi = ref.uniform32(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert lo.dtype == np.float32 and float(lo) == 2.0 ** -24 and float(hi) == 1.0 - 2.0 ** -24
    g = ref.gumbel32(np.array([0, 0xFFFFFFFF], dtype=np.uint32))
    assert np.isfinite(g).all()
    assert -2.82 < float(g[0]) < -2.81 and 16.63 < float(g[1]) < 16.64
    # every u is exact: the fp32 value equals the float64 formula
    w = ref.words(7, 3, 0, 4096)
    assert np.array_equal(ref.uniform32(w).astype(np.float64), ((w >> 9).astype(np.float64) + 0.5) * 2.0 ** -23)
    # a 24-bit mantissa of the top word would round to 1: what the 23-bit construction avoids
    assert np.float32((0xFFFFFFFF >> 8) + 0.5) * np.float32(2.0 ** -24) == np.float32(1.0)


def test_fp32_G_against_float64_over_2_20_words():
    w = ref.words(7, 3, 0, 1 << 20)
    g32, g64 = ref.gumbel32(w).astype(np.float64), ref.gumbel64(w)
    scaled = np.abs(g32 - g64) / np.maximum(1.0, np.abs(g64))
    print('max |G32 - G64| / max(1, |G|) =', scaled.max(), 'bound', 8 * 2.0 ** -23)
    assert (np.abs(g32 - g64) <= ref.gumbel_bound(g64)).all()


LOGITS = np.array([0.3, -0.5, 1.1, 0.0])
BOUND = 0.0177                      # 5 binomial standard deviations at p = 1 / 2, n = 20000: 5 * sqrt(0.25 / 20000)


def _softmax(a):
    e = np.exp(a - a.max())
    return e / e.sum()


def test_gumbel_max_frequencies_one_step():
    g = ref.gumbel64(ref.words(1234, 0, 0, 20000 * 4)).reshape(20000, 4)
    freq = np.bincount(np.argmax(LOGITS + g, axis=1), minlength=4) / 20000.0
    dev = np.abs(freq - _softmax(LOGITS)).max()
    print('gumbel-max deviation', dev)
    assert 5.0 * np.sqrt(0.25 / 20000.0) <= BOUND
    assert dev <= BOUND


def test_gumbel_max_frequencies_four_steps():
    """4 steps of 5000 rows: the `step << 32` term of the counter; the steps' draws are different and jointly Gumbel."""
    gs = [ref.gumbel64(ref.words(1234, s, 0, 5000 * 4)).reshape(5000, 4) for s in range(4)]
    for s in range(1, 4):
        assert not np.array_equal(gs[0], gs[s])
    g = np.concatenate(gs)
    freq = np.bincount(np.argmax(LOGITS + g, axis=1), minlength=4) / 20000.0
    dev = np.abs(freq - _softmax(LOGITS)).max()
    print('gumbel-max deviation over 4 steps', dev)
    assert dev <= BOUND


def test_counter_layout_and_salt():
    seed, step = 0x123456789ABCDEF0, 5
    key = seed ^ 0x6A09E667F3BCC908
    w = ref.words(seed, step, 0, 10)
    for e in range(10):
        four = philox4x32_10(np.array([(step << 32) + (e >> 2)], dtype=np.uint64), key)[0]
        assert int(w[e]) == int(four[e & 3])
    # e0 shifts the sequence: a split call draws what one call draws
    assert np.array_equal(ref.words(seed, step, 6, 4), w[6:])


def test_elements_that_straddle_a_tensor_boundary():
    """A 3 x 3 tensor followed by a 2 x 2 one: flat elements 8 (last of the first) and 9 (first of the second) share
    counter 2 and take its words 0 and 1; element 12 (last of the second) takes word 0 of counter 3."""
    shapes = [(3, 3), (2, 2)]
    seed, step = 99, 2
    n = ref.noise64(shapes, seed, step)
    assert [t.shape for t in n] == shapes
    key = seed ^ ref.SALT
    c2 = philox4x32_10(np.array([(step << 32) + 2], dtype=np.uint64), key)[0]
    c3 = philox4x32_10(np.array([(step << 32) + 3], dtype=np.uint64), key)[0]
    assert n[0][2, 2] == ref.gumbel64(c2[0:1])[0]
    assert n[1][0, 0] == ref.gumbel64(c2[1:2])[0]
    assert n[1][0, 1] == ref.gumbel64(c2[2:3])[0]
    assert n[1][1, 1] == ref.gumbel64(c3[0:1])[0]


def test_relax_arithmetic_is_rounded_step_by_step():
    a = [np.array([[0.1, 0.7]], np.float32)]
    g = [np.array([[1.3, -0.4]], np.float32)]
    z = ref.relax(a, g, 0.3)[0]
    s = (a[0] + g[0]).astype(np.float32)
    assert z.dtype == np.float32 and np.array_equal(z, s / np.float32(0.3))
    assert np.array_equal(ref.relax(a, None, 5.0)[0], a[0] / np.float32(5.0))
    assert np.array_equal(ref.relax_bwd(g, 0.3)[0], g[0] / np.float32(0.3))


# ---- the schedule and the object's host side ---------------------------------------------------------------------------
def test_schedule_end_points_and_monotonicity():
    from bmnas.nn import ArchRelaxation, relax_schedule_tau
    taus = [relax_schedule_tau(5.0, 0.1, 30, e) for e in range(30)]
    assert taus[0] == 5.0 and abs(taus[-1] - 0.1) <= 1e-15
    assert all(b < a for a, b in zip(taus, taus[1:]))
    for e in range(30):
        assert taus[e] == ref.schedule(5.0, 0.1, 30, e)
    ratios = [b / a for a, b in zip(taus, taus[1:])]
    assert max(ratios) - min(ratios) < 1e-12                     # exponential: a constant ratio
    assert relax_schedule_tau(5.0, 0.1, 1, 0) == 5.0             # epochs == 1
    assert relax_schedule_tau(2.0, 2.0, 7, 3) == 2.0
    r = ArchRelaxation(tau=5.0).set_schedule(5.0, 0.1, 30)
    assert r.set_epoch(0) == 5.0 and r.tau == 5.0
    assert r.set_epoch(29) == taus[-1] and r.tau == taus[-1]
    assert r.set_epoch(40) == taus[-1]                           # past the end: the last value holds
    one = ArchRelaxation(tau=3.0).set_schedule(3.0, 0.5, 1)
    assert one.set_epoch(0) == 3.0
    free = ArchRelaxation(tau=0.7)
    assert free.set_epoch(5) == 0.7                              # no schedule: tau stays


def test_refusals_of_tau_and_schedule():
    from bmnas.nn import ArchRelaxation
    for bad in (0.0, -1.0, float('nan'), float('inf')):
        with pytest.raises(ValueError, match='tau'):
            ArchRelaxation(tau=bad)
    r = ArchRelaxation()
    with pytest.raises(ValueError, match='tau'):
        r.tau = 0
    assert r.tau == 1.0                                          # a refused value changes nothing
    with pytest.raises(ValueError, match='tau_min'):
        r.set_schedule(1.0, 2.0, 10)                             # tau_min > tau_max
    with pytest.raises(ValueError, match='tau_min'):
        r.set_schedule(1.0, 0.0, 10)
    with pytest.raises(ValueError, match='epochs'):
        r.set_schedule(1.0, 0.5, 0)
    assert r.schedule is None


def test_state_block_layout_and_state_dict_round_trip():
    from bmnas import lib
    from bmnas.nn import ArchRelaxation
    r = ArchRelaxation(tau=0.3, gumbel=True, seed=0xFEDCBA9876543210)
    assert r.state.dtype == torch.int64 and r.state.numel() == lib.RELAX_STATE_WORDS == 3
    raw = r.state.numpy().tobytes()
    assert np.frombuffer(raw[0:4], np.float32)[0] == np.float32(0.3)            # float tau at offset 0
    assert int(np.frombuffer(raw[8:16], np.uint64)[0]) == 0xFEDCBA9876543210    # uint64 seed at offset 8
    assert int(np.frombuffer(raw[16:24], np.uint64)[0]) == 0                    # uint64 step at offset 16
    r.set_schedule(2.0, 0.3, 12)
    r.set_epoch(4)
    r.counter.fill_(41)
    sd = r.state_dict()
    assert set(sd) == {'tau', 'gumbel', 'seed', 'counter', 'schedule', 'epoch'}
    q = ArchRelaxation()
    q.load_state_dict(sd)
    assert (q.tau, q.gumbel, q.seed, q.schedule, q.epoch) == (r.tau, True, 0xFEDCBA9876543210, (2.0, 0.3, 12), 4)
    assert torch.equal(q.state, r.state)
    assert int(q.counter) == 41
    saved = q.save_counter()
    q.counter.add_(3)
    q.restore_counter(saved)
    assert int(q.counter) == 41
    # seed None: torch's
    torch.manual_seed(1234)
    assert ArchRelaxation().seed == 1234
    assert ArchRelaxation().draws(True) is False and ArchRelaxation(gumbel=True).draws(False) is False
    assert ArchRelaxation(gumbel=True).draws(True) is True


def test_relaxation_needs_device_tensors():
    from bmnas.nn import ArchRelaxation
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ArchRelaxation(tau=2.0)(True, torch.zeros(3, 2, requires_grad=True))


def test_network_default_is_no_relaxation():
    from models.search.darts.model_search import FusionNetwork

    class A:
        C, L, drpt, num_input_nodes, node_steps, node_multiplier = 16, 8, 0.1, 3, 1, 1

    net = FusionNetwork(2, 2, 3, 2, A())
    assert net.relaxation is None
    g = net.genotype()
    from bmnas.nn import ArchRelaxation
    r = ArchRelaxation(tau=0.2, gumbel=True, seed=5)
    assert net.set_relaxation(r) is net and net.relaxation is r
    assert net.genotype() == g                                   # reads the raw tensors
    assert 'relax' not in ''.join(net.state_dict())              # not a submodule: the reference's keys
    net.set_relaxation(None)
    assert net.relaxation is None


# ---- the trainers' argument reader -------------------------------------------------------------------------------------
def _args(**kw):
    return types.SimpleNamespace(**kw)


def test_argument_reader(monkeypatch):
    from models.search._common import relaxation_option
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    assert relaxation_option(_args(), 'search', 10) is None
    assert relaxation_option(_args(arch_tau=None, arch_tau_min=None, arch_gumbel=False), 'search', 10) is None
    assert relaxation_option(_args(), 'eval', 10) is None and relaxation_option(_args(unrolled=True), 'search', 3, world=4) is None
    r = relaxation_option(_args(arch_tau=2.0), 'search', 10)
    assert (r.tau, r.gumbel, r.schedule) == (2.0, False, None)
    r = relaxation_option(_args(arch_tau=4.0, arch_tau_min=0.5, seed=77), 'search', 10)
    assert r.schedule == (4.0, 0.5, 10) and r.seed == 77 and not r.gumbel
    torch.manual_seed(4321)
    r = relaxation_option(_args(arch_gumbel=True), 'search', 10)
    assert r.tau == 1.0 and r.gumbel and r.seed == 4321
    r = relaxation_option(_args(arch_tau_min=0.25), 'search', 1)
    assert r.schedule == (1.0, 0.25, 1) and r.set_epoch(0) == 1.0
    for a in (_args(arch_tau=2.0), _args(arch_gumbel=True), _args(arch_tau_min=0.5)):
        with pytest.raises(ValueError, match='found-stage'):
            relaxation_option(a, 'eval', 10)
    with pytest.raises(ValueError, match='unrolled'):
        relaxation_option(_args(arch_tau=2.0, unrolled=True), 'search', 10)
    with pytest.raises(ValueError, match='data parallelism'):
        relaxation_option(_args(arch_gumbel=True), 'search', 10, world=2)
    monkeypatch.setenv('WORLD_SIZE', '2')
    with pytest.raises(ValueError, match='data parallelism'):
        relaxation_option(_args(arch_gumbel=True), 'search', 10)
    monkeypatch.delenv('WORLD_SIZE')
    with pytest.raises(ValueError, match='tau'):
        relaxation_option(_args(arch_tau=0.0), 'search', 10)
    with pytest.raises(ValueError, match='tau_min'):
        relaxation_option(_args(arch_tau=0.5, arch_tau_min=1.0), 'search', 10)


@pytest.mark.parametrize('status,extra,world,match', [('eval', {}, 1, 'found-stage'), ('search', dict(unrolled=True), 1, 'unrolled'),
                                                      ('search', {}, 2, 'data parallelism')])
def test_run_refuses_at_its_start(status, extra, world, match, monkeypatch):
    import models.search.train_searchable._loop as loop
    monkeypatch.delenv('BMNAS_STEPS_PER_REPLAY', raising=False)
    monkeypatch.delenv('WORLD_SIZE', raising=False)
    monkeypatch.setattr(loop, '_world', lambda: world)
    # nothing else is looked at: no model, no loaders
    with pytest.raises(ValueError, match=match):
        loop.run(None, None, None, None, None, None, None, None, 1, None, None, _args(arch_gumbel=True, **extra), status,
                 None, None, None, None)


def test_loop_sets_the_relaxation_on_the_network_and_keeps_it(monkeypatch):
    import models.search.train_searchable._loop as loop
    from models.search.darts.model_search import FusionNetwork
    monkeypatch.delenv('WORLD_SIZE', raising=False)

    class A:
        C, L, drpt, num_input_nodes, node_steps, node_multiplier = 16, 8, 0.1, 3, 1, 1

    model = types.SimpleNamespace(fusion_net=FusionNetwork(2, 2, 3, 2, A()))
    assert loop._set_relaxation(model, _args(), 'search', 5) is None and model.fusion_net.relaxation is None
    r = loop._set_relaxation(model, _args(arch_tau=2.0, arch_tau_min=0.5, arch_gumbel=True, seed=9), 'search', 5)
    assert model.fusion_net.relaxation is r and r.schedule == (2.0, 0.5, 5) and r.gumbel and r.seed == 9
    taus = [r.set_epoch(e) for e in range(5)]
    assert taus[0] == 2.0 and abs(taus[-1] - 0.5) < 1e-15 and taus == sorted(taus, reverse=True)
    r.counter.fill_(17)
    block = r.state.data_ptr()
    # a second run() on the same model: the object (captured steps hold its block) stays, the settings are the new ones
    r2 = loop._set_relaxation(model, _args(arch_tau=1.5), 'search', 3)
    assert r2 is r and r.state.data_ptr() == block and int(r.counter) == 17
    assert (r.tau, r.gumbel, r.schedule) == (1.5, False, None)
    with pytest.raises(ValueError, match='search hypernet'):
        loop._set_relaxation(types.SimpleNamespace(fusion_net=torch.nn.Identity()), _args(arch_tau=2.0), 'search', 3)


# ---- the C ABI (tests/test_abi.py's checks for the two entry points) -----------------------------------------------------
def test_entry_points_are_declared_exported_and_bound():
    import os
    import re
    from bmnas import build, lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(root, 'include', 'bmnas_hip.h')).read(), flags=re.S)
    so = ctypes.CDLL(build.build())
    for name in ('bmnas_arch_relax_fwd', 'bmnas_arch_relax_bwd'):
        assert re.search(r'\bint\s+' + name + r'\s*\(', text)
        assert hasattr(so, name) and name in lib.SIGNATURES
    assert 'bmnas_arch_relax_state_t' in text
    assert len(lib.SIGNATURES['bmnas_arch_relax_fwd'][0]) == 11 and len(lib.SIGNATURES['bmnas_arch_relax_bwd'][0]) == 7
    assert 'relax.hip' in build.SOURCES


def test_refusals_return_codes_without_a_launch():
    """Argument errors are answered on the host, before any HIP call: the pointers below are never dereferenced on a
    device (this machine may have none)."""
    from bmnas import lib
    so = lib.load()
    P, I = ctypes.c_void_p, ctypes.c_int
    buf = (ctypes.c_float * 8)()                                   # stands for device memory; never read
    addr = ctypes.addressof(buf)
    state = (ctypes.c_int64 * 3)()
    sp = ctypes.addressof(state)

    def ptrs(*v):
        return (P * len(v))(*v)

    def ints(*v):
        return (I * len(v))(*v)

    E_ARG, E_LIMIT = -1, -3
    fwd, bwd = so.bmnas_arch_relax_fwd, so.bmnas_arch_relax_bwd
    ok = (ptrs(addr), ptrs(addr), None, ints(2), ints(2), 1, 0, sp, 0, 0, None)

    def with_(i, v):
        a = list(ok)
        a[i] = v
        return a

    assert fwd(*with_(0, None)) == E_ARG and fwd(*with_(1, None)) == E_ARG
    assert fwd(*with_(3, None)) == E_ARG and fwd(*with_(4, None)) == E_ARG
    assert fwd(*with_(7, None)) == E_ARG                           # no state block
    assert fwd(*with_(0, ptrs(None))) == E_ARG and fwd(*with_(1, ptrs(None))) == E_ARG
    assert fwd(*with_(3, ints(0))) == E_ARG and fwd(*with_(4, ints(0))) == E_ARG
    assert fwd(*with_(5, 0)) == E_ARG and fwd(*with_(6, -1)) == E_ARG
    assert fwd(*with_(5, 17)) == E_LIMIT
    assert fwd(ptrs(addr), ptrs(addr), None, ints(65537), ints(1), 1, 0, sp, 0, 0, None) == E_LIMIT
    # 256 x 128 + 257 x 128 = 65664 elements, 128 more than a launch takes
    assert fwd(ptrs(addr, addr), ptrs(addr, addr), None, ints(256, 257), ints(128, 128), 2, 0, sp, 1, 1, None) == E_LIMIT
    okb = (ptrs(addr), ptrs(addr), ints(2), ints(2), 1, sp, None)
    for i, v, rc in ((0, None, E_ARG), (1, None, E_ARG), (2, None, E_ARG), (3, None, E_ARG), (5, None, E_ARG),
                     (0, ptrs(None), E_ARG), (2, ints(-3), E_ARG), (3, ints(0), E_ARG), (4, 0, E_ARG), (4, 17, E_LIMIT)):
        a = list(okb)
        a[i] = v
        assert bwd(*a) == rc, (i, rc)
    assert state[2] == 0 and all(x == 0.0 for x in buf)
