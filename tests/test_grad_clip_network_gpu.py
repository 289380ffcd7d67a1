"""-m gpu: bmnas.optim.Adam(max_grad_norm=...) inside captured steps of whole networks — GraphedTrainStep against an eager
twin that clips with torch.nn.utils.clip_grad_norm_, k steps per replay, the launches of the captured step, the
deterministic mode, the drivers' arguments, and two data-parallel ranks.  Small configurations of
tests/test_crit_network_gpu.py (SMALL_LAZY search cell, SMALL_PLAIN found network, batch 17).

Parameters are compared at the gradient tolerance of tests/gpu_util.py (2e-4 of |want| + scale): the two sides' gradients
agree to that (fp32 atomics accumulate them in a run-dependent order) and Adam's update is bounded by lr per step."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from fc_edges_util import device_kernels
from gpu_util import assert_close_scaled, dev
from oracle import fusion_oracle as fo
from test_crit_network_gpu import SMALL_LAZY, SMALL_PLAIN, _batch, _model

pytestmark = pytest.mark.gpu

BATCH, NOUT = 17, 23
GRAD_REL = 2e-4
HELPERS = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers')
CHILD = os.path.join(HELPERS, 'clip_dp_child.py')


def _crit():
    from bmnas import nn as bnn
    return bnn.BCEWithLogitsLoss()


def _first_norm(shape, found, xs, y):
    """Global gradient norm of the first step of a fresh model (nothing of its autograd graph survives the call)."""
    model = _model(fo.make_cfg(**shape), NOUT, found)
    _crit()(model(xs), y).backward()
    n = float(torch.nn.utils.clip_grad_norm_(list(model.parameters()), 1e30))
    torch.cuda.synchronize()
    return n


def _eager_clipped(model, opt, crit, xs, y, c):
    """backward, torch's clip_grad_norm_, an UNCLIPPED bmnas.optim.Adam step -> the pre-clip norm"""
    opt.zero_grad()
    crit(model(xs), y).backward()
    n = float(torch.nn.utils.clip_grad_norm_(list(model.parameters()), c))
    opt.step()
    return n


def _same_params(label, got, want):
    for (k, a), (_, b) in zip(got.named_parameters(), want.named_parameters()):
        assert_close_scaled(f'{label} {k}', a, b, rel=GRAD_REL)


@pytest.mark.parametrize('shape,found', [(SMALL_LAZY, False), (SMALL_PLAIN, True)], ids=['search', 'found'])
def test_captured_clipped_step_follows_the_eager_twin(shape, found):
    from bmnas import cell as K
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg = fo.make_cfg(**shape)
    xs, y = _batch(cfg, BATCH, NOUT, 'bce', None)
    n0 = _first_norm(shape, found, xs, y)
    c = n0 / 2                                                    # half the first step's norm: it clips
    crit = _crit()
    models = [_model(cfg, NOUT, found) for _ in range(2)]
    opt_g = Adam(list(models[0].parameters()), lr=1e-3, weight_decay=1e-4, max_grad_norm=c)
    opt_e = Adam(list(models[1].parameters()), lr=1e-3, weight_decay=1e-4)
    step = GraphedTrainStep(models[0], crit, opt_g, xs, y)
    start = [p.detach().clone() for p in models[0].parameters()]
    for r in range(3):
        if r == 2:
            c = opt_g.max_grad_norm = c / 4                       # in place, between replays 2 and 3
        step(xs, y)
        got = float(opt_g.last_grad_norm)
        want = _eager_clipped(models[1], opt_e, crit, xs, y, c)
        print(f'replay {r}: norm {got!r} twin {want!r} max_grad_norm {c!r}')
        assert want > c and abs(got - want) <= GRAD_REL * want
        _same_params(f'replay {r}', models[0], models[1])
    assert any(not torch.equal(a, b) for a, b in zip(start, models[0].parameters()))


def test_two_steps_per_replay_equal_two_single_replays():
    """GraphedTrainStep(k=2) with clipping: one norm output per slot.  Against two single replays on a twin: parameters at
    the gradient tolerance; grad_norms' two entries against the twin's two last_grad_norm values at the same (the two
    graphs accumulate their gradients in run-dependent order)."""
    from bmnas import cell as K
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg = fo.make_cfg(**SMALL_LAZY)
    batches = [_batch(cfg, BATCH, NOUT, 'bce', None, seed=s) for s in (31, 32)]
    c = _first_norm(SMALL_LAZY, False, *batches[0]) / 2
    crit = _crit()
    models = [_model(cfg, NOUT) for _ in range(2)]
    opts = [Adam(list(m.parameters()), lr=1e-3, weight_decay=1e-4, max_grad_norm=c) for m in models]
    g2 = GraphedTrainStep(models[0], crit, opts[0], *batches[0], k=2)
    g1 = GraphedTrainStep(models[1], crit, opts[1], *batches[0])
    for j, (xs, y) in enumerate(batches):
        g2.stage(j, xs, y)
    g2.replay_staged()
    norms = opts[0].grad_norms
    assert norms.shape == (2,) and norms.dtype == torch.float32
    singles = []
    for xs, y in batches:
        g1(xs, y)
        singles.append(float(opts[1].last_grad_norm))
    assert opts[1].grad_norms.shape == (1,)
    print(f'k=2 norms {norms.tolist()!r} single replays {singles!r}')
    for a, b in zip(norms.tolist(), singles):
        assert b > c and abs(a - b) <= GRAD_REL * b
    assert float(opts[0].last_grad_norm) == float(norms[1])
    _same_params('k=2', models[0], models[1])


@pytest.mark.parametrize('shape,found', [(SMALL_LAZY, False), (SMALL_PLAIN, True)], ids=['search', 'found'])
def test_clipped_captured_step_has_one_more_device_event(shape, found):
    """The norm launch is the one addition; the clipped update replaces the unclipped one; nothing of aten."""
    from bmnas import cell as K
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    if not K.FUSE_HEAD:
        pytest.skip('BMNAS_FUSE_HEAD=0')
    cfg = fo.make_cfg(**shape)
    xs, y = _batch(cfg, BATCH, NOUT, 'bce', None)
    names = {}
    for label, c in (('plain', None), ('clipped', 1.0)):
        model = _model(cfg, NOUT, found)
        step = GraphedTrainStep(model, _crit(), Adam(list(model.parameters()), lr=1e-3, max_grad_norm=c), xs, y)
        step(xs, y)
        torch.cuda.synchronize()
        names[label] = device_kernels(lambda: step(xs, y))
        assert torch.isfinite(step(xs, y)[0]).all()
        del step
    plain, clipped = names['plain'], names['clipped']
    print(f'{len(plain)} device events unclipped, {len(clipped)} clipped')
    assert len(clipped) == len(plain) + 1, (plain, clipped)
    assert not [n for n in clipped if 'at::native' in n]
    assert sum('grad_sqnorm_multi_k' in n for n in clipped) == 1 and sum('adam_multi_clip_k' in n for n in clipped) == 1
    assert not [n for n in plain if 'grad_sqnorm_multi_k' in n or 'adam_multi_clip_k' in n]


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


def test_deterministic_mode_clipped_replays_are_bit_identical(deterministic):
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    cfg = fo.make_cfg(**SMALL_LAZY)
    xs, y = _batch(cfg, BATCH, NOUT, 'bce', None)
    c = _first_norm(SMALL_LAZY, False, xs, y) / 2
    runs = []
    for _ in range(2):
        model = _model(cfg, NOUT)
        opt = Adam(list(model.parameters()), lr=1e-3, weight_decay=1e-4, max_grad_norm=c)
        step = GraphedTrainStep(model, _crit(), opt, xs, y)
        norms = []
        for _ in range(3):
            step(xs, y)
            norms.append(opt.last_grad_norm.clone())
        torch.cuda.synchronize()
        out = {k: v.detach().clone() for k, v in model.named_parameters()}
        out.update({f'norm.{i}': n for i, n in enumerate(norms)})
        runs.append(out)
        del step
    a, b = runs
    assert float(a['norm.0']) > c
    diff = [k for k in a if not torch.equal(a[k].view(torch.int32), b[k].view(torch.int32))]
    assert not diff, (len(diff), diff[:6])


def test_search_setup_reads_grad_clip_and_arch_grad_clip():
    sys.path.insert(0, HELPERS)
    import clip_dp_child as ch
    _, _, optimizer, architect, _ = ch.build()
    assert optimizer.max_grad_norm is None and architect.optimizer.max_grad_norm is None
    _, _, optimizer, architect, _ = ch.build(grad_clip=5.0, arch_grad_clip=0.5)
    assert optimizer.max_grad_norm == 5.0 and architect.optimizer.max_grad_norm == 0.5
    assert all('max_grad_norm' not in g for g in optimizer.state_dict()['param_groups'])


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_ranks_clip_the_same_averaged_gradients(tmp_path):
    """Two fresh child processes, one GPU, gloo (tests/test_dp_gpu.py's arrangement).  Every rank clips the all-reduced
    gradients with the same deterministic reduction: bit-identical parameters and norms after two steps, no broadcast.
    The single-process reference takes the global batch shard by shard (per-replica BatchNorm statistics, as
    nn.DataParallel and the data-parallel oracle of test_dp_gpu.py do), averages the shard gradients, clips with torch
    and steps an unclipped optimizer; tolerance: that file's 5e-4."""
    sys.path.insert(0, HELPERS)
    import clip_dp_child as ch
    from bmnas import dist as bdist
    model, crit, optimizer, _, _ = ch.build()
    X, Y = ch.global_batch(dev())
    shards = [([bdist.shard(x, r, 2).contiguous() for x in X], bdist.shard(Y, r, 2).contiguous()) for r in range(2)]
    params = [p for g in optimizer.param_groups for p in g['params']]

    def averaged_grads():
        acc = None
        for xs, y in shards:
            optimizer.zero_grad()
            crit(model(xs), y).backward()
            gs = [None if p.grad is None else p.grad.detach().clone() for p in params]
            acc = gs if acc is None else [a if g is None else a + g for a, g in zip(acc, gs)]
        for p, a in zip(params, acc):
            p.grad = None if a is None else a / 2
    averaged_grads()
    c = float(torch.nn.utils.clip_grad_norm_(params, 1e30)) / 2
    want_norms = []
    for it in range(ch.STEPS):
        if it:
            averaged_grads()
        want_norms.append(float(torch.nn.utils.clip_grad_norm_(params, c)))
        optimizer.step()
    torch.cuda.synchronize()
    want = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}

    port = _free_port()
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE='2', MASTER_ADDR='127.0.0.1',
                   MASTER_PORT=str(port), BMNAS_FORCE_DEVICE='0', BMNAS_DIST_BACKEND='gloo',
                   HSA_ENABLE_IPC_MODE_LEGACY='0')
        env.pop('BMNAS_HIP_GRAPH', None)
        procs.append(subprocess.Popen([sys.executable, CHILD, str(tmp_path), repr(c)], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True))
    logs = []
    for p in procs:
        try:
            o, _ = p.communicate(timeout=600)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        logs.append(o)
    for r, (p, o) in enumerate(zip(procs, logs)):
        assert p.returncode == 0, f'rank {r} failed:\n{o[-4000:]}'
    d0 = torch.load(tmp_path / 'clip_rank0.pt')
    d1 = torch.load(tmp_path / 'clip_rank1.pt')
    assert set(d0) == set(d1)
    for k in d0:
        assert torch.equal(d0[k].view(torch.int32), d1[k].view(torch.int32)), k
    for it, n in enumerate(want_norms):
        got = float(d0[f'norm:{it}'])
        print(f'step {it}: norm {got!r} single process {n!r} max_grad_norm {c!r}')
        assert n > c and abs(got - n) <= 5e-4 * n
    checked = 0
    for n, w in want.items():
        assert_close_scaled(n, d0['param:' + n], w, rel=5e-4)
        checked += 1
    assert checked > 20
