"""-m gpu: mixed-edge sums whose PRIMITIVES list holds fc_relu / fc_mish on the grouped kernels of csrc/fcedge.hip
(bmnas.functions.FcEdgeSumFn, reached through models.search.darts.operations.general_edge_sum) against the CPU
oracle (fo.mixed_edge_general summed over the edges), and the launch accounting of that path.

ReLU decisions: a pre-activation of fc_relu within round-off of zero may fall on either side, and one such element
moves its column of dx well beyond the gradient tolerance.  The kernel's stored pre-activations are read back
(out.grad_fn.fc_U); every element whose sign disagrees with the fp32 oracle's must have |u_oracle| < 2e-5 (the `near`
of gpu_util.match_step) — anything else fails — and the gradients are then compared, every element, against the
oracle evaluated under exactly those decisions (fo.relu_decisions(flips=...))."""
import contextlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fusion_oracle as fo
from oracle import synth
from fc_edges_util import device_kernels, edited_primitives, recorded_sites
from gpu_util import Args, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

FULL = ['none', 'fc_relu', 'fc_mish', 'skip']
LISTS = [FULL, ['skip', 'fc_mish', 'none'], ['none', 'skip', 'fc_relu']]
# (n, C, L, b, inner): inner = 2 states that are ONE tensor and 2-column weight rows (a search NodeCell's first sum)
SHAPES = [(6, 192, 16, 128, False), (7, 192, 16, 37, False), (8, 128, 8, 64, False), (9, 128, 8, 7, False),
          (2, 192, 16, 128, True), (2, 128, 8, 8, True), (4, 128, 8, 6, False), (3, 48, 8, 5, False),
          (2, 80, 4, 3, True)]
MODES = ['eval', 'train_nodrop', 'train_drop']
NEAR = 2e-5


def build_edges(prims, n, C, L, mode, seed, drpt=0.1):
    """n FusionMixedOps over the edited list with the synthetic parameters of cell._ops.{0..n-1}."""
    from models.search.darts.operations import FusionMixedOp
    cfg = fo.make_cfg(N=n, C=C, L=L, S=1, M=1, drpt=drpt)
    p = synth.make_params(cfg, seed, fo.param_shapes(cfg, prims))
    with edited_primitives(prims):
        ops = torch.nn.ModuleList(FusionMixedOp(C, L, Args(cfg)) for _ in range(n))
    sd = {k[len('cell._ops.'):]: v for k, v in p.items() if k.startswith('cell._ops.')}
    assert set(sd) == set(ops.state_dict())
    ops.load_state_dict(sd)
    ops.to(dev())
    ops.train(mode != 'eval')
    for m in ops.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = drpt if mode == 'train_drop' else 0.0
    return cfg, p, ops


def make_case(prims, n, C, L, b, inner, seed):
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    n_x = 1 if inner else n
    xs = [torch.from_numpy(np.maximum(rng.standard_normal((b, C, L)), 0.0).astype(np.float32)) for _ in range(n_x)]
    P = 2 if inner else len(prims)
    w = torch.softmax(torch.from_numpy((0.5 * rng.standard_normal((n, P))).astype(np.float32)), -1)
    gw = torch.from_numpy(rng.standard_normal((b, C, L)).astype(np.float32))
    return xs, w, gw


def oracle_run(prims, cfg, p, xs, w, gw, n, inner, training, drpt, masks, flips):
    po = {k: (v.clone() if fo.is_buffer(k) else v.clone().requires_grad_(True)) for k, v in p.items()}
    xo = [x.clone().requires_grad_(True) for x in xs]
    wo = w.clone().requires_grad_(True)
    states = [xo[0]] * n if inner else xo
    inj = fo.injected_masks(masks) if masks else contextlib.nullcontext()
    with inj, fo.relu_decisions(0.0, flips):
        out = sum(fo.mixed_edge_general(h, wo[j], po, f'cell._ops.{j}', prims, training, drpt)
                  for j, h in enumerate(states))
    if masks:
        assert inj.used == len(masks)
    out.backward(gw)
    return out.detach(), xo, wo, po


def relu_flips(prims, part, p, xs, n, inner, U):
    """(site, flat index) of every fc_relu pre-activation the kernel put on the other side of zero than the fp32
    oracle; asserts each of them is within NEAR of zero in the oracle."""
    if 'fc_relu' not in part:
        return []
    fcs = [q for q in part if q in ('fc_relu', 'fc_mish')]
    f, pi = fcs.index('fc_relu'), part.index('fc_relu')
    C = xs[0].shape[1]
    flips = []
    for j in range(n):
        x = xs[0] if inner else xs[j]
        u_or = F.linear(x.transpose(1, 2), p[f'cell._ops.{j}._ops.{pi}.linear.weight'],
                        p[f'cell._ops.{j}._ops.{pi}.linear.bias']).transpose(1, 2).reshape(-1)
        u_k = U[j][:, f * C:(f + 1) * C, :].cpu().reshape(-1)
        assert_close_scaled(f'U[{j}]', u_k, u_or)
        bad = torch.nonzero((u_k > 0) != (u_or > 0)).reshape(-1)
        if bad.numel():
            worst = float(u_or[bad].abs().max())
            print(f'edge {j}: {bad.numel()} ReLU decisions differ from the fp32 oracle, largest |u_oracle| {worst:.3e}')
            assert worst < NEAR, (j, bad.numel(), worst)
        flips += [(j, int(i)) for i in bad.tolist()]          # relu site j: one fc_relu per edge, in edge order
    return flips


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('prims', LISTS, ids=lambda l: '+'.join(l))
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'n%d_C%d_L%d_b%d%s' % (s[0], s[1], s[2], s[3], '_inner' if s[4] else ''))
def test_fc_edge_sum_matches_oracle(shape, prims, mode):
    from bmnas.functions import FC_KINDS
    from models.search.darts import operations as ops_mod
    n, C, L, b, inner = shape
    seed, drpt = 31, 0.1
    cfg, p, ops = build_edges(prims, n, C, L, mode, seed, drpt)
    xs, w, gw = make_case(prims, n, C, L, b, inner, seed)
    part = ops_mod.participating_primitives(prims, w.shape[1])
    n_fc = sum(q in FC_KINDS for q in part)
    xg = [x.to(dev()).requires_grad_(True) for x in xs]
    wg = w.to(dev()).requires_grad_(True)
    states = [xg[0]] * n if inner else xg
    route, _ = ops_mod.edge_sum_route(ops, states, wg, 0)
    assert route == ('fc' if n_fc else 'mixsum'), route
    with recorded_sites() as rec:
        out = ops_mod.general_edge_sum(ops, states, wg, 0)
    out.backward(gw.to(dev()))
    torch.cuda.synchronize()
    training = mode != 'eval'
    masks = None
    if mode == 'train_drop' and n_fc:
        from bmnas import lib
        assert len(rec) == n * n_fc and all(m == b * C * L for _, m in rec)
        masks = [lib.dropout_mask(d, m, dev()).cpu() for d, m in rec]
        assert 0.05 < float((masks[0] == 0).float().mean()) < 0.15
    else:
        assert rec == []
    flips = []
    if n_fc:
        assert type(out.grad_fn).__name__ == 'FcEdgeSumFnBackward'
        U = out.grad_fn.fc_U
        assert tuple(U.shape) == (n, b, n_fc * C, L)
        flips = relu_flips(prims, part, p, xs, n, inner, U)
    o_out, xo, wo, po = oracle_run(prims, cfg, p, xs, w, gw, n, inner, training,
                                   drpt if mode == 'train_drop' else 0.0, masks, flips)
    assert_close_scaled('out', out, o_out, rel=1e-4)
    for j in range(len(xs)):
        assert_close_scaled(f'dx[{j}]', xg[j].grad, xo[j].grad, rel=2e-4)
    assert_close_scaled('dw', wg.grad, wo.grad, rel=2e-4)
    for c, q in enumerate(part):
        if q == 'none':
            assert float(wg.grad[:, c].abs().max()) == 0.0
    params = dict(ops.named_parameters())
    seen = 0
    for name, t in params.items():
        j, pi = int(name.split('.')[0]), int(name.split('.')[2])
        key = 'cell._ops.' + name
        if pi < len(part):
            assert_close_scaled('grad:' + name, t.grad, po[key].grad, rel=2e-4)
            seen += 1
        else:
            assert t.grad is None and po[key].grad is None, name       # beyond the row: not evaluated (zip quirk)
    assert seen == 4 * n * n_fc
    for name, t in ops.state_dict().items():
        if fo.is_buffer(name):
            want = po['cell._ops.' + name]
            if name.endswith('num_batches_tracked'):
                assert int(t) == int(want), name
            else:
                assert_close_scaled('buf:' + name, t, want, rel=1e-4)


# ------------------------------------------------------------------------------------ launch accounting
def _one_sum(n, inner=False, prims=FULL, mode='train_drop', C=128, L=8, b=8):
    from models.search.darts import operations as ops_mod
    cfg, p, ops = build_edges(prims, n, C, L, mode, 31)
    xs, w, gw = make_case(prims, n, C, L, b, inner, 31)
    xg = [x.to(dev()).requires_grad_(True) for x in xs]
    wg = w.to(dev()).requires_grad_(True)
    states = [xg[0]] * n if inner else xg
    gwd = gw.to(dev())
    params = [t for t in ops.parameters()]

    def run():
        out = ops_mod.general_edge_sum(ops, states, wg, 0)
        out.backward(gwd)
        return out
    return run, xg, wg, params


def test_launch_count_does_not_depend_on_n(monkeypatch):
    """Counted at the Python boundary, the way tests/test_dispatch_gpu.py counts: every bmnas.lib wrapper that
    launches is wrapped; one sum issues the same launches for n = 2 and n = 9, <= 3 forward and <= 4 backward."""
    from bmnas import lib
    calls = []
    names = [k for k in dir(lib) if k.startswith('fc_edges_') and k != 'fc_edges_ok'] + ['cell_prologue']
    for k in names:
        orig = getattr(lib, k)
        monkeypatch.setattr(lib, k, (lambda o, nm: (lambda *a, **kw: (calls.append(nm), o(*a, **kw))[1]))(orig, k))
    counts = {}
    for n, inner in ((2, True), (9, False)):
        run, *_ = _one_sum(n, inner)
        calls.clear()
        before = dict(lib.FC_EDGE_LAUNCHES)
        run()
        torch.cuda.synchronize()
        launches = [c for c in calls if c != 'fc_edges_zero']           # fc_edges_zero IS its cell_prologue call
        fwd = lib.FC_EDGE_LAUNCHES['fwd'] - before['fwd']
        bwd = lib.FC_EDGE_LAUNCHES['bwd'] - before['bwd']
        assert fwd + bwd == len(launches), (launches, fwd, bwd)
        assert fwd <= 3 and bwd <= 4, (fwd, bwd)
        counts[n] = launches
    assert counts[2] == counts[9], counts


OURS = ('fc_gemm_fwd_k', 'fc_mix_fwd_k', 'fc_bwd_reduce_k', 'fc_bwd_du_k', 'fc_bwd_gemm_k', 'prologue')


@pytest.mark.parametrize('n,inner', [(2, True), (6, False), (9, False)])
def test_function_runs_only_library_kernels(n, inner):
    """torch.profiler over forward + backward of the Function alone: every device kernel is one of
    libbmnas_hip.so's (the csrc/ kernels fc_*_k and the prologue's zero-fill), no memcpy, no aten kernel — and the
    device sees the same 3 + 4 launches for n = 2, 6 and 9."""
    from models.search.darts import operations as ops_mod
    prims = FULL[:2] if inner else FULL
    cfg, p, ops = build_edges(FULL, n, 128, 8, 'train_drop', 31)
    xs, w, gw = make_case(FULL, n, 128, 8, 8, inner, 31)
    xg = [x.to(dev()).requires_grad_(True) for x in xs]
    wg = w.to(dev()).requires_grad_(True)
    gwd = gw.to(dev())
    states = [xg[0]] * n if inner else xg
    reached = [t for k, t in ops.named_parameters() if int(k.split('.')[2]) < len(prims)]
    leaves = xg + [wg] + reached

    def run():
        out = ops_mod.fc_edge_sum_apply(ops, states, wg, prims)
        return torch.autograd.grad(out, leaves, gwd)
    assert all(g is not None for g in run())
    torch.cuda.synchronize()
    names = device_kernels(run)
    foreign = [k for k in names if not any(s in k for s in OURS)]
    assert not foreign, foreign
    assert [next(s for s in OURS if s in k) for k in names] == \
        ['prologue', 'fc_gemm_fwd_k', 'fc_mix_fwd_k', 'prologue', 'fc_bwd_reduce_k', 'fc_bwd_du_k', 'fc_bwd_gemm_k'], names


def test_unsupported_shapes_are_refused_and_fall_back():
    from bmnas import lib
    from models.search.darts import operations as ops_mod
    assert lib.fc_edges_ok(6, 2, 4, 128, 192, 16) and lib.fc_edges_ok(2, 1, 2, 8, 128, 8)
    assert not lib.fc_edges_ok(16, 2, 4, 8, 128, 8)          # more edges than the cell's limit
    assert not lib.fc_edges_ok(6, 2, 4, 8, 128, 32)          # L outside {4, 8, 16}
    assert not lib.fc_edges_ok(6, 2, 4, 8, 24, 8)            # C % 16
    assert not lib.fc_edges_ok(6, 3, 4, 8, 128, 8)
    cfg, p, ops = build_edges(FULL, 3, 24, 8, 'eval', 31)    # C = 24: composed, same numbers as the oracle
    xs, w, gw = make_case(FULL, 3, 24, 8, 5, False, 31)
    xg = [x.to(dev()) for x in xs]
    assert ops_mod.edge_sum_route(ops, xg, w.to(dev()), 0)[0] == 'composed'
    out = ops_mod.general_edge_sum(ops, xg, w.to(dev()), 0)
    want = sum(fo.mixed_edge_general(h, w[j], p, f'cell._ops.{j}', FULL, False, 0.0) for j, h in enumerate(xs))
    assert_close_scaled('out', out, want)
