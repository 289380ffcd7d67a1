"""-m gpu: NodeMixedOp over an edited STEP_STEP_PRIMITIVES list on the selected-term kernels of csrc/nodemix_sel.hip
(bmnas.functions.NodeMixedSelFn, reached through node_operations.node_mix_route) against the CPU oracle
(node_prims_util.node_mixed_general: fo.op_sum / op_scaled_dot_attn / op_linear_glu / op_concat_fc in list order),
the launch accounting of that path, its refusals, and that the default list is untouched.

ReLU decisions of ConcatFC (the protocol of tests/test_fc_edges_gpu.py): the kernel's pre-activation — its stored conv
output under its stored BatchNorm affine — is read back; every element whose sign disagrees with the fp32 oracle's must
have |u_oracle| < 2e-5, and the gradients are then compared, every element, against the oracle evaluated under exactly
those decisions (fo.relu_decisions(flips=...)).  The seeds of node_prims_util.case_seed were checked on the CPU with the
oracle alone, in fp32 and in float64: no ConcatFC pre-activation of any case below lies within 2e-5 of zero
(node_prims_util.SEED_SALT moves a case to the next seed where one did; test_seeds_keep_relu_inputs_away_from_zero
repeats the check)."""
import numpy as np
import pytest
import torch

from oracle import fusion_oracle as fo
from fc_edges_util import device_kernels, recorded_sites
from gpu_util import Args, assert_close_scaled, dev, set_mode
from node_prims_util import (KINDS, NEAR, PERMUTATIONS, PREFIX, SUBSETS, edited_step_prims, fc_preactivation, list_id,
                             make_case, min_fc_margin, oracle_op)

pytestmark = pytest.mark.gpu

SUBSET_SHAPES = [(4, 16, 8, True), (5, 16, 8, False)]
# (b, C, L, same, training)
PERM_SHAPES = [(6, 48, 4, True, True), (3, 32, 16, True, False), (6, 192, 16, True, True), (7, 128, 8, False, True)]
LIVE = ['ConcatFC', 'ScaleDotAttn', 'Sum', 'LinearGLU']


def shape_id(s):
    return 'b%d_C%d_L%d_%s%s' % (s[0], s[1], s[2], 'same' if s[3] else 'xy', '' if len(s) < 5 or s[4] else '_eval')


def build_op(prims, p, C, L, mode, drpt=0.0):
    from models.search.darts.node_operations import NodeMixedOp
    cfg = fo.make_cfg(N=2, C=C, L=L, S=1, M=1, ns=1, nm=1, drpt=drpt)
    with edited_step_prims(prims):
        op = NodeMixedOp(C, L, Args(cfg, drpt))
    sd = {k[len('op.'):]: v.clone() for k, v in p.items()}
    assert list(sd) == list(op.state_dict())
    op.load_state_dict(sd)
    op.to(dev())
    set_mode(op, mode)
    return op


def run_hip(op, x, y, gamma, g, same):
    xd = x.to(dev()).requires_grad_(True)
    yd = xd if same else y.to(dev()).requires_grad_(True)
    wd = gamma.to(dev()).requires_grad_(True)
    out = op(xd, yd, wd)
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    return out, xd, yd, wd


def kernel_flips(prims, out, p, x, y, training):
    """(site, flat index) of every ConcatFC pre-activation the kernel put on the other side of zero than the fp32
    oracle; asserts each of them is within NEAR of zero in the oracle."""
    if 'ConcatFC' not in prims:
        return []
    sv = out.grad_fn.sv
    C = x.shape[1]
    M = sv.conv.M
    lo = 2 * C if 'LinearGLU' in prims else 0
    U = sv.conv.U[:, lo:lo + C, :].double().cpu()
    chan = sv.conv.chan.double().cpu()
    u_k = (U * chan[2 * M + lo:2 * M + lo + C][None, :, None] + chan[3 * M + lo:3 * M + lo + C][None, :, None]).reshape(-1)
    u_or = fc_preactivation(x, y, p, f'{PREFIX}.{prims.index("ConcatFC")}', training).reshape(-1)
    assert_close_scaled('ConcatFC pre-activation', u_k, u_or)
    bad = torch.nonzero((u_k > 0) != (u_or > 0)).reshape(-1)
    if bad.numel():
        worst = float(u_or[bad].abs().max())
        print(f'{bad.numel()} ReLU decisions differ from the fp32 oracle, largest |u_oracle| {worst:.3e}')
        assert worst < NEAR, (bad.numel(), worst)
    return [(0, int(i)) for i in bad.tolist()]              # one ReLU site: ConcatFC's


def check_case(prims, b, C, L, same, training, mode=None, drpt=0.0):
    """One forward + backward of the module against the oracle -> (op, out) for further checks."""
    import models.search.darts.node_operations as no
    from bmnas import lib
    p, x, y, gamma, g = make_case(prims, b, C, L, same)
    mode = mode or ('train_nodrop' if training else 'eval')
    op = build_op(prims, p, C, L, mode, drpt)
    xd = x.to(dev())
    assert no.node_mix_route(op, xd, xd if same else y.to(dev()), gamma.to(dev())) == 'selected'
    before = dict(lib.NODE_SEL_LAUNCHES)
    with recorded_sites() as rec:
        out, xd, yd, wd = run_hip(op, x, y, gamma, g, same)
    assert type(out.grad_fn).__name__ == 'NodeMixedSelFnBackward'
    assert lib.NODE_SEL_LAUNCHES['fwd'] - before['fwd'] == 1 and lib.NODE_SEL_LAUNCHES['bwd'] - before['bwd'] == 1
    masks, attn_drop = None, 0.0
    if mode == 'train':
        owners = [q for q in prims if q != 'Sum']
        assert len(rec) == len(owners) and all(m == b * C * L for _, m in rec)
        masks = [lib.dropout_mask(d, m, dev()).cpu() for d, m in rec]
        for q, m in zip(owners, masks):                     # list order: each site carries its owner's rate
            want = 0.1 if q == 'ScaleDotAttn' else drpt
            assert abs(float((m == 0).float().mean()) - want) < 0.03, (q, float((m == 0).float().mean()))
            keep = m[m != 0]
            assert_close_scaled('kept multiplier of ' + q, keep, torch.full_like(keep, 1.0 / (1.0 - want)))
        attn_drop = 0.1
    else:
        assert rec == []
    flips = kernel_flips(prims, out, p, x, y, training)
    o_out, o_dw, o_dx, o_dy, po = oracle_op(prims, p, x, y, gamma, g, same, training, drpt if masks else 0.0, attn_drop,
                                            masks, flips)
    assert_close_scaled('out', out, o_out, rel=1e-4)
    assert tuple(wd.grad.shape) == (len(prims),)
    assert_close_scaled('dgamma', wd.grad, o_dw, rel=2e-4)
    assert_close_scaled('dx', xd.grad, o_dx, rel=2e-4)
    if not same:
        assert_close_scaled('dy', yd.grad, o_dy, rel=2e-4)
    seen = 0
    for k, v in op.named_parameters():
        want = po['op.' + k].grad
        if k.endswith('conv.bias') and training:            # in front of a train-mode BatchNorm: zero up to round-off
            assert float(v.grad.abs().max()) < 1e-4, k
        else:
            assert_close_scaled('d' + k, v.grad, want, rel=2e-4)
        seen += 1
    assert seen == 2 * ('ScaleDotAttn' in prims) + 4 * ('LinearGLU' in prims) + 4 * ('ConcatFC' in prims)
    for k, v in op.state_dict().items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == (1 if training else 0), k
        elif fo.is_buffer(k):
            assert_close_scaled(k, v.float(), po['op.' + k].float(), rel=1e-4)
    return op, out


def test_seeds_keep_relu_inputs_away_from_zero():
    """The CPU oracle alone, fp32 and float64: no ConcatFC pre-activation of any case of this file within 2e-5 of 0."""
    cases = [(s, *sh, True) for s in SUBSETS for sh in SUBSET_SHAPES] + [(s, *sh) for s in PERMUTATIONS for sh in PERM_SHAPES]
    cases.append((LIVE, 8, 32, 16, True, True))
    for prims, b, C, L, same, training in cases:
        p, x, y, _, _ = make_case(prims, b, C, L, same)
        assert min_fc_margin(prims, p, x, y, training) > NEAR, (prims, b, C, L, same)


@pytest.mark.parametrize('shape', SUBSET_SHAPES, ids=shape_id)
@pytest.mark.parametrize('prims', SUBSETS, ids=list_id)
def test_every_subset_matches_oracle(prims, shape):
    """All 15 non-empty subsets in canonical order; 32 float4 slots are less than one 64-slot block, and a batch of 5
    is no multiple of the backward's four sample lanes.  (The full list in canonical order IS the default list: it
    stays on its own path and is compared there by tests/test_kernels_gpu.py::test_node_mixed_op.)"""
    if prims == KINDS:
        import models.search.darts.node_operations as no
        p, x, y, gamma, g = make_case(prims, *shape)
        op = build_op(prims, p, shape[1], shape[2], 'train_nodrop')
        xd = x.to(dev())
        assert no.node_mix_route(op, xd, xd, gamma.to(dev())) == 'default'
        return
    check_case(prims, *shape, True)


@pytest.mark.parametrize('shape', PERM_SHAPES, ids=shape_id)
@pytest.mark.parametrize('prims', PERMUTATIONS, ids=list_id)
def test_permutations_match_oracle(prims, shape):
    """L / 4 = 1 (a one-lane channel row), eval mode, several column blocks, x != y with a 7-sample tail."""
    check_case(prims, *shape)


def test_all_four_in_another_order_takes_the_stacked_storage():
    """Both convs present and LinearGLU BEHIND ConcatFC in the list: the stacked GEMM still has the LinearGLU rows
    first, the modules are found by kind and state_dict keys by list position."""
    prims = ['ConcatFC', 'ScaleDotAttn', 'LinearGLU', 'Sum']
    op, out = check_case(prims, 6, 64, 16, True, True)
    st = op._stack
    assert st is not None and op._ops[2].conv.weight.data_ptr() == st.W.data_ptr()
    assert op._ops[0].conv.weight.data_ptr() == st.W[2 * 64:].data_ptr()
    assert out.grad_fn.sv.conv.M == 3 * 64


def test_live_dropout_sites_in_list_order():
    """All three dropout owners in a non-default order: three Philox sites in list order (ConcatFC, ScaleDotAttn,
    LinearGLU), the masks exported and injected into the oracle at the same positions."""
    check_case(LIVE, 8, 32, 16, True, True, mode='train', drpt=0.2)


def test_native_and_composed_issue_the_same_dropout_sites():
    """From the same Philox offset both paths issue the same site descriptors, in list order: the same seed gives both
    the same masks."""
    import models.search.darts.node_operations as no
    from bmnas import cell as K
    b, C, L = 8, 32, 16
    p, x, y, gamma, g = make_case(LIVE, b, C, L, True)
    op = build_op(LIVE, p, C, L, 'train', 0.2)
    xd, wd = x.to(dev()), gamma.to(dev())
    sites = {}
    start = K.DROP.offset
    for native in (True, False):
        K.DROP.offset = start
        no.NODE_PRIMS_NATIVE = native
        try:
            assert no.node_mix_route(op, xd, xd, wd) == ('selected' if native else 'composed')
            with recorded_sites() as rec:
                op(xd, xd, wd)
        finally:
            no.NODE_PRIMS_NATIVE = True
        sites[native] = [(d.thr, d.scale, d.seed, d.offset, d.step, n) for d, n in rec]
    assert len(sites[True]) == 3 and sites[True] == sites[False]
    assert [s[0] for s in sites[True]] == [int(q * 4294967296.0) for q in (0.2, 0.1, 0.2)]


# ------------------------------------------------------------------------------------ route and launches
def _runner(prims, b, C, L, same, native=True):
    import models.search.darts.node_operations as no
    p, x, y, gamma, g = make_case(prims, b, C, L, same)
    op = build_op(prims, p, C, L, 'train_nodrop')
    xd = x.to(dev()).requires_grad_(True)
    yd = xd if same else y.to(dev()).requires_grad_(True)
    wd, gd = gamma.to(dev()).requires_grad_(True), g.to(dev())

    def run():
        no.NODE_PRIMS_NATIVE = native
        try:
            out = op(xd, yd, wd)
            out.backward(gd)
        finally:
            no.NODE_PRIMS_NATIVE = True
        return out
    run()                                                   # warm-up: stacked storage, lazy allocations
    torch.cuda.synchronize()
    return run


_DEFAULT_EVENTS = {}


def default_events(b, C, L, same):
    key = (b, C, L, same)
    if key not in _DEFAULT_EVENTS:
        _DEFAULT_EVENTS[key] = device_kernels(_runner(KINDS, b, C, L, same))
    return _DEFAULT_EVENTS[key]


def is_library_kernel(name):
    """Not an aten kernel, a memcpy / memset or the runtime's own fill / copy kernel (a torch.zeros shows up as one):
    the same notion of 'foreign' as tests/test_graph_forward_gpu.py."""
    return not ('at::' in name or 'Memcpy' in name or 'Memset' in name or 'rocclr' in name)


def base(name):
    """The kernel's own name: no return type, namespace, template arguments or parameter list
    ('void (anonymous namespace)::node_mix_sel_fwd_k<1>(float const*, ...)' -> 'node_mix_sel_fwd_k')."""
    n = name.replace('(anonymous namespace)::', '')
    if n.startswith('void '):
        n = n[len('void '):]
    return n.split('(')[0].split('<')[0].strip()


COUNT_CASES = [(s, 4, 16, 8, True) for s in SUBSETS if s != KINDS] + [(s, 6, 192, 16, True) for s in PERMUTATIONS] + \
              [(s, 7, 128, 8, False) for s in PERMUTATIONS]


@pytest.mark.parametrize('prims,b,C,L,same', COUNT_CASES, ids=lambda v: list_id(v) if isinstance(v, list) else str(v))
def test_device_events_against_default_and_composed(prims, b, C, L, same):
    """torch.profiler over forward + backward: the selected path issues no more device events than the default list at
    the same shape and strictly fewer than the same list composed; no GEMM / BatchNorm kernel without a conv, no
    attention kernel without ScaleDotAttn, and ['Sum'] is one kernel of this library per direction."""
    from bmnas import lib
    native = device_kernels(_runner(prims, b, C, L, same))
    before = dict(lib.NODE_SEL_LAUNCHES)
    composed = device_kernels(_runner(prims, b, C, L, same, native=False))
    assert lib.NODE_SEL_LAUNCHES == before                  # the composed sum issues none of the new launches
    default = default_events(b, C, L, same)
    print(f'{list_id(prims)} {(b, C, L, same)}: native {len(native)}, default list {len(default)}, composed {len(composed)}')
    assert len(native) <= len(default), (native, default)
    assert len(native) < len(composed), (native, composed)
    ours = [base(k) for k in native if is_library_kernel(k)]
    assert sum('node_mix_sel_fwd_k' in k for k in ours) == 1 and sum('node_mix_sel_bwd_k' in k for k in ours) == 1
    if not {'LinearGLU', 'ConcatFC'} & set(prims):
        assert not [k for k in ours if 'conv' in k or 'bn_' in k or 'fold' in k], ours
    if 'ScaleDotAttn' not in prims:
        assert not [k for k in ours if 'sdpa' in k or 'ln_affine' in k], ours
    if prims == ['Sum']:
        assert len(ours) == 2, ours


# ------------------------------------------------------------------------------------------- refusals
def test_shapes_outside_the_limits_are_refused_and_compose():
    import models.search.darts.node_operations as no
    from bmnas import lib
    ok = lib.node_mix_sel_ok
    assert ok(0b0011, 4, 16, 8) and ok(0b0001, 3, 5, 12) and ok(0b1101, 128, 192, 16) and ok(0b0010, 2, 512, 4)
    assert not ok(0b0011, 4, 16, 6)                         # attention: L of 4, 8 or 16
    assert not ok(0b0001, 4, 16, 6) and not ok(0b0001, 4, 16, 0)      # L % 4
    assert not ok(0b0010, 4, 528, 8)                        # attention: C <= 512
    assert not ok(0b1000, 4, 24, 8) and not ok(0b0100, 4, 16, 12)     # the conv GEMM's tiles
    assert not ok(0, 4, 16, 8) and not ok(16, 4, 16, 8) and not ok(1, 0, 16, 8)
    # L = 6 with attention: composed, and the C entry point refuses before anything is launched
    prims = ['Sum', 'ScaleDotAttn']
    p, x, y, gamma, g = make_case(prims, 4, 16, 6, True)
    op = build_op(prims, p, 16, 6, 'eval')
    xd, wd = x.to(dev()), gamma.to(dev())
    assert no.node_mix_route(op, xd, xd, wd) == 'composed'
    out = torch.full_like(xd, 7.0)
    before = dict(lib.NODE_SEL_LAUNCHES)
    sel = lib.make_node_sel(prims)
    with pytest.raises(lib.BmnasError, match='limit exceeded'):
        lib.node_mix_sel_fwd(xd, xd, xd, None, None, wd, sel, out, 4, 16, 6)
    dg, dx = torch.zeros(2, device=dev()), torch.full_like(xd, 7.0)
    with pytest.raises(lib.BmnasError, match='limit exceeded'):
        lib.node_mix_sel_bwd(xd, xd, xd, xd, None, None, wd, sel, dg, dx, None, 0, None, None, 4, 16, 6)
    torch.cuda.synchronize()
    assert lib.NODE_SEL_LAUNCHES == before
    assert float(out.min()) == 7.0 and float(dx.min()) == 7.0 and float(dg.abs().max()) == 0.0
    # a conv list at C = 24 composes and computes what the oracle computes
    prims = ['ConcatFC', 'Sum']
    p, x, y, gamma, g = make_case(prims, 4, 24, 8, False)
    op = build_op(prims, p, 24, 8, 'eval')
    xd, yd, wd = x.to(dev()), y.to(dev()), gamma.to(dev())
    assert no.node_mix_route(op, xd, yd, wd) == 'composed'
    # a bad descriptor is a bad argument, not a launch
    bad = lib.NodeSel((lib.C.c_int * 4)(0, 0, -1, -1), 2)
    with pytest.raises(lib.BmnasError, match='bad argument'):
        lib.node_mix_sel_fwd(xd, xd, xd, None, None, wd, bad, torch.empty_like(xd), 4, 24, 8)


# ------------------------------------------------------------------------------ in-kernel BatchNorm finalisation
@pytest.mark.parametrize('prims', [['Sum', 'ConcatFC'], ['LinearGLU'], ['ConcatFC', 'ScaleDotAttn', 'LinearGLU']], ids=list_id)
def test_forward_finalises_the_batchnorm_in_kernel(prims):
    """bmnas_bn_fin_t on = 1 (the GEMM accumulates batch sums, the combine finalises them, updates the running
    statistics and the one or two num_batches_tracked counters) against on = 0 (bmnas_bn_finalize in front)."""
    from bmnas import cell as K
    from bmnas import lib
    b, C, L = 6, 48, 8
    p, x, y, gamma, g = make_case(prims, b, C, L, True)
    outs, bufs = [], []
    for on in (0, 1):
        op = build_op(prims, p, C, L, 'train_nodrop')
        P = op.pack()
        xd, wd = x.to(dev()), gamma.to(dev())
        stats = None
        if on:
            stats = K.StatArena(xd, [P.M], torch.zeros(K.StatArena.numel_for([P.M]), device=dev()))
        Weff = torch.empty(P.M, C, device=dev())
        lib.fold_weight(P.stack_W, Weff, P.M, C)
        U, chan, sv = K.conv_bn_fwd([xd], C, Weff, C, P.stack_bias, P.stack_bn_w, P.stack_bn_b, P.stack_rm, P.stack_rv,
                                    P.stack_nbt, True, dup=C, stats=stats)
        assert sv.fin.on == on
        p1 = torch.randn(b, C, L, generator=torch.Generator().manual_seed(3)).to(dev()) if 'ScaleDotAttn' in prims else None
        out = torch.empty_like(xd)
        has_sum = 'Sum' in prims
        lib.node_mix_sel_fwd(xd if has_sum else None, xd if has_sum else None, p1, U, chan, wd, lib.make_node_sel(prims),
                             out, b, C, L, fin=sv.fin)
        torch.cuda.synchronize()
        outs.append(out)
        bufs.append({k: v.clone() for k, v in op.state_dict().items() if fo.is_buffer(k)})
        bufs[-1]['chan'] = chan
    assert_close_scaled('out', outs[1], outs[0], rel=1e-4)
    for k, v in bufs[0].items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == 1 and int(bufs[1][k]) == 1, k
        else:
            assert_close_scaled(k, bufs[1][k], v, rel=1e-4)


# ---------------------------------------------------------------------------------- the default list is untouched
def test_default_list_is_bit_identical_whatever_the_switch():
    """(4, 16, 8): one workgroup per reduction, so the default path is reproducible to the bit; it must not notice
    NODE_PRIMS_NATIVE."""
    import models.search.darts.node_operations as no
    from bmnas import lib
    b, C, L = 4, 16, 8
    p, x, y, gamma, g = make_case(KINDS, b, C, L, True)
    results, names = [], []
    before = dict(lib.NODE_SEL_LAUNCHES)
    for native in (True, False, True):
        op = build_op(KINDS, p, C, L, 'train_nodrop')
        no.NODE_PRIMS_NATIVE = native
        try:
            xd = x.to(dev())
            assert no.node_mix_route(op, xd, xd, gamma.to(dev())) == 'default'
            out, xd, yd, wd = run_hip(op, x, y, gamma, g, True)
            res = [out.detach(), xd.grad, wd.grad] + [t.grad for t in op.parameters()] + \
                  [v for k, v in op.state_dict().items() if fo.is_buffer(k)]

            def again():
                o = op(xd, xd, wd)
                o.backward(g.to(dev()))
            names.append(device_kernels(again))
        finally:
            no.NODE_PRIMS_NATIVE = True
        assert type(out.grad_fn).__name__ == 'NodeMixedFnBackward'
        results.append([t.clone() for t in res])
    assert lib.NODE_SEL_LAUNCHES == before
    for other in results[1:]:
        assert len(other) == len(results[0])
        for a, b_ in zip(results[0], other):
            assert torch.equal(a, b_)
    assert names[0] == names[1] == names[2]
