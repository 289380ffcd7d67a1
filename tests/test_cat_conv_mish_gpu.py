"""-m gpu: the CatConvMish step-node primitive (reference models/search/darts/node_operations.py:58-82) on the gfx950
kernels — in the FC slot of the selected-term mix (csrc/nodemix_sel.hip with ACT = Mish, reached through
node_operations.node_mix_route) and as the standalone op (bmnas_bn_mish_fwd / _bwd of csrc/bnmix.hip behind the conv
GEMM) — against the CPU restatement of cat_conv_mish_util (pinned to the reference by tests/test_cat_conv_mish_host.py).

Mish is smooth: no ReLU-decision protocol, every element of every tensor is compared.  Tolerances are the project's:
1e-4 of scale for outputs and buffers, 2e-4 for gradients (gpu_util.assert_close_scaled)."""
import numpy as np
import pytest
import torch

import cat_conv_mish_util as cm
from cat_conv_mish_util import LIVE, MISH, PERMUTATIONS, SUBSETS, list_id
from fc_edges_util import device_kernels, recorded_sites
from gpu_util import Args, assert_close_scaled, dev, set_mode
from oracle import fusion_oracle as fo

pytestmark = pytest.mark.gpu

SUBSET_SHAPES = [(4, 16, 8, True), (5, 16, 8, False)]
# (b, C, L, same, training): the shapes of tests/test_node_prims_gpu.py
PERM_SHAPES = [(6, 48, 4, True, True), (3, 32, 16, True, False), (6, 192, 16, True, True), (7, 128, 8, False, True)]


def shape_id(s):
    return 'b%d_C%d_L%d_%s%s' % (s[0], s[1], s[2], 'same' if s[3] else 'xy', '' if len(s) < 5 or s[4] else '_eval')


def seed_of(prims, b, C, L, same):
    return 4100 + 17 * sum((i + 1) * (cm.BUILTIN4.index(q) + 1) for i, q in enumerate(prims)) + b + C + L + same


def build_op(prims, p, C, L, mode, drpt=0.0):
    from models.search.darts.node_operations import NodeMixedOp
    cfg = fo.make_cfg(N=2, C=C, L=L, S=1, M=1, ns=1, nm=1, drpt=drpt)
    with cm.mish_list(prims):
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


def compare(op, training, out, xd, yd, wd, same, want):
    o_out, o_dw, o_dx, o_dy, po = want
    assert_close_scaled('out', out, o_out, rel=1e-4)
    if wd is not None:
        assert_close_scaled('dgamma', wd.grad, o_dw, rel=2e-4)
    assert_close_scaled('dx', xd.grad, o_dx, rel=2e-4)
    if not same:
        assert_close_scaled('dy', yd.grad, o_dy, rel=2e-4)
    seen = 0
    for k, v in op.named_parameters():
        if k.endswith('conv.bias') and training:            # in front of a train-mode BatchNorm: zero up to round-off
            assert float(v.grad.abs().max()) < 1e-4, k
        else:
            assert_close_scaled('d' + k, v.grad, po['op.' + k].grad, rel=2e-4)
        seen += 1
    for k, v in op.state_dict().items():
        if k.endswith('num_batches_tracked'):
            assert int(v) == (1 if training else 0), k
        elif fo.is_buffer(k):
            assert_close_scaled(k, v.float(), po['op.' + k].float(), rel=1e-4)
    return seen


def check_case(prims, b, C, L, same, training, mode=None, drpt=0.0):
    import models.search.darts.node_operations as no
    from bmnas import lib
    p, x, y, gamma, g = cm.make_case(prims, b, C, L, same, seed_of(prims, b, C, L, same))
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
    want = cm.oracle_op(prims, p, x, y, gamma, g, same, training, drpt if masks else 0.0, attn_drop, masks)
    assert tuple(wd.grad.shape) == (len(prims),)
    seen = compare(op, training, out, xd, yd, wd, same, want)
    assert seen == 2 * ('ScaleDotAttn' in prims) + 4 * ('LinearGLU' in prims) + 4
    return op, out


# ------------------------------------------------------------------------------------------ one NodeMixedOp
@pytest.mark.parametrize('shape', SUBSET_SHAPES, ids=shape_id)
@pytest.mark.parametrize('prims', SUBSETS, ids=list_id)
def test_every_fc_slot_subset_matches_restatement(prims, shape):
    """The 8 subsets with CatConvMish in canonical order — the four-entry one is NOT the default list and takes the
    selected path too; 32 float4 slots are less than one 64-slot block, 5 samples no multiple of the four lanes."""
    op, _ = check_case(prims, *shape, True)
    assert not op._default


@pytest.mark.parametrize('shape', PERM_SHAPES, ids=shape_id)
@pytest.mark.parametrize('prims', PERMUTATIONS, ids=list_id)
def test_permutations_match_restatement(prims, shape):
    """L / 4 = 1 (a one-lane channel row), eval mode, several column blocks, x != y with a 7-sample tail.  With both
    convs in the list the stacked storage holds the LinearGLU rows first, whatever the list order."""
    op, out = check_case(prims, *shape)
    if 'LinearGLU' in prims:
        C = shape[1]
        st = op._stack
        assert st is not None and op._ops[0].conv.weight.data_ptr() == st.W.data_ptr()
        assert op._ops[1].conv.weight.data_ptr() == st.W[2 * C:].data_ptr()
        assert out.grad_fn.sv.conv.M == 3 * C


def test_live_dropout_sites_in_list_order():
    """Three Philox sites in list order (CatConvMish, ScaleDotAttn, LinearGLU) with their owners' rates; the masks are
    exported and injected into the restatement at the same positions."""
    check_case(LIVE, 8, 32, 16, True, True, mode='train', drpt=0.2)


def test_native_and_composed_issue_the_same_dropout_sites():
    import models.search.darts.node_operations as no
    from bmnas import cell as K
    b, C, L = 8, 32, 16
    p, x, y, gamma, g = cm.make_case(LIVE, b, C, L, True, seed_of(LIVE, b, C, L, True))
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


def _runner(prims, b, C, L, native=True):
    import models.search.darts.node_operations as no
    p, x, y, gamma, g = cm.make_case(prims, b, C, L, True, seed_of(cm.BUILTIN4, b, C, L, True))
    op = build_op(prims, p, C, L, 'train_nodrop')
    xd = x.to(dev()).requires_grad_(True)
    wd, gd = gamma.to(dev()).requires_grad_(True), g.to(dev())

    def run():
        no.NODE_PRIMS_NATIVE = native
        try:
            op(xd, xd, wd).backward(gd)
        finally:
            no.NODE_PRIMS_NATIVE = True
    run()                                                   # warm-up: stacked storage, lazy allocations
    torch.cuda.synchronize()
    return run


def test_device_events_against_concat_fc_and_composed():
    """torch.profiler over forward + backward at b6 C64 L16: no more device events than the same list with ConcatFC in
    the slot, strictly fewer than the same list composed (whose CatConvMish is the standalone native op)."""
    b, C, L = 6, 64, 16
    native = device_kernels(_runner(cm.BUILTIN4, b, C, L))
    relu = device_kernels(_runner(['Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC'], b, C, L))     # (the default list)
    composed = device_kernels(_runner(cm.BUILTIN4, b, C, L, native=False))
    print(f'native {len(native)}, ConcatFC in the slot {len(relu)}, composed {len(composed)}')
    assert len(native) <= len(relu), (native, relu)
    assert len(native) < len(composed), (native, composed)
    assert sum('node_mix_sel_fwd_k' in k for k in native) == 1 and sum('node_mix_sel_bwd_k' in k for k in native) == 1
    assert any('bn_mish_fwd_k' in k for k in composed) and any('bn_mish_bwd_k' in k for k in composed)
    assert not [k for k in composed if 'at::native' in k and ('softplus' in k or 'tanh' in k)], composed


def test_c_abi_refuses_an_unknown_activation():
    from bmnas import lib
    b, C, L = 4, 16, 8
    x = torch.zeros(b, C, L, device=dev())
    w = torch.ones(2, device=dev())
    out = torch.full_like(x, 7.0)
    before = dict(lib.NODE_SEL_LAUNCHES)
    with pytest.raises(lib.BmnasError, match='bad argument'):
        lib.node_mix_sel_fwd(x, x, None, x, torch.zeros(4 * C, device=dev()), w, lib.make_node_sel(['Sum', 'ConcatFC']),
                             out, b, C, L, fc_act=2)
    torch.cuda.synchronize()
    assert lib.NODE_SEL_LAUNCHES == before and float(out.min()) == 7.0


# ------------------------------------------------------------------------------------------- Mish regimes
SEGMENTS = [(-100.0, -20.0), (-20.0, -5.0), (-5.0, 5.0), (5.0, 20.5), (20.5, 100.0)]


def identity_params(prims, C, L):
    """Eval-mode parameters under which CatConvMish's pre-activation IS its first input: conv = [I | 0], no bias,
    running mean 0 / var 1, bn.weight = sqrt(1 + eps)."""
    p = {k: torch.zeros(s) for k, s in cm.op_param_shapes(prims, C, L, cm.PREFIX).items()}
    pre = f'{cm.PREFIX}.{prims.index(MISH)}'
    p[pre + '.conv.weight'][:, :C, 0] = torch.eye(C)
    p[pre + '.bn.running_var'].fill_(1.0)
    p[pre + '.bn.weight'].fill_(float(np.sqrt(np.float64(1.0) + 1e-5)))
    p[pre + '.bn.num_batches_tracked'] = torch.zeros((), dtype=torch.long)
    return p


@pytest.mark.parametrize('prims', [[MISH], ['Sum', MISH]], ids=list_id)
def test_mish_regimes_against_float64(prims):
    """A ramp over each of the five segments of the fp32 formula (q / (q + 2), its u > 20 branch, the clamp of the
    exponential) as the pre-activation of a (5, 16, 16) input, sample by segment: forward and backward against the
    float64 restatement, per segment, at the standard tolerances; everything finite; |out| <= 1e-6 for u <= -20;
    out = u and dx = g to 1e-6 relative for u > 20.  [CatConvMish] alone is the standalone op (bn_mish kernels),
    ['Sum', 'CatConvMish'] the mix kernels (Sum weighted 0 so that the Mish term is what is compared)."""
    import models.search.darts.node_operations as no
    C, L = 16, 16
    n = C * L
    u = torch.stack([torch.linspace(lo, hi, n, dtype=torch.float64) for lo, hi in SEGMENTS]).reshape(5, C, L).float()
    y = torch.from_numpy(np.random.Generator(np.random.PCG64(5)).standard_normal((5, C, L)).astype(np.float32))
    g = torch.from_numpy(np.random.Generator(np.random.PCG64(6)).standard_normal((5, C, L)).astype(np.float32))
    p = identity_params(prims, C, L)
    op = build_op(prims, p, C, L, 'eval')
    mix = len(prims) > 1
    gamma = torch.tensor([0.0, 1.0]) if mix else torch.ones(1)
    xd, yd = u.to(dev()).requires_grad_(True), y.to(dev()).requires_grad_(True)
    if mix:
        wd = gamma.to(dev())
        assert no.node_mix_route(op, xd, yd, wd) == 'selected'
        out = op(xd, yd, wd)
        assert type(out.grad_fn).__name__ == 'NodeMixedSelFnBackward'
    else:
        out = op._ops[0](xd, yd)
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    o64, _, dx64, dy64, _ = cm.oracle_op(prims, p, u, y, gamma, g, False, False, double=True)
    # the pre-activation of the restatement is the ramp (fp32 round-off of sqrt(1 + eps) / sqrt(1 + eps) aside)
    assert torch.isfinite(out).all() and torch.isfinite(xd.grad).all() and torch.isfinite(yd.grad).all()
    for s, (lo, hi) in enumerate(SEGMENTS):
        assert_close_scaled(f'out [{lo}, {hi}]', out[s], o64[s], rel=1e-4)
        assert_close_scaled(f'dx [{lo}, {hi}]', xd.grad[s], dx64[s], rel=2e-4)
    assert float(yd.grad.abs().max()) == 0.0 and float(dy64.abs().max()) == 0.0      # the zero half of the conv
    oc, dxc, uc, gc = out.detach().cpu().double(), xd.grad.cpu().double(), u.double(), g.double()
    low = uc <= -20.0
    assert float(oc[low].abs().max()) <= 1e-6
    high = uc > 20.0
    assert float(((oc[high] - uc[high]).abs() / uc[high].abs()).max()) <= 1e-6
    assert float(((dxc[high] - gc[high]).abs() / gc[high].abs().clamp_min(1e-30)).max()) <= 1e-6


# ------------------------------------------------------------------------------------------ standalone op
def build_alone(p, C, L, mode, drpt=0.0):
    from models.search.darts.node_operations import CatConvMish
    cfg = fo.make_cfg(N=2, C=C, L=L, S=1, M=1, ns=1, nm=1, drpt=drpt)
    m = CatConvMish(C, Args(cfg, drpt))
    m.load_state_dict({k[len(cm.PREFIX) + 3:]: v.clone() for k, v in p.items()})
    m.to(dev())
    set_mode(m, mode)
    return m


class _Holder(torch.nn.Module):
    """compare() walks `op.named_parameters()` with keys `_ops.0.…`."""
    def __init__(self, m):
        super().__init__()
        self._ops = torch.nn.ModuleList([m])


@pytest.mark.parametrize('same', [False, True], ids=['xy', 'same'])
@pytest.mark.parametrize('mode', ['train_nodrop', 'eval', 'train'])
@pytest.mark.parametrize('b,C,L', [(5, 16, 8), (7, 128, 8)])
def test_standalone_op_matches_restatement(b, C, L, mode, same):
    from bmnas import lib
    training = mode != 'eval'
    drpt = 0.2 if mode == 'train' else 0.0
    p, x, y, _, g = cm.make_case([MISH], b, C, L, same, 4300 + b + C + same)
    m = build_alone(p, C, L, mode, drpt)
    xd = x.to(dev()).requires_grad_(True)
    yd = xd if same else y.to(dev()).requires_grad_(True)
    with recorded_sites() as rec:
        out = m(xd, yd)
    assert type(out.grad_fn).__name__ == 'ConvBnActFnBackward'
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    masks = None
    if mode == 'train':
        assert len(rec) == 1 and rec[0][1] == b * C * L
        masks = [lib.dropout_mask(rec[0][0], rec[0][1], dev()).cpu()]
        assert abs(float((masks[0] == 0).float().mean()) - drpt) < 0.04
    else:
        assert rec == []
    want = cm.oracle_op([MISH], p, x, y, torch.ones(1), g, same, training, drpt, 0.0, masks)
    assert compare(_Holder(m), training, out, xd, yd, None, same, want) == 4


@pytest.mark.parametrize('b,C,L', [(5, 16, 8), (7, 128, 8)])
def test_forward_thru_gives_the_gradients_of_forward(b, C, L):
    """forward_thru hands both inputs back; a later torch reader of both aliases must see its gradient accumulated by
    the op's data-gradient launch: the same input and parameter gradients as forward with the readers on x and y."""
    p, x, y, _, g = cm.make_case([MISH], b, C, L, False, 4400 + b + C)
    res = []
    for thru in (False, True):
        m = build_alone(p, C, L, 'train_nodrop')
        xd, yd = x.to(dev()).requires_grad_(True), y.to(dev()).requires_grad_(True)
        if thru:
            s, ax, ay = m.forward_thru(xd, yd)
            assert type(s.grad_fn).__name__ == 'ConvBnActThruFnBackward'
        else:
            s, ax, ay = m(xd, yd), xd, yd
        (s * 1.5 + ax * ay + ax.sin()).backward(g.to(dev()))
        torch.cuda.synchronize()
        res.append([s.detach(), xd.grad, yd.grad] + [v.grad for v in m.parameters()])
    for i, (a, b_) in enumerate(zip(*res)):
        if i == 4:                                          # conv.bias in front of a train-mode BatchNorm
            assert float(a.abs().max()) < 1e-4 and float(b_.abs().max()) < 1e-4
        else:
            assert_close_scaled(f'tensor {i}', b_, a, rel=2e-4 if i else 1e-4)
