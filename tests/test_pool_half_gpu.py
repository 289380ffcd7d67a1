"""-m gpu: bf16 / fp16 backbone features in the reshape layers' pooling (csrc/pool.hip, bmnas_adaptive_maxpool_*_group_ex).

Everything is compared with torch.equal — max pooling selects an element, its fp32 widening is exact, and the upstream
gradients (tests/pool_ref.make_grad: multiples of 2^-6 in [-4, 4]) make every fp32 window sum exact in any order, so the
expected dx is that sum rounded once to the element type.  The rule itself is tests/pool_ref.py (pinned to aten's CPU
op in tests/test_pool_ref.py).  Inputs (pool_ref.make_input): few levels, so zeros and ties fill every window; +0 / -0
mixed; an all-equal and an all -inf window; NaNs, two of them adjacent.

Shapes: the smallest at which each path of the kernels can go wrong — a window that is one contiguous span of the plane
(ReshapeInputLayer) aligned and not, planes whose size in bytes is no multiple of 16, overlapping and repeated windows,
more than one 16-byte pass per lane with a tail, H = W = 1; 2-D windows (ReshapeInputLayer_MMIMDB) whose row is exactly
one 16-byte segment, narrower, overlapping, H < oh, odd widths; tensors that start 2, 4 and 8 bytes behind a 16-byte
boundary (the first and last chunk of the tensor then stick out of it and are accessed element by element)."""
import copy
import ctypes
import os
import sys

import pytest
import torch
import torch.nn as nn

import pool_ref
from gpu_util import assert_close_scaled, dev

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

HALF = [torch.bfloat16, torch.float16]
GUARD = 64
SPAN = [((2, 3, 8, 40), 4), ((2, 3, 5, 7), 4), ((2, 3, 2, 7), 4), ((2, 3, 13, 3, 3), 8), ((1, 2, 8, 1030), 8),
        ((3, 48), 8)]
WIN2D = [((2, 3, 20, 32), 16), ((2, 3, 10, 16), 16), ((2, 3, 5, 8), 16), ((2, 3, 3, 3), 16), ((2, 3, 6, 6), 16),
         ((2, 16), 16)]


class _A:
    drpt = 0.0


def _dims(kind, shape, L):
    """(C, H, W, oh, ow) as the reshape layer of that kind views a feature of that shape"""
    import models.auxiliary.aux_models as aux
    cls = aux.ReshapeInputLayer if kind == 'span' else aux.ReshapeInputLayer_MMIMDB
    return cls(shape[1], 16, L, _A()).pool_dims(torch.empty(shape, device='meta'))


def _bits(t):
    """equality that tells +0 from -0 and takes every NaN for the same value"""
    t = t.detach().cpu()
    if t.dtype == torch.float32:
        return torch.where(t.isnan(), torch.full_like(t, 7.0), t).view(torch.int32)
    return torch.where(t.isnan(), torch.full_like(t, 7.0), t).view(torch.int16)


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


class Guarded:
    """tensors of any type inside sentinel-filled buffers, `offset` elements behind the buffer's (16-byte aligned)
    start; check(): no byte outside them was written"""

    def __init__(self):
        self.bufs = []

    def new(self, shape, dtype, base=None, offset=0):
        n = 1
        for s in shape:
            n *= int(s)
        raw = torch.full((n + 2 * GUARD + 8,), 1 if dtype == torch.int32 else 3.0, dtype=dtype, device=dev())
        assert raw.data_ptr() % 16 == 0
        lo = GUARD + offset
        view = raw[lo:lo + n].view(*shape)
        if base is not None:
            view.copy_(base)
        self.bufs.append((raw, lo, n, raw.clone()))
        return view

    def check(self):
        torch.cuda.synchronize()
        for raw, lo, n, before in self.bufs:
            assert torch.equal(raw[:lo], before[:lo]) and torch.equal(raw[lo + n:], before[lo + n:]), \
                f'an element outside a {n}-element tensor was written'


def _expected(x, dims, seed):
    C, H, W, oh, ow = dims
    b = x.shape[0]
    v, i = pool_ref.pool_fwd(x.view(b, C, H, W), oh, ow)
    g = pool_ref.make_grad(tuple(v.shape), seed)
    return v, i, g, pool_ref.pool_bwd(g, i, H, W, x.dtype).view(x.shape)


def _launch(xs, dims, gs, offsets=None, want_idx=True):
    """the two launches through bmnas.lib on guarded device tensors -> (outs, idxs, dxs)"""
    from bmnas import lib
    G = Guarded()
    offsets = offsets or [0] * len(xs)
    b = xs[0].shape[0]
    xd = [G.new(x.shape, x.dtype, x, off) for x, off in zip(xs, offsets)]
    n_out = [(b, d[0], d[3] * d[4]) for d in dims]
    outs = [G.new(s, torch.float32) for s in n_out]
    idxs = [G.new(s, torch.int32) if want_idx else None for s in n_out]
    before = [x.clone() for x in xd]
    lib.adaptive_maxpool_group(xd, dims, outs, idxs, b)
    dxs = None
    if want_idx:
        gd = [g.to(dev()) for g in gs]
        dxs = [G.new(x.shape, x.dtype, None, off) for x, off in zip(xs, offsets)]
        lib.adaptive_maxpool_group_bwd(gd, idxs, dxs, dims, b)
    G.check()
    for x, was in zip(xd, before):
        assert torch.equal(_bits(x), _bits(was))
    return outs, idxs, dxs


CACHE = {}


def _case(kind, shape, L, dtype):
    """(x, dims, expected) of a case, computed once"""
    key = (kind, shape, L, dtype)
    if key not in CACHE:
        dims = _dims(kind, shape, L)
        b = shape[0]
        x = pool_ref.make_input((b,) + dims[:3], dims[3], dims[4], dtype, seed=len(CACHE) + 11).view(shape)
        CACHE[key] = (x, dims, _expected(x, dims, seed=len(CACHE) + 101))
    return CACHE[key]


def _check_member(tag, x, want, out, idx, dx):
    v, i, _, wdx = want
    assert out.dtype == torch.float32 and _same(out.cpu(), v), f'{tag}: pooled values'
    if idx is not None:
        assert torch.equal(idx.cpu(), i), f'{tag}: argmax'
    if dx is not None:
        assert dx.dtype == x.dtype and _same(dx.cpu(), wdx), f'{tag}: dx'


@pytest.mark.parametrize('dtype', HALF, ids=str)
@pytest.mark.parametrize('kind,shape,L', [('span',) + c for c in SPAN] + [('2d',) + c for c in WIN2D])
def test_half_pool_is_the_rule(kind, shape, L, dtype):
    x, dims, want = _case(kind, shape, L, dtype)
    assert x.isnan().any() and (x == 0).any()
    if dtype == torch.bfloat16 and shape == (2, 3, 2, 7):
        # repeated windows: an element receives the sum of two gradients, which bf16 cannot hold — the narrowing rounds
        exact = pool_ref.pool_bwd(want[2], want[1], dims[1], dims[2], torch.float32).view(shape)
        assert not torch.equal(want[3].float(), exact)
    outs, idxs, dxs = _launch([x], [dims], [want[2]])
    _check_member(f'{kind} {shape}', x, want, outs[0], idxs[0], dxs[0])


@pytest.mark.parametrize('dtype', HALF, ids=str)
@pytest.mark.parametrize('kind,shape,L', [('span', (2, 3, 5, 7), 4), ('span', (1, 2, 8, 1030), 8),
                                          ('2d', (2, 3, 20, 32), 16), ('2d', (2, 3, 6, 6), 16)])
def test_any_pointer_alignment(kind, shape, L, dtype):
    """the same map 2, 4 and 8 bytes behind a 16-byte boundary: the results of the aligned copy"""
    x, dims, want = _case(kind, shape, L, dtype)
    for off in (1, 2, 4):
        outs, idxs, dxs = _launch([x], [dims], [want[2]], offsets=[off])
        _check_member(f'{kind} {shape} +{2 * off} B', x, want, outs[0], idxs[0], dxs[0])


def _mixed():
    cases = [('2d', (2, 3, 5, 8), 16, torch.float32), ('2d', (2, 3, 20, 32), 16, torch.bfloat16),
             ('2d', (2, 3, 5, 8), 16, torch.float16), ('span', (2, 3, 5, 7), 4, torch.bfloat16)]
    return [_case(*c) for c in cases]


def test_mixed_group_and_the_fp32_member_keeps_its_bits():
    """[fp32, bf16, fp16, bf16] in one launch; the fp32 member against the entry points without a type, called on it
    alone: out, idx and dx bit for bit"""
    from bmnas import lib
    members = _mixed()
    xs, dims, wants = [m[0] for m in members], [m[1] for m in members], [m[2] for m in members]
    outs, idxs, dxs = _launch(xs, dims, [w[2] for w in wants])
    for k, (x, w) in enumerate(zip(xs, wants)):
        _check_member(f'member {k}', x, w, outs[k], idxs[k], dxs[k])
    x, (C, H, W, oh, ow), g = xs[0].to(dev()), dims[0], wants[0][2].to(dev())
    out = torch.full_like(outs[0], 3.0)
    idx = torch.full_like(idxs[0], 1)
    dx = torch.full_like(x, 3.0)
    fwd = (lib.PoolProb * 1)(lib.PoolProb(x.data_ptr(), out.data_ptr(), idx.data_ptr(), None, None, C, H, W, oh, ow))
    bwd = (lib.PoolProb * 1)(lib.PoolProb(None, None, idx.data_ptr(), g.data_ptr(), dx.data_ptr(), C, H, W, oh, ow))
    stream = torch.cuda.current_stream().cuda_stream
    assert lib.load().bmnas_adaptive_maxpool_fwd_group(fwd, 1, 2, stream) == 0
    assert lib.load().bmnas_adaptive_maxpool_bwd_group(bwd, 1, 2, stream) == 0
    torch.cuda.synchronize()
    assert _same(out.cpu(), outs[0].cpu()) and torch.equal(idx, idxs[0]) and _same(dx.cpu(), dxs[0].cpu())


@pytest.mark.parametrize('n', [1, 8])
def test_groups_of_one_and_of_max_group(n):
    from bmnas import lib
    assert lib.MAX_GROUP == 8
    pool = _mixed() + [_case('span', (2, 3, 5, 7), 4, torch.float16), _case('span', (2, 3, 8, 40), 4, torch.bfloat16),
                       _case('span', (2, 3, 2, 7), 4, torch.float16), _case('2d', (2, 3, 3, 3), 16, torch.bfloat16)]
    members = pool[1:2] if n == 1 else pool
    assert len(members) == n
    outs, idxs, dxs = _launch([m[0] for m in members], [m[1] for m in members], [m[2][2] for m in members])
    for k, m in enumerate(members):
        _check_member(f'member {k} of {n}', m[0], m[2], outs[k], idxs[k], dxs[k])


def test_forward_without_indices():
    members = _mixed()
    outs, _, _ = _launch([m[0] for m in members], [m[1] for m in members], None, want_idx=False)
    for k, m in enumerate(members):
        _check_member(f'member {k}', m[0], m[2], outs[k], None, None)
    # ... and through the Function when no input wants a gradient
    from bmnas.functions import PoolGroupFn
    res = PoolGroupFn.apply([m[1] for m in members], *[m[0].to(dev()) for m in members])
    for k, m in enumerate(members):
        assert not res[k].requires_grad and _same(res[k].cpu(), m[2][0])


def test_function_backward_for_a_subset_and_in_each_inputs_dtype():
    from bmnas.functions import PoolGroupFn
    members = _mixed()
    xs = [m[0].to(dev()).requires_grad_(k != 2) for k, m in enumerate(members)]
    res = PoolGroupFn.apply([m[1] for m in members], *xs)
    sum((r * m[2][2].to(dev())).sum() for r, m in zip(res, members)).backward()
    for k, (x, m) in enumerate(zip(xs, members)):
        assert res[k].dtype == torch.float32 and _same(res[k].detach().cpu(), m[2][0])
        if k == 2:
            assert x.grad is None
        else:
            assert x.grad.dtype == x.dtype and _same(x.grad.cpu(), m[2][3]), k
    with pytest.raises(TypeError, match='fp32 only'):
        PoolGroupFn.apply([members[0][1]], members[0][0].double().to(dev()))


def test_nan_gradient_stays_nan():
    from bmnas import lib
    for dtype in HALF:
        x = torch.arange(32, dtype=torch.float32).view(1, 2, 4, 4).to(dtype).to(dev())
        out = torch.empty(1, 2, 4, device=dev())
        idx = torch.empty(1, 2, 4, dtype=torch.int32, device=dev())
        lib.adaptive_maxpool_group([x], [(2, 4, 4, 2, 2)], [out], [idx], 1)
        g = torch.tensor([[[1.0, float('nan'), 2.0, float('inf')], [70000.0, -1.0, 0.0, 1e-30]]], device=dev())
        dx = torch.empty_like(x)
        lib.adaptive_maxpool_group_bwd([g], [idx], [dx], [(2, 4, 4, 2, 2)], 1)
        want = torch.zeros(1, 2, 16)
        want[0, :, [5, 7, 13, 15]] = g[0].cpu()
        assert _same(dx.cpu().view(1, 2, 16), want.to(dtype))           # (fp16: 70000 overflows to inf, as torch's cast)
        assert dx.view(-1)[7].isnan()


def test_bad_dtype_code_is_refused_before_any_launch():
    from bmnas import lib
    x = torch.ones(2, 3, 4, 4, device=dev(), dtype=torch.bfloat16)
    out = torch.full((2, 3, 4), 3.0, device=dev())
    idx = torch.full((2, 3, 4), 1, dtype=torch.int32, device=dev())
    g = torch.ones(2, 3, 4, device=dev())
    dx = torch.full_like(x, 3.0)
    stream = torch.cuda.current_stream().cuda_stream
    for code in (3, -1, 1 << 16):
        probs = (lib.PoolProbEx * 2)(
            lib.PoolProbEx(x.data_ptr(), out.data_ptr(), idx.data_ptr(), g.data_ptr(), dx.data_ptr(), 3, 4, 4, 2, 2,
                           lib.DT_BF16),
            lib.PoolProbEx(x.data_ptr(), out.data_ptr(), idx.data_ptr(), g.data_ptr(), dx.data_ptr(), 3, 4, 4, 2, 2,
                           code))
        for fn in (lib.load().bmnas_adaptive_maxpool_fwd_group_ex, lib.load().bmnas_adaptive_maxpool_bwd_group_ex):
            rc = fn(probs, 2, 2, stream)
            assert rc == -1                                              # BMNAS_E_ARG
            with pytest.raises(lib.BmnasError, match='bad argument'):
                lib._check(rc, 'adaptive_maxpool_group_ex')
    torch.cuda.synchronize()
    assert (out == 3.0).all() and (idx == 1).all() and (dx == 3.0).all()  # the valid first problem was not launched either
    # an odd address cannot hold half elements
    raw = torch.zeros(2 * x.numel() + 2, dtype=torch.uint8, device=dev())
    bad = (lib.PoolProbEx * 1)(lib.PoolProbEx(raw.data_ptr() + 1, out.data_ptr(), None, None, None, 3, 4, 4, 2, 2,
                                              lib.DT_F16))
    assert lib.load().bmnas_adaptive_maxpool_fwd_group_ex(bad, 1, 2, stream) == -1


# ------------------------------------------------------------------------------------------------------ module level
def _layers(kind, n, L, seed):
    import models.auxiliary.aux_models as aux
    torch.manual_seed(seed)
    cls = aux.ReshapeInputLayer_MMIMDB if kind == 'mmimdb' else aux.ReshapeInputLayer
    return [cls(16, 16, L, _A()).to(dev()).train() for _ in range(n)]


def _raw(shape, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.round(torch.relu(torch.randn(shape, generator=g)) * 4) / 4).to(dtype).to(dev())


@pytest.mark.parametrize('kind,L,shapes,dtypes', [
    ('mmimdb', 16, [(4, 16, 20, 32), (4, 16, 10, 16), (4, 16, 5, 8), (4, 16)],
     [torch.bfloat16, torch.bfloat16, torch.float16, torch.float32]),
    ('video', 8, [(4, 16, 8, 6, 6), (4, 16, 13, 3, 3), (4, 16, 3, 4), (4, 16)],
     [torch.float16, torch.bfloat16, torch.bfloat16, torch.float16])])
def test_reshape_all_on_half_maps_equals_the_widened_maps(kind, L, shapes, dtypes):
    """aux.reshape_all on half raw maps = reshape_all on the same maps widened to fp32: outputs and the conv
    parameters' gradients with torch.equal (the pooled tensors are the same bits; everything behind them is fp32)"""
    import models.auxiliary.aux_models as aux
    layers = _layers(kind, len(shapes), L, 4)
    twins = copy.deepcopy(layers)
    raws = [_raw(s, dt, 20 + k) for k, (s, dt) in enumerate(zip(shapes, dtypes))]
    got = aux.reshape_all(layers, raws)
    want = aux.reshape_all(twins, [r.float() for r in raws])
    ws = [_raw(tuple(o.shape), torch.float32, 40 + k) for k, o in enumerate(got)]
    sum((o * w).sum() for o, w in zip(got, ws)).backward()
    sum((o * w).sum() for o, w in zip(want, ws)).backward()
    for k, (a, b_) in enumerate(zip(got, want)):
        assert a.dtype == torch.float32 and torch.equal(a, b_), (kind, k)
    for k, (m, t) in enumerate(zip(layers, twins)):
        for (name, p), (_, q) in zip(m.named_parameters(), t.named_parameters()):
            assert p.grad is not None and torch.equal(p.grad, q.grad), (kind, k, name)


def test_a_single_half_feature_among_ineligible_ones():
    """one half map, one fp32 map (alone: the torch pool, as always) and a found net's placeholder"""
    import models.auxiliary.aux_models as aux
    layers = _layers('mmimdb', 2, 16, 5) + [nn.ReLU()]
    twins = copy.deepcopy(layers)
    raws = [_raw((4, 16, 5, 8), torch.bfloat16, 1), _raw((3, 16, 5, 8), torch.float32, 2),
            _raw((4, 16, 16), torch.float32, 3)]
    assert aux.pool_groups(layers, raws) == [[0]]
    got = aux.reshape_all(layers, raws)
    want = aux.reshape_all(twins, [r.float() for r in raws])
    for a, b_ in zip(got, want):
        assert a.dtype == torch.float32 and torch.equal(a, b_)
    # a layer called on its own: the native pool as a group of one
    assert torch.equal(layers[0].eval()(raws[0]), twins[0].eval()(raws[0].float()))


def _hyper_args(cname):
    import bench as B
    c = dict(B.CONFIGS[cname], drpt=0.0)
    args = B.make_args(c)
    args.num_outputs = c['nout']
    return c, args


def test_hypernet_with_backbones_under_autocast():
    """a HyperNetBase whose backbones are small conv stacks, args.backbone_dtype = 'bf16': the reshape layers are handed
    bf16 maps, the fusion path sees fp32, forward + backward run and the backbone weights receive finite gradients"""
    import models.auxiliary.aux_models as aux
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase
    c, args = _hyper_args('mmimdb')
    args.backbone_dtype = 'bf16'
    seen = {}

    class Net(HyperNetBase):
        def __init__(self):
            super().__init__()
            self.image = nn.ModuleList([nn.Conv2d(3, 16, 3, padding=1), nn.Conv2d(16, 16, 3, stride=2, padding=1),
                                        nn.Conv2d(16, 16, 3, stride=2, padding=1), nn.Conv2d(16, 16, 1)])
            self.text = nn.ModuleList([nn.Linear(12, 16), nn.Linear(16, 16)])
            self._build_head(args, bnn.BCEWithLogitsLoss(),
                             self.make_reshape_layers(aux.ReshapeInputLayer_MMIMDB, [16] * 6, args), 6, 2)

        def reshape_input_features(self, feats):
            seen['raw'] = [f.dtype for f in feats]
            out = super().reshape_input_features(feats)
            seen['fused'] = [f.dtype for f in out]
            return out

        def forward(self, inputs):
            text, image = inputs
            with self.backbone_autocast():
                feats, h = [], image
                for m in self.image:
                    h = torch.relu(m(h))
                    feats.append(h)
                h = text
                for m in self.text:
                    h = torch.relu(m(h))
                    feats.append(h)
            assert not torch.is_autocast_enabled('cuda')
            return self.fuse(feats)

    torch.manual_seed(6)
    net = Net().to(dev()).train()
    g = torch.Generator().manual_seed(7)
    text, image = torch.randn(4, 12, generator=g).to(dev()), torch.randn(4, 3, 20, 32, generator=g).to(dev())
    y = (torch.rand(4, c['nout'], generator=g) < 0.2).float().to(dev())
    logits = net((text, image))
    assert seen['raw'] == [torch.bfloat16] * 6 and seen['fused'] == [torch.float32] * 6
    assert logits.dtype == torch.float32 and logits.shape == (4, c['nout']) and torch.isfinite(logits).all()
    net.criterion(logits, y).backward()
    for name, p in list(net.image.named_parameters()) + list(net.text.named_parameters()):
        assert p.grad is not None and p.grad.dtype == torch.float32 and torch.isfinite(p.grad).all(), name
    assert any(float(p.grad.abs().max()) > 0 for p in net.image.parameters())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in net.reshape_layers.parameters())


def test_captured_found_step_over_half_raw_maps():
    """GraphedTrainStep over a found-stage model with reshape layers, fed bf16 image maps and fp32 text vectors: the
    pooling launch sits inside the graph, the static inputs keep their dtypes; two replays on different batches each
    equal the eager step of a twin on the same batch"""
    import bench as B
    import models.auxiliary.aux_models as aux
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    from models.search._common import HyperNetBase
    c, args = _hyper_args('mmimdb')
    genotype = B.found_genotype('mmimdb')

    class Net(nn.Module):
        """reshape layers -> found fusion network -> classifier, wired like Found_Image_Text_Net behind its backbones"""

        def __init__(self):
            super().__init__()
            self.reshape_layers = HyperNetBase.make_reshape_layers(aux.ReshapeInputLayer_MMIMDB, [16] * 6, args, genotype)
            self.found = B.FoundNet(c, 'mmimdb')

        def forward(self, raws):
            return self.found(aux.reshape_all(list(self.reshape_layers), list(raws)))

    nets = []
    for _ in range(2):
        torch.manual_seed(8)
        nets.append(Net().to(dev()).train())
        for mod in nets[-1].modules():                 # deterministic: dropout parity has its own tests
            if isinstance(mod, nn.Dropout):
                mod.p = 0.0
    assert any(isinstance(m, aux._ReshapeBase) for m in nets[0].reshape_layers)
    crit = bnn.BCEWithLogitsLoss()
    opts = [Adam(m.parameters(), lr=1e-3, weight_decay=1e-4) for m in nets]
    shapes = [(8, 16, 20, 32), (8, 16, 10, 16), (8, 16, 5, 8), (8, 16, 5, 8), (8, 16), (8, 16)]
    dtypes = [torch.bfloat16] * 4 + [torch.float32] * 2

    def batch(seed):
        g = torch.Generator().manual_seed(seed)
        y = (torch.rand(8, c['nout'], generator=g) < 0.2).float().to(dev())
        return [_raw(s, dt, seed * 10 + k) for k, (s, dt) in enumerate(zip(shapes, dtypes))], y

    xs, y = batch(1)
    step = GraphedTrainStep(nets[0], crit, opts[0], xs, y)
    start = [p.detach().clone() for p in nets[0].parameters()]
    for it in (2, 3, 4):           # (loss and logits of a later step depend on the earlier updates: they pin those too)
        xs, y = batch(it)
        loss_g, logits_g = step(xs, y)[:2]
        opts[1].zero_grad()
        logits_e = nets[1](xs)
        loss_e = crit(logits_e, y)
        loss_e.backward()
        opts[1].step()
        torch.cuda.synchronize()
        assert_close_scaled(f'replay {it} loss', loss_g.reshape(1), loss_e.detach().reshape(1))
        assert_close_scaled(f'replay {it} logits', logits_g, logits_e.detach())
    assert any(not torch.equal(a, b_) for a, b_ in zip(start, nets[0].parameters()))       # the replays do train
