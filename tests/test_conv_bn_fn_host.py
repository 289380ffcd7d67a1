"""CPU: which launches the conv + BatchNorm autograd Functions and the two NodeMixedOp Functions issue, with which
arguments — ConvBnActFn, ConvBnActThruFn, ConvBnReluLnFn, ReshapeGroupFn (bmnas.functions) and NodeMixedFn /
NodeMixedSelFn through bmnas.cell.node_mixed_* — and the layout of the `bn_grad | dW | dbias` gradient chunk.

Every bmnas.lib wrapper these Functions reach is replaced by a recorder, `_require_gpu` is stubbed, and forward +
backward run on CPU tensors at b = 3, C_src = 8, M = 16, L = 4 with two sources.  A recorder notes the wrapper's name
and, per argument: a tensor as `T<k>+<offset>:<shape>` (k numbers the storages in the order the trace meets them, so a
slice of one zero-filled chunk shows as the chunk's number plus its offset; `:nc` marks a non-contiguous one), an int /
float / bool / None as its value, a ctypes descriptor by its plain fields (pointers as ptr / None), lists and tuples
element by element.  `fork.side` marks work handed to a bmnas.cell._Fork.  Behind the calls: the gradient every
differentiable input received.

The expected traces in tests/golden/conv_bn_fn_calls.json were recorded from commit 9575678 ("Kernel-level float64
tests for the search-stage grouped FC-edge kernels"), the parent of the commit that gave these Functions one forward
prologue, one backward body and one gradient layout: that commit had to reproduce them without a regenerated row.
Regenerate with
    python tests/test_conv_bn_fn_host.py > tests/golden/conv_bn_fn_calls.json
only when a launch sequence is changed on purpose."""
import contextlib
import ctypes as C
import json
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_bn_fn_calls.json')

B, C_SRC, M_OUT, L_SEQ = 3, 8, 16, 4

# the bmnas.lib wrappers that launch (or, conv1x1_num_partials, ask the library): everything else these Functions take
# from bmnas.lib builds a descriptor on the host and stays as it is
LAUNCHERS = ('conv1x1_fwd', 'conv1x1_fwd_sdpa', 'conv1x1_bwd_data', 'conv1x1_bwd_weight', 'conv1x1_bwd_all',
             'conv1x1_bwd_all_sdpa', 'bn_finalize', 'bn_bwd_apply', 'bn_glu_fwd', 'bn_glu_bwd', 'bn_relu_fwd',
             'bn_relu_bwd', 'bn_mish_fwd', 'bn_mish_bwd', 'bn_relu_ln_fwd', 'bn_relu_ln_bwd', 'ln_affine_bwd',
             'ln_affine_bwd_multi', 'cell_prologue', 'conv1x1_fwd_group', 'bn_relu_fwd_group', 'bn_relu_bwd_group',
             'conv1x1_bwd_group', 'sdpa_ln_fwd', 'sdpa_ln_bwd', 'fold_weight', 'node_mix_fwd', 'node_mix_bwd',
             'node_mix_sel_fwd', 'node_mix_sel_bwd', 'node_mix_ln_fwd', 'node_mix_ln_bwd', 'node_mix_pre_fwd',
             'node_mix_lnp_bwd')
N_PARTIALS = 2          # what the stubbed conv1x1_num_partials answers


class Recorder:
    def __init__(self):
        self.calls, self.keep, self.storages = [], [], {}

    def tensor(self, t):
        self.keep.append(t)                      # alive until the case ends: no address is handed out twice
        if t.numel() == 0:
            return f'T-:{tuple(t.shape)}'
        k = self.storages.setdefault(t.untyped_storage().data_ptr(), len(self.storages))
        return f'T{k}+{t.storage_offset()}:{tuple(t.shape)}' + ('' if t.is_contiguous() else ':nc')

    def desc(self, v):
        if torch.is_tensor(v):
            return self.tensor(v)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        if isinstance(v, (list, tuple)):
            return [self.desc(e) for e in v]
        if isinstance(v, dict):
            return {k: self.desc(e) for k, e in sorted(v.items())}
        if isinstance(v, C.Structure):
            parts = []
            for name, typ in v._fields_:
                e = getattr(v, name)
                if typ is C.c_void_p:
                    e = 'ptr' if e else None
                elif isinstance(e, C.Array):
                    e = list(e)
                parts.append(f'{name}={e}')
            return f'{type(v).__name__}({", ".join(parts)})'
        if isinstance(v, torch.device):
            return str(v)
        return f'<{type(v).__name__}>'

    def wrapper(self, name, result=None):
        def record(*a, **k):
            self.calls.append([name] + [self.desc(e) for e in a] + [f'{n}={self.desc(e)!r}' for n, e in sorted(k.items())])
            return result
        return record

    def cut(self):
        calls, self.calls = self.calls, []
        return calls


@contextlib.contextmanager
def recording(fuse_attn=True, standalone_bn=True):
    """The Functions on CPU tensors, their launches recorded; pools, dropout offsets and seed at a fixed start."""
    from bmnas import cell as K
    from bmnas import functions as F
    rec = Recorder()
    mp = pytest.MonkeyPatch()
    try:
        for name in LAUNCHERS:
            mp.setattr(F.lib, name, rec.wrapper(name))
        mp.setattr(F.lib, 'conv1x1_num_partials', rec.wrapper('conv1x1_num_partials', N_PARTIALS))
        mp.setattr(F, '_require_gpu', lambda t, what: None)

        class Fork:                                  # bmnas.cell._Fork without its HIP streams
            def __init__(self, device):
                pass

            def __enter__(self):
                return self

            def __exit__(self, *exc):
                return False

            def side(self, fn):
                rec.calls.append(['fork.side'])
                fn()

        mp.setattr(K, '_Fork', Fork)
        mp.setattr(K, 'FUSE_ATTN_GEMM', fuse_attn)
        mp.setattr(F, 'FUSE_STANDALONE_BN', standalone_bn)
        mp.setattr(F, 'ZERO_POOL', F._ZeroPool())
        mp.setattr(F, 'FWD_STAT_POOL', F._FwdStatPool())
        mp.setattr(K.DROP, 'offset', 0)
        torch.manual_seed(0)
        yield rec
    finally:
        mp.undo()


def _t(*shape, grad=True):
    return torch.randn(*shape).requires_grad_(grad)


def _bn(M):
    return torch.zeros(M), torch.ones(M), torch.zeros((), dtype=torch.long)


def _conv_params(M, K_in):
    return _t(M, K_in, 1), _t(M), _t(M), _t(M)


def _finish(rec, fwd, inputs):
    return {'fwd': fwd, 'bwd': rec.cut(), 'grads': [rec.desc(t.grad) for t in inputs]}


# ------------------------------------------------------------------------------------------------ the cases
def case_conv_bn_act(act, training, frozen_src=False, standalone_bn=True):
    from bmnas.functions import ConvBnActFn
    with recording(standalone_bn=standalone_bn) as rec:
        srcs = [_t(B, C_SRC, L_SEQ), _t(B, C_SRC, L_SEQ, grad=not frozen_src)]
        prm = _conv_params(M_OUT, 2 * C_SRC)
        out = ConvBnActFn.apply(act, 0.2, training, *_bn(M_OUT), 0.1, *prm, *srcs)
        fwd = rec.cut()
        assert tuple(out.shape) == (B, M_OUT // 2 if act == 'glu' else M_OUT, L_SEQ)
        assert type(out.grad_fn).__name__ == 'ConvBnActFnBackward'
        out.sum().backward()
        return _finish(rec, fwd, [*prm, *srcs])


def case_unknown_activation():
    from bmnas.functions import ConvBnActFn
    with recording() as rec:
        rm, rv, nbt = _bn(M_OUT)
        with pytest.raises(ValueError, match='no kernel for the activation'):
            ConvBnActFn.apply('gelu', 0.2, True, rm, rv, nbt, 0.1, *_conv_params(M_OUT, 2 * C_SRC),
                              _t(B, C_SRC, L_SEQ), _t(B, C_SRC, L_SEQ))
        assert int(nbt) == 0
        return {'fwd': rec.cut(), 'bwd': [], 'grads': []}


def run_thru(arrival):
    """arrival: 'identity' (only a handed-back source is differentiated), 'contiguous', 'strided'.
    -> (case record, gradient that arrived for source 0, gradient handed on for source 0)"""
    from bmnas.functions import ConvBnActThruFn
    with recording() as rec:
        leaves = [_t(B, C_SRC, L_SEQ), _t(B, C_SRC, L_SEQ)]
        srcs = [t * 1.0 for t in leaves]                 # not leaves: a hook sees what the backward returns for them
        prm = _conv_params(M_OUT, 2 * C_SRC)
        out, s0, s1 = ConvBnActThruFn.apply('relu', 0.2, True, *_bn(M_OUT), 0.1, *prm, *srcs)
        fwd = rec.cut()
        assert type(out.grad_fn).__name__ == 'ConvBnActThruFnBackward'
        arrived, returned = [], []
        s0.register_hook(arrived.append)
        srcs[0].register_hook(returned.append)
        if arrival == 'identity':
            loss = (s0 * 2.0).sum()
        elif arrival == 'contiguous':
            loss = out.sum() + (s0 * 2.0).sum()           # the product's backward hands over a fresh contiguous tensor
        else:
            loss = out.sum() + s0.sum()                   # sum's backward: an expanded (stride 0) tensor
        loss.backward()
        return _finish(rec, fwd, [*prm, *leaves]), arrived[0], returned[0]


def case_conv_bn_relu_ln(want_sums):
    from bmnas.functions import ConvBnReluLnFn
    with recording() as rec:
        srcs = [_t(B, C_SRC, L_SEQ), _t(B, C_SRC, L_SEQ)]
        prm = _conv_params(M_OUT, 2 * C_SRC)
        ln_w, ln_b, x = _t(M_OUT, L_SEQ), _t(M_OUT, L_SEQ), _t(B, M_OUT, L_SEQ)
        out, sums = ConvBnReluLnFn.apply(0.2, True, want_sums, *_bn(M_OUT), 0.1, *prm, ln_w, ln_b, x, *srcs)
        fwd = rec.cut()
        assert tuple(sums.shape) == ((B, 2) if want_sums else (0,))
        assert type(out.grad_fn).__name__ == 'ConvBnReluLnFnBackward'
        out.sum().backward()
        return _finish(rec, fwd, [*prm, ln_w, ln_b, x, *srcs])


RESHAPE_C_IN = (8, 12)


def case_reshape_group():
    """-> the first pass, and a second backward over the retained graph (the forward's cleared buffer is gone)"""
    from bmnas.functions import ReshapeGroupFn
    with recording() as rec:
        xs = [_t(B, c, L_SEQ) for c in RESHAPE_C_IN]
        prm = [p for c in RESHAPE_C_IN for p in _conv_params(M_OUT, c)]
        outs = ReshapeGroupFn.apply(2, 0.2, True, [_bn(M_OUT) for _ in RESHAPE_C_IN], *xs, *prm)
        fwd = rec.cut()
        assert type(outs[0].grad_fn).__name__ == 'ReshapeGroupFnBackward'
        loss = outs[0].sum() + outs[1].sum()
        loss.backward(retain_graph=True)
        first = _finish(rec, fwd, [*xs, *prm])
        loss.backward()
        return first, _finish(rec, [], [*xs, *prm])


class _Args:
    drpt = 0.2


DEFAULT_PRIMS = ['Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC']
SEL_LISTS = (['Sum'], ['ScaleDotAttn'], ['LinearGLU', 'Sum'], ['ConcatFC', 'LinearGLU', 'ScaleDotAttn', 'Sum'])


def case_node_mixed(prims, same, fuse_attn):
    """NodeMixedFn for the default list, NodeMixedSelFn for an edited one, over a real NodeMixedOp's pack."""
    import models.search.darts.genotypes as gt
    from bmnas.functions import NodeMixedFn, NodeMixedSelFn
    from models.search.darts.node_operations import NodeMixedOp
    saved = list(gt.STEP_STEP_PRIMITIVES)
    gt.STEP_STEP_PRIMITIVES[:] = prims
    try:
        with recording(fuse_attn=fuse_attn) as rec:
            op = NodeMixedOp(C_SRC, L_SEQ, _Args())
            op.train()
            x = _t(B, C_SRC, L_SEQ)
            y = x if same else _t(B, C_SRC, L_SEQ)
            gamma = _t(len(prims))
            fn = NodeMixedFn if prims == DEFAULT_PRIMS else NodeMixedSelFn
            out = fn.apply(op, True, x, y, gamma, *op.param_list())
            fwd = rec.cut()
            assert type(out.grad_fn).__name__ == fn.__name__ + 'Backward'
            out.sum().backward()
            return _finish(rec, fwd, [x, y, gamma, *op.param_list()])
    finally:
        gt.STEP_STEP_PRIMITIVES[:] = saved


def _mixed_id(prims, same, fuse_attn):
    return (f'node_mixed {"default" if prims == DEFAULT_PRIMS else "+".join(prims)} '
            f'{"x is y" if same else "x, y"} fuse_attn={int(fuse_attn)}')


MIXED = [(p, s, f) for p in (DEFAULT_PRIMS,) + SEL_LISTS for s in (True, False) for f in (True, False)]


def record():
    out = {}
    for act in ('glu', 'relu', 'mish'):
        for training in (True, False):
            out[f'conv_bn_act {act} training={int(training)}'] = case_conv_bn_act(act, training)
    out['conv_bn_act relu, source 1 without requires_grad'] = case_conv_bn_act('relu', True, frozen_src=True)
    out['conv_bn_act relu, bn_finalize launch'] = case_conv_bn_act('relu', True, standalone_bn=False)
    out['conv_bn_act unknown activation'] = case_unknown_activation()
    for arrival in ('identity', 'contiguous', 'strided'):
        out[f'conv_bn_act_thru {arrival}'] = run_thru(arrival)[0]
    for want_sums in (True, False):
        out[f'conv_bn_relu_ln want_sums={int(want_sums)}'] = case_conv_bn_relu_ln(want_sums)
    out['reshape_group'], out['reshape_group second backward'] = case_reshape_group()
    for prims, same, fuse in MIXED:
        out[_mixed_id(prims, same, fuse)] = case_node_mixed(prims, same, fuse)
    return json.loads(json.dumps(out))               # tuples -> lists, as the file holds them


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def traces():
    return record()


def test_the_case_list_is_the_recorded_one(traces):
    assert sorted(traces) == sorted(_golden()), 'the case list and the recorded file differ: regenerate on purpose only'


@pytest.mark.parametrize('cid', sorted(_golden()) if os.path.exists(GOLDEN) else [])
def test_launch_sequence_is_the_parents(traces, cid):
    got, want = traces[cid], _golden()[cid]
    for part in ('fwd', 'bwd'):
        assert [c[0] for c in got[part]] == [c[0] for c in want[part]], f'{cid}: other launches in {part}'
        for i, (g, w) in enumerate(zip(got[part], want[part])):
            assert g == w, f'{cid}: {part} call {i} ({g[0]}) differs'
    assert got['grads'] == want['grads'], f'{cid}: other gradients handed to autograd'


def test_what_the_recorded_traces_must_show():
    """The properties the cases were chosen for, read from the recorded file itself."""
    g = _golden()
    names = lambda cid, part: [c[0] for c in g[cid][part]]
    assert g['conv_bn_act unknown activation'] == {'fwd': [], 'bwd': [], 'grads': []}
    assert g['conv_bn_act_thru identity']['bwd'] == []
    for act in ('glu', 'relu', 'mish'):
        for tr in (0, 1):
            cid = f'conv_bn_act {act} training={tr}'
            # training: the statistics are finalised inside the activation launch; eval: a bn_finalize launch
            assert names(cid, 'fwd') == ['conv1x1_fwd'] + ['bn_finalize'] * (1 - tr) + [f'bn_{act}_fwd'], cid
            assert names(cid, 'bwd')[0] == f'bn_{act}_bwd', cid
            C_out = M_OUT // 2 if act == 'glu' else M_OUT               # GLU halves the channels
            assert g[cid]['fwd'][-1][4:7] == [B, C_out, L_SEQ] and g[cid]['bwd'][0][6:9] == [B, C_out, L_SEQ], cid
    assert names('conv_bn_act relu, bn_finalize launch', 'fwd') == ['conv1x1_num_partials', 'conv1x1_fwd', 'bn_finalize',
                                                                    'bn_relu_fwd']
    assert g['conv_bn_act relu, source 1 without requires_grad']['grads'][-1] is None
    assert names('conv_bn_relu_ln want_sums=1', 'fwd') == ['conv1x1_fwd', 'bn_relu_ln_fwd']
    assert g['conv_bn_relu_ln want_sums=0']['fwd'][1][-1] is None and g['conv_bn_relu_ln want_sums=1']['fwd'][1][-1]
    assert names('reshape_group', 'fwd') == ['cell_prologue', 'conv1x1_fwd_group', 'bn_relu_fwd_group']
    assert names('reshape_group', 'bwd') == names('reshape_group second backward', 'bwd') == \
        ['bn_relu_bwd_group', 'conv1x1_bwd_group']
    for prims, same, fuse in MIXED:
        cid = _mixed_id(prims, same, fuse)
        has_attn, conv = 'ScaleDotAttn' in prims, any(p in prims for p in ('LinearGLU', 'ConcatFC'))
        merged_fwd = has_attn and conv and same and fuse
        assert ('conv1x1_fwd_sdpa' in names(cid, 'fwd')) == merged_fwd, cid
        assert ('sdpa_ln_fwd' in names(cid, 'fwd')) == (has_attn and not merged_fwd), cid
        assert ('conv1x1_bwd_all_sdpa' in names(cid, 'bwd')) == merged_fwd, cid      # (every list here with both: M = 3C)
        assert ('sdpa_ln_bwd' in names(cid, 'bwd')) == (has_attn and not merged_fwd), cid
        assert ('fork.side' in names(cid, 'fwd')) == (has_attn and conv and not merged_fwd), cid


def test_thru_accumulates_onto_a_contiguous_arrival_in_place():
    _, arrived, returned = run_thru('contiguous')
    assert returned is arrived or returned.data_ptr() == arrived.data_ptr()
    assert returned.data_ptr() == arrived.data_ptr() and returned.shape == arrived.shape
    _, arrived, returned = run_thru('strided')           # cannot be accumulated onto: a sum of its own
    assert not arrived.is_contiguous() and returned.data_ptr() != arrived.data_ptr()
    _, arrived, returned = run_thru('identity')
    assert returned.data_ptr() == arrived.data_ptr()


# ------------------------------------------------------------------------- the bn_grad | dW | dbias layout
@pytest.mark.parametrize('M,ldw', [(16, 16), (16, 12), (6, 5)])
def test_conv_grad_chunk_is_tiled_by_its_three_slices(M, ldw):
    from bmnas.functions import conv_grad_floats, conv_grad_split
    n = conv_grad_floats(M, ldw)
    assert n == 2 * M + M * ldw + M
    buf = torch.arange(n + 8, dtype=torch.float32)
    for off in (0, 4):
        bn_grad, dW, dbias = conv_grad_split(buf, M, ldw, off)
        assert tuple(bn_grad.shape) == (2 * M,) and tuple(dW.shape) == (M, ldw) and tuple(dbias.shape) == (M,)
        # back to back, in this order, nothing left over: the three slices read the chunk's floats once each
        assert torch.equal(torch.cat([bn_grad, dW.reshape(-1), dbias]), buf[off:off + n])
        assert dW.is_contiguous() and dW.data_ptr() == buf.data_ptr() + 4 * (off + 2 * M)


def test_round4_and_the_group_offsets():
    from bmnas import cell as K
    from bmnas.functions import _round4, conv_grad_floats, conv_grad_offsets
    assert [_round4(n) for n in (0, 1, 3, 4, 5, 498)] == [0, 4, 4, 4, 8, 500]
    # the ReshapeGroupFn case above: two layers of M = 16 rows with C_in = 8 and 12, behind the forward's batch sums
    base = len(RESHAPE_C_IN) * K.STAT_SHARDS * M_OUT * 2
    offs = conv_grad_offsets(M_OUT, list(RESHAPE_C_IN), base=base)
    assert offs == [256, 256 + 176, 256 + 176 + 240] and conv_grad_offsets(M_OUT, [], base=base) == [base]
    for M, ldws in ((M_OUT, list(RESHAPE_C_IN)), (6, [5, 7, 5]), (5, [6, 6])):
        offs = conv_grad_offsets(M, ldws)
        assert len(offs) == len(ldws) + 1 and offs[0] == 0
        for i, ldw in enumerate(ldws):
            assert offs[i] % 4 == 0 and offs[i] + conv_grad_floats(M, ldw) <= offs[i + 1]      # aligned, no overlap
            assert offs[i + 1] - offs[i] < conv_grad_floats(M, ldw) + 4                          # ... and no gap of 4
    # what the recorded launches of that case were handed
    bwd = _golden()['reshape_group']['bwd'][1]
    assert bwd[0] == 'conv1x1_bwd_group' and bwd[5] == ['T0+288:(16, 8)', 'T0+464:(16, 12)']
    assert bwd[6] == ['T0+416:(16,)', 'T0+656:(16,)'] and bwd[9] == ['T0+256:(32,)', 'T0+432:(32,)']


# ------------------------------------------------------------------------- profiler accounting (GPU)
# what this tree's parent (9575678) listed for the same two passes: recorded there with this very test body
PROFILED_CALLS = {'glu': ['conv1x1_fwd', 'bn_glu_fwd', 'bn_glu_bwd'], 'relu': ['conv1x1_fwd', 'bn_relu_fwd', 'bn_relu_bwd']}


@pytest.mark.gpu
@pytest.mark.parametrize('act', ['glu', 'relu'])
def test_profiler_lists_the_activation_launches_of_both_directions(act):
    """lib.profile_begin swaps bmnas.lib's wrappers for timed ones: the Functions must look the activation wrappers up by
    name when they launch, or bench.py's per-kernel accounting loses them without an error."""
    from bmnas import lib
    from bmnas.functions import ConvBnActFn
    b, C_src, M, L = 4, 16, 32, 16
    dev = torch.device('cuda:0')
    torch.manual_seed(5)
    srcs = [torch.randn(b, C_src, L, device=dev, requires_grad=True) for _ in range(2)]
    prm = [torch.randn(*s, device=dev, requires_grad=True) for s in ((M, 2 * C_src, 1), (M,), (M,), (M,))]
    rm, rv = torch.zeros(M, device=dev), torch.ones(M, device=dev)
    nbt = torch.zeros((), device=dev, dtype=torch.long)
    algo = {n: (lambda *a, **k: ('hbm', 1)) for n in ('bn_glu_fwd', 'bn_glu_bwd', 'bn_relu_fwd', 'bn_relu_bwd',
                                                       'conv1x1_fwd')}
    lib.profile_begin(algo, events=False)
    try:
        out = ConvBnActFn.apply(act, 0.0, True, rm, rv, nbt, 0.1, *prm, *srcs)
        out.sum().backward()
        torch.cuda.synchronize()
    finally:
        calls = lib.profile_end_calls()
    names = [c[0] for c in calls]
    print('profiled calls', act, names)
    assert f'bn_{act}_fwd' in names and f'bn_{act}_bwd' in names
    assert names == PROFILED_CALLS[act]
    assert tuple(out.shape) == (b, M // 2 if act == 'glu' else M, L) and bool(torch.isfinite(out).all())
    assert all(t.grad is not None and bool(torch.isfinite(t.grad).all()) for t in (*prm, *srcs))


if __name__ == '__main__':
    for p in (ROOT, os.path.join(ROOT, 'bm-nas_amd'), os.path.join(ROOT, 'tests')):
        sys.path.insert(0, p)
    json.dump(record(), sys.stdout, indent=0, sort_keys=True)
    print()
