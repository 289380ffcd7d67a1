"""Fusion primitives of a step node and the gamma-weighted NodeMixedOp.

Mirror of the reference's models/search/darts/node_operations.py (STEP_STEP_OPS :9-14,
Sum :16-20, LinearGLU :22-39, ConcatFC :41-56, Mish / CatConvMish :58-82, ScaledDotAttn :84-108, NodeMixedOp :110-120):
same class names, constructor/forward signatures and state_dict keys, but every forward
runs on the gfx950 kernels of libbmnas_hip.so (no eager-PyTorch math on the hot path).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from bmnas.cell import Arena, Pack
from bmnas import lib as _lib
from bmnas.functions import (ConvBnActFn, ConvBnActThruFn, MixSumFn, NodeMixedFn, NodeMixedSelFn,
                             SdpaLnFn, SdpaLnThruFn)

from .genotypes import *  # noqa: F401,F403
from .genotypes import STEP_STEP_PRIMITIVES
from .operations import _MHA_CLASSES, Attention

# every node operation takes two (b, C, L) inputs and returns one (b, C, L) output
# (CatConvMish is not registered, as in the reference: `STEP_STEP_OPS['CatConvMish'] = lambda C, L, args:
# CatConvMish(C, args)` adds it; likewise MultiHeadAttn, the two-input form of operations.Attention)
STEP_STEP_OPS = {
    'Sum': lambda C, L, args: Sum(),
    'ScaleDotAttn': lambda C, L, args: ScaledDotAttn(C, L),
    'LinearGLU': lambda C, L, args: LinearGLU(C, args),
    'ConcatFC': lambda C, L, args: ConcatFC(C, args),
}

_ONES = {}


def _ones2(device):
    t = _ONES.get(device)
    if t is None:
        t = torch.ones(2, device=device, dtype=torch.float32)
        _ONES[device] = t
    return t


class Sum(nn.Module):
    """x + y (reference :16-20), as the two-input mixed-sum kernel with unit weights."""

    def forward(self, x, y):
        return MixSumFn.apply(_ones2(x.device), x, y)


class _CatConvBn(nn.Module):
    """cat([x, y], 1) -> Conv1d(2C, M, 1) -> BatchNorm1d(M) -> act -> Dropout(args.drpt)."""
    _act = None

    def __init__(self, C, M, args):
        super().__init__()
        self.conv = nn.Conv1d(2 * C, M, 1, 1)
        self.bn = nn.BatchNorm1d(M)
        self.dropout = nn.Dropout(args.drpt)

    def forward(self, x, y):
        bn = self.bn
        return ConvBnActFn.apply(self._act, self.dropout.p, self.training, bn.running_mean,
                                 bn.running_var, bn.num_batches_tracked, bn.momentum, self.conv.weight,
                                 self.conv.bias, bn.weight, bn.bias, x, y)

    def forward_thru(self, x, y):
        """-> (out, x', y'): the same, with the two inputs handed back for their LATER readers (bmnas.functions
        ConvBnActThruFn: those readers' gradients are then accumulated by this op's data-gradient launch, not by
        autograd `add` launches)."""
        bn = self.bn
        return ConvBnActThruFn.apply(self._act, self.dropout.p, self.training, bn.running_mean,
                                     bn.running_var, bn.num_batches_tracked, bn.momentum, self.conv.weight,
                                     self.conv.bias, bn.weight, bn.bias, x, y)


class LinearGLU(_CatConvBn):
    """reference :22-39 (glu over the channel dim halves 2C -> C)."""
    _act = 'glu'

    def __init__(self, C, args):
        super().__init__(C, 2 * C, args)


class ConcatFC(_CatConvBn):
    """reference :41-56."""
    _act = 'relu'

    def __init__(self, C, args):
        super().__init__(C, C, args)


class Mish(nn.Module):
    """x tanh(softplus(x)) (reference :58-63).  CatConvMish holds one for the module tree; its forward applies the
    activation inside the BatchNorm tail kernel (csrc/mish.hpp) instead of calling it."""

    def forward(self, x):
        return x * torch.tanh(F.softplus(x))


class CatConvMish(_CatConvBn):
    """reference :65-82: ConcatFC with Mish in place of ReLU; state_dict keys as ConcatFC (Mish has no state)."""
    _act = 'mish'

    def __init__(self, C, args):
        super().__init__(C, C, args)
        self.mish = Mish()


class ScaledDotAttn(nn.Module):
    """Scaled dot-product attention without projections (reference :84-108):
    q = x^T, k = y, v = y^T; softmax(q k / sqrt(C)) v, Dropout(0.1), LayerNorm([C, L])."""

    def __init__(self, C, L):
        super().__init__()
        self.dropout = nn.Dropout(0.1)
        self.ln = nn.LayerNorm([C, L])

    def forward(self, x, y):
        return SdpaLnFn.apply(x, y, self.ln.weight, self.ln.bias, self.dropout.p, self.training)

    def forward_thru(self, x, y):
        """-> (out, x', y'): the same, with the two inputs handed back for their LATER readers (bmnas.functions
        SdpaLnThruFn: those readers' gradients are then accumulated by this op's backward launch, not by autograd
        `add` launches)."""
        return SdpaLnThruFn.apply(x, y, self.ln.weight, self.ln.bias, self.dropout.p, self.training)


class MultiHeadAttn(Attention):
    """The reference's Attention (operations.py:67-86, "step node operation") in the two-input form of a step-node
    primitive: the query comes from x, keys and values from y — ScaledDotAttn's roles, with learned projections and
    `args.num_heads` heads (the reference mains' commented-out --num_heads; 2 when args has none).  state_dict keys as
    Attention's (attn.*).  Not registered, like CatConvMish: `STEP_STEP_OPS['MultiHeadAttn'] = lambda C, L, args:
    MultiHeadAttn(C, L, args)` adds it.  In an edited STEP_STEP_PRIMITIVES list NodeMixedOp keeps its composed sum, with
    this term on its own kernels (bmnas.functions.MhaFn) inside it."""

    def __init__(self, C, L, args):
        super().__init__(C, getattr(args, 'num_heads', 2), args.drpt)

    def forward(self, x, y):
        return Attention.forward(self, x, y, y)


_MHA_CLASSES.append(MultiHeadAttn)

_DEFAULT_PRIMS = ['Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC']
_BUILTIN = {'Sum': Sum, 'ScaleDotAttn': ScaledDotAttn, 'LinearGLU': LinearGLU, 'ConcatFC': ConcatFC,
            'CatConvMish': CatConvMish}
# the primitives of the mix kernels' FC slot (mask bit 3, the C conv rows behind LinearGLU's, the drop_fc site): a list
# holds at most one of them natively
_FC_SLOT = ('ConcatFC', 'CatConvMish')
_FC_ACT = {'ConcatFC': _lib.FC_ACT_RELU, 'CatConvMish': _lib.FC_ACT_MISH}


def _slot_name(p):
    """The kind a primitive name has in the selection descriptor (lib.NODE_KINDS)."""
    return 'ConcatFC' if p in _FC_SLOT else p


# An edited STEP_STEP_PRIMITIVES list made of the built-in primitives (the four of STEP_STEP_OPS and CatConvMish, with
# at most one of ConcatFC / CatConvMish) runs on the selected-term kernels (csrc/nodemix_sel.hip); False forces the composed sum `sum(w * op(x, y))` for A/B timing and tests (the cell-level
# counterpart is operations.FC_EDGES_NATIVE).  The default list is not affected either way.
NODE_PRIMS_NATIVE = True


def node_mix_route(op, x, y, weights):
    """Which path NodeMixedOp.forward(x, y, weights) takes: 'default' (the unedited list: NodeMixedFn), 'selected'
    (a subset / permutation of the built-in primitives, CatConvMish in ConcatFC's place included: NodeMixedSelFn) or
    'composed' (everything else, a list with both ConcatFC and CatConvMish among it: the reference's own sum over the
    primitive modules, node_operations.py:118-120).  Host logic only."""
    if op._default:
        return 'default'
    if not NODE_PRIMS_NATIVE:
        return 'composed'
    prims = op._prims
    if not prims or len(set(prims)) != len(prims) or any(p not in _BUILTIN for p in prims):
        return 'composed'
    if sum(p in _FC_SLOT for p in prims) > 1:
        return 'composed'                    # one FC slot in the kernels
    if len(op._ops) != len(prims) or any(type(m) is not _BUILTIN[p] for p, m in zip(prims, op._ops)):
        return 'composed'                    # an edited STEP_STEP_OPS registry: somebody else's module
    for t in (x, y):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 3):
            return 'composed'
    if x.shape != y.shape or x.device != y.device or tuple(x.shape[1:]) != (op.C, op.L):
        return 'composed'
    if not (torch.is_tensor(weights) and weights.dim() == 1 and weights.numel() == len(prims)
            and weights.dtype == torch.float32):
        return 'composed'
    if any(m.training != op.training for m in op.modules()):
        return 'composed'
    for m in op._ops:
        if isinstance(m, _CatConvBn):
            bn = m.bn
            if not (bn.momentum == 0.1 and bn.eps == 1e-5 and bn.affine and bn.track_running_stats
                    and bn.running_mean is not None and bn.weight.is_cuda):
                return 'composed'
        elif isinstance(m, ScaledDotAttn):
            if not (m.ln.eps == 1e-5 and m.ln.elementwise_affine and m.ln.weight.is_cuda):
                return 'composed'
    mask = sum(1 << _DEFAULT_PRIMS.index(_slot_name(p)) for p in prims)
    if not _lib.node_mix_sel_ok(mask, x.shape[0], op.C, op.L):
        return 'composed'
    return 'selected'


class NodeMixedOp(nn.Module):
    """sum_p weights[p] * op_p(x, y) over STEP_STEP_PRIMITIVES (reference :110-120).

    With the default primitive list the whole mixed op is one fused kernel sequence
    (bmnas.functions.NodeMixedFn); with a subset / permutation of the four built-in primitives it is the same
    sequence over the present terms (bmnas.functions.NodeMixedSelFn, see node_mix_route); CatConvMish may stand where
    ConcatFC does ("the FC slot").  To feed ONE stacked GEMM, the LinearGLU and FC-slot conv / BatchNorm parameters and
    buffers — when both are in the list — are kept as views into stacked tensors (rows [0, 2C) = LinearGLU, rows
    [2C, 3C) = ConcatFC | CatConvMish, whatever their list order);
    names, shapes and state_dict keys are exactly the reference's (`_ops.<list position>.…`)."""

    def __init__(self, C, L, args):
        super().__init__()
        self._ops = nn.ModuleList(STEP_STEP_OPS[p](C, L, args) for p in STEP_STEP_PRIMITIVES)
        self.C, self.L = C, L
        self._prims = list(STEP_STEP_PRIMITIVES)
        self._default = self._prims == _DEFAULT_PRIMS
        self._stack = None

    def _kind(self, name):
        """The module of built-in primitive `name`, or None when the list does not hold it."""
        return self._ops[self._prims.index(name)] if name in self._prims else None

    def _fc_name(self):
        """The name of the list's FC-slot primitive (ConcatFC | CatConvMish; the first, should a composed list hold
        both), or None."""
        return next((p for p in self._prims if p in _FC_SLOT), None)

    def _fc(self):
        name = self._fc_name()
        return None if name is None else self._kind(name)

    # -- stacked storage ---------------------------------------------------------------
    def _stack_ok(self):
        st = self._stack
        if st is None:
            return False
        glu, cfc = self._kind('LinearGLU'), self._fc()
        C = self.C
        return (glu.conv.weight.data_ptr() == st.W.data_ptr()
                and cfc.conv.weight.data_ptr() == st.W[2 * C:].data_ptr()
                and glu.bn.running_mean.data_ptr() == st.rm.data_ptr()
                and cfc.bn.running_var.data_ptr() == st.rv[2 * C:].data_ptr()
                and glu.bn.weight.data_ptr() == st.bn_w.data_ptr()
                and cfc.conv.bias.data_ptr() == st.bias[2 * C:].data_ptr())

    @torch.no_grad()
    def _restack(self):
        glu, cfc = self._kind('LinearGLU'), self._fc()
        C = self.C
        dev = glu.conv.weight.device

        def stack(a, b, shape_a, shape_b, rows, dtype=torch.float32):
            buf = torch.empty((3 * C,) + rows, device=dev, dtype=dtype)
            buf[:2 * C].copy_(a.detach().reshape((2 * C,) + rows))
            buf[2 * C:].copy_(b.detach().reshape((C,) + rows))
            a.data = buf[:2 * C].view(shape_a)
            b.data = buf[2 * C:].view(shape_b)
            return buf

        W = stack(glu.conv.weight, cfc.conv.weight, (2 * C, 2 * C, 1), (C, 2 * C, 1), (2 * C,))
        bias = stack(glu.conv.bias, cfc.conv.bias, (2 * C,), (C,), ())
        bn_w = stack(glu.bn.weight, cfc.bn.weight, (2 * C,), (C,), ())
        bn_b = stack(glu.bn.bias, cfc.bn.bias, (2 * C,), (C,), ())
        rm = stack(glu.bn.running_mean, cfc.bn.running_mean, (2 * C,), (C,), ())
        rv = stack(glu.bn.running_var, cfc.bn.running_var, (2 * C,), (C,), ())
        nbt = torch.stack([glu.bn.num_batches_tracked.detach().to(dev),
                           cfc.bn.num_batches_tracked.detach().to(dev)])
        glu.bn.num_batches_tracked.data = nbt[0]
        cfc.bn.num_batches_tracked.data = nbt[1]
        self._stack = Pack(W=W, bias=bias, bn_w=bn_w, bn_b=bn_b, rm=rm, rv=rv, nbt=nbt)

    def settle_storage(self):
        """Move the conv + BatchNorm tensors into their stacked storage NOW instead of at the next pack(): a deep copy of
        this module holds clones of the parameters next to a copy of the stack, and whoever keeps the copy's tensor
        addresses (bmnas.optim.AveragedModel under a captured update) needs them final."""
        if self._kind('LinearGLU') is not None and self._fc() is not None and not self._stack_ok():
            self._restack()

    def conv_rows(self):
        """M: rows of the one conv GEMM of this op (2C LinearGLU + C ConcatFC | CatConvMish, as present)."""
        return (2 * self.C if 'LinearGLU' in self._prims else 0) + (self.C if self._fc_name() else 0)

    def pack(self):
        """Parameter pack consumed by bmnas.cell.node_mixed_fwd / node_mixed_sel_fwd: by kind and presence (absent:
        None / p = 0).  stack_*: the conv + BatchNorm storage of the present conv rows — the stacked tensors when
        both convs are in the list, else the one conv's own tensors.  prims names the FC-slot primitive 'ConcatFC'
        (the kind of the selection descriptor), with what it applies behind its BatchNorm in fc_act."""
        attn, glu, cfc = self._kind('ScaleDotAttn'), self._kind('LinearGLU'), self._fc()
        P = Pack(prims=[_slot_name(p) for p in self._prims], M=self.conv_rows(),
                 fc_act=_FC_ACT.get(self._fc_name(), _lib.FC_ACT_RELU),
                 ln_w=None if attn is None else attn.ln.weight.detach(),
                 ln_b=None if attn is None else attn.ln.bias.detach(),
                 attn_p=0.0 if attn is None else attn.dropout.p,
                 glu_p=0.0 if glu is None else glu.dropout.p, fc_p=0.0 if cfc is None else cfc.dropout.p)
        if glu is not None and cfc is not None:
            if not self._stack_ok():
                self._restack()
            st = self._stack
            if glu.bn.momentum != cfc.bn.momentum:           # ONE launch finalises both: one momentum
                raise _lib.BmnasError(
                    f'NodeMixedOp: the stacked BatchNorms share one launch and need one momentum, but '
                    f'{type(glu).__name__}.bn has momentum={glu.bn.momentum!r} and {type(cfc).__name__}.bn has '
                    f'momentum={cfc.bn.momentum!r}')
            P.__dict__.update(stack_W=st.W, stack_bias=st.bias, stack_bn_w=st.bn_w, stack_bn_b=st.bn_b,
                              stack_rm=st.rm, stack_rv=st.rv, stack_nbt=st.nbt, stack_mom=glu.bn.momentum)
        elif glu is not None or cfc is not None:
            m = glu if glu is not None else cfc
            P.__dict__.update(stack_W=m.conv.weight.detach().view(P.M, 2 * self.C), stack_bias=m.conv.bias.detach(),
                              stack_bn_w=m.bn.weight.detach(), stack_bn_b=m.bn.bias.detach(),
                              stack_rm=m.bn.running_mean, stack_rv=m.bn.running_var,
                              stack_nbt=m.bn.num_batches_tracked, stack_mom=m.bn.momentum)
        return P

    def param_list(self):
        """The parameters in named_parameters() order: list position by list position."""
        out = []
        for m in self._ops:
            if isinstance(m, ScaledDotAttn):
                out += [m.ln.weight, m.ln.bias]
            elif isinstance(m, _CatConvBn):
                out += [m.conv.weight, m.conv.bias, m.bn.weight, m.bn.bias]
        return out

    def plan_grads(self, arena):
        C, L, M = self.C, self.L, self.conv_rows()
        attn = 'ScaleDotAttn' in self._prims
        return (arena.ask(M, 2 * C) if M else None, arena.ask(M) if M else None, arena.ask(2 * M) if M else None,
                arena.ask(C, L) if attn else None, arena.ask(C, L) if attn else None)

    def bind_grads(self, arena, h):
        v = [None if i is None else arena.view(i) for i in h]
        return Pack(stack_dW=v[0], stack_dbias=v[1], stack_bn_grad=v[2], dln_w=v[3], dln_b=v[4])

    def grad_pack(self, device):
        arena = Arena()
        h = self.plan_grads(arena)
        arena.alloc(device)
        return self.bind_grads(arena, h)

    def grads_in_param_order(self, G):
        C, M = self.C, self.conv_rows()
        dW, db, bn = G.stack_dW, G.stack_dbias, G.stack_bn_grad
        fo = 2 * C if 'LinearGLU' in self._prims else 0          # first FC-slot row
        out = []
        for p in self._prims:
            if p == 'ScaleDotAttn':
                out += [G.dln_w, G.dln_b]
            elif p == 'LinearGLU':
                out += [dW[:2 * C].view(2 * C, 2 * C, 1), db[:2 * C], bn[0:2 * C], bn[M:M + 2 * C]]
            elif p in _FC_SLOT:
                out += [dW[fo:fo + C].view(C, 2 * C, 1), db[fo:fo + C], bn[fo:fo + C], bn[M + fo:M + fo + C]]
        return out

    def forward(self, x, y, weights):
        route = node_mix_route(self, x, y, weights)
        if route == 'composed':
            return sum(w * op(x, y) for w, op in zip(weights, self._ops))
        w = weights if weights.device == x.device else weights.to(x.device)
        if route == 'selected':
            return NodeMixedSelFn.apply(self, self.training, x, y, w, *self.param_list())
        return NodeMixedFn.apply(self, self.training, x, y, w, *self.param_list())
