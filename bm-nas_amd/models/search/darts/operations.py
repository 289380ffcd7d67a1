"""Cell-level edge primitives and the architecture-weighted mixed edge.

Mirror of the reference's models/search/darts/operations.py (OPS :7-12, Zero :14-20,
FC_Relu :22-38, FC_Mish :48-65, Identity :88-93, FusionMixedOp :95-105) on the gfx950
kernels: with the default PRIMITIVES ['none', 'skip'] the mixed edge is the HIP mixsum
kernel (bmnas_mixsum_fwd/bwd).  FC_Relu / FC_Mish are not in the default search space
(SURVEY.md a14): they stay ordinary PyTorch modules (same state_dict keys, usable alone), and the
sum over the incoming edges of a cell / node step runs them on the grouped kernels of
csrc/fcedge.hip (bmnas.functions.FcEdgeSumFn) — general_edge_sum below.  The fc_relu / fc_mish edges of a FOUND
cell (each with an output of its own) run on the same file's grouped kernels through found_fc_route /
found_fc_apply (bmnas.functions.FoundFcEdgesFn).  Attention (:67-86, the reference's unregistered "step node operation":
nn.MultiheadAttention over (b, C, L) tensors) runs on projection GEMMs and the per-head core of csrc/mha.hip
(bmnas.functions.MhaFn; attention_route).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from bmnas import lib
from bmnas.functions import FC_KINDS, FcEdgeSumFn, FoundFcEdgesFn, MhaFn, MixSumFn

from .genotypes import *  # noqa: F401,F403
from .genotypes import PRIMITIVES

OPS = {
    'none': lambda C, L, args: Zero(),
    'fc_relu': lambda C, L, args: FC_Relu(C, L, args),
    'fc_mish': lambda C, L, args: FC_Mish(C, L, args),
    'skip': lambda C, L, args: Identity(),
}


class Zero(nn.Module):
    def forward(self, x):
        return x.mul(0.)


class Identity(nn.Module):
    def forward(self, x):
        return x


class Mish(nn.Module):
    def forward(self, x):
        return x * torch.tanh(F.softplus(x))


class _FCBase(nn.Module):
    """Linear over the channel dim -> activation -> BatchNorm1d -> Dropout."""

    def __init__(self, C, L, args):
        super().__init__()
        self.linear = nn.Linear(C, C)
        self.bn = nn.BatchNorm1d(C)
        self.dropout = nn.Dropout(args.drpt)

    def _act(self, x):
        raise NotImplementedError

    def forward(self, x):
        out = self.linear(x.transpose(1, 2)).transpose(1, 2)
        return self.dropout(self.bn(self._act(out)))


class FC_Relu(_FCBase):
    def _act(self, x):
        return F.relu(x)


class FC_Mish(_FCBase):
    def __init__(self, C, L, args):
        super().__init__(C, L, args)
        self.mish = Mish()

    def _act(self, x):
        return self.mish(x)


# False: Attention.forward always takes the reference's own composition around nn.MultiheadAttention (A/B timing, tests)
MHA_NATIVE = True
# the classes whose forward IS the reference's: Attention here, MultiHeadAttn in node_operations.py.  Anybody else's
# subclass may have changed what forward means and keeps the composed route.
_MHA_CLASSES = []


def attention_route(module, q, k, v):
    """Which path Attention.forward(q, k, v) takes: 'native' (bmnas.functions.MhaFn: projection GEMMs + the per-head
    core of csrc/mha.hip) or 'composed' (the reference's transposes around self.attn(..., need_weights=False)) — for a
    subclass, an edited self.attn (kdim / vdim, bias=False, add_bias_kv, add_zero_attn, batch_first), inputs that are
    not three fp32 (b, C, L) tensors of one shape and device, or a shape outside lib.mha_ok.  Host logic only: CPU
    tensors are routed like any others, and the native forward then refuses them."""
    if not MHA_NATIVE or type(module) not in _MHA_CLASSES:
        return 'composed'
    a = module.attn
    if type(a) is not nn.MultiheadAttention or type(a.out_proj) is not nn.modules.linear.NonDynamicallyQuantizableLinear:
        return 'composed'
    if (not a._qkv_same_embed_dim or a.in_proj_weight is None or a.in_proj_bias is None or a.out_proj.bias is None
            or a.bias_k is not None or a.bias_v is not None or a.add_zero_attn or a.batch_first):
        return 'composed'
    ts = (q, k, v)
    if not all(torch.is_tensor(t) and t.dim() == 3 and t.dtype == torch.float32 for t in ts):
        return 'composed'
    if any(t.shape != q.shape or t.device != q.device for t in ts):
        return 'composed'
    params = (a.in_proj_weight, a.in_proj_bias, a.out_proj.weight, a.out_proj.bias)
    if any(w.dtype != torch.float32 or w.device != q.device for w in params):
        return 'composed'
    b, C, L = q.shape
    if C != a.embed_dim or a.head_dim * a.num_heads != a.embed_dim or not 0.0 <= a.dropout < 1.0:
        return 'composed'
    if not lib.mha_ok(b, C, L, a.num_heads):
        return 'composed'
    return 'native'


class Attention(nn.Module):
    """Multi-head attention over (b, C, L) tensors: the L positions are the tokens, the C channels the features
    (reference operations.py:67-86, "step node operation").  Parameters, their initialisation and the state_dict keys
    are nn.MultiheadAttention's (attn.in_proj_weight, attn.in_proj_bias, attn.out_proj.weight, attn.out_proj.bias); the
    forward runs on the gfx950 kernels (attention_route)."""

    def __init__(self, embed_dim, num_heads, drpt):
        super().__init__()
        self.attn = nn.MultiheadAttention(embed_dim, num_heads, drpt)

    def forward(self, q, k, v):
        if attention_route(self, q, k, v) == 'composed':
            q, k, v = (t.transpose(0, 1).transpose(0, 2) for t in (q, k, v))
            out = self.attn(q, k, v, need_weights=False)[0]
            return out.transpose(0, 2).transpose(0, 1)
        a = self.attn
        uniq, roles = [], []
        for t in (q, k, v):
            i = next((j for j, u in enumerate(uniq) if u is t), len(uniq))
            if i == len(uniq):
                uniq.append(t)
            roles.append(i)
        return MhaFn.apply(a.num_heads, a.dropout, a.training, tuple(roles), a.in_proj_weight, a.in_proj_bias,
                           a.out_proj.weight, a.out_proj.bias, *uniq)


_MHA_CLASSES.append(Attention)


class FusionMixedOp(nn.Module):
    """sum_p weights[p] * op_p(x) over PRIMITIVES (reference operations.py:95-105)."""

    def __init__(self, C, L, args):
        super().__init__()
        self._ops = nn.ModuleList(OPS[p](C, L, args) for p in PRIMITIVES)
        self._prims = list(PRIMITIVES)
        self._default = self._prims == ['none', 'skip']

    def forward(self, x, weights):
        if self._default:
            # w_none * (x * 0) + w_skip * x: the 'none' term vanishes for finite x
            w = weights if weights.device == x.device else weights.to(x.device)
            return MixSumFn.apply(w[1:2], x)
        return sum(w * op(x) for w, op in zip(weights, self._ops))


def mixed_edge_sum(states, weights, offset):
    """sum_j FusionMixedOp_j(states[j], weights[offset + j]) as ONE HIP kernel
    (reference model_search.py:58 / node_search.py:54)."""
    n = len(states)
    w = weights if weights.device == states[0].device else weights.to(states[0].device)
    return MixSumFn.apply(w[offset:offset + n, 1], *states)


FC_EDGES_NATIVE = True      # False: general_edge_sum and the found cell's FC edges always compose (A/B timing, tests)
_BUILTIN = {'none': Zero, 'skip': Identity, 'fc_relu': FC_Relu, 'fc_mish': FC_Mish}


def participating_primitives(primitives, n_cols):
    """The primitives a FusionMixedOp evaluates for a weight row of n_cols columns: `zip(weights, self._ops)`
    (reference operations.py:105) stops at the shorter sequence, so a NodeCell's inner rows — always
    len(STEP_EDGE_PRIMITIVES) = 2 columns — reach only the first two entries of an edited PRIMITIVES list."""
    return list(primitives[:n_cols])


def _composed_edge_sum(ops, states, weights, offset):
    return sum(ops[offset + j](h, weights[offset + j]) for j, h in enumerate(states))


def edge_sum_route(ops, states, weights, offset):
    """How general_edge_sum evaluates this sum: 'fc' (FcEdgeSumFn), 'mixsum' (no FC primitive takes part: the K1
    kernel over the skip column) or 'composed' (op by op — primitives registered by a user, shapes outside the
    kernels' limits, CPU tensors)."""
    n = len(states)
    mods = [ops[offset + j] for j in range(n)]
    x = states[0]
    if not (FC_EDGES_NATIVE and x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and weights.dim() == 2
            and all(h.shape == x.shape for h in states)):
        return 'composed', None
    prims = participating_primitives(mods[0]._prims, weights.shape[-1])
    for m in mods:
        if m._prims != mods[0]._prims or len(m._ops) != len(m._prims):
            return 'composed', None
        # the registry may have been edited: only the four built-in classes have kernels
        if any(name not in _BUILTIN or type(op) is not _BUILTIN[name] for name, op in zip(prims, m._ops)):
            return 'composed', None
    F = sum(name in FC_KINDS for name in prims)
    if F == 0:
        return ('mixsum', prims) if prims.count('skip') == 1 else ('composed', None)
    fcs = [op for m in mods for name, op in zip(prims, m._ops) if name in FC_KINDS]
    same_mode = all(op.training == fcs[0].training and op.bn.training == fcs[0].training
                    and op.dropout.training == fcs[0].training
                    and op.dropout.p == fcs[0].dropout.p and op.bn.track_running_stats
                    and op.bn.momentum == 0.1 and op.bn.eps == 1e-5 and op.bn.affine for op in fcs)
    b, Cc, L = x.shape
    if not same_mode or not lib.fc_edges_ok(n, F, len(prims), b, Cc, L):
        return 'composed', None
    return 'fc', prims


def general_edge_sum(ops, states, weights, offset):
    """sum_j ops[offset + j](states[j], weights[offset + j]) for FusionMixedOps built from an edited PRIMITIVES
    list (reference model_search.py:58 / node_search.py:54)."""
    route, prims = edge_sum_route(ops, states, weights, offset)
    if route == 'composed':
        return _composed_edge_sum(ops, states, weights, offset)
    n = len(states)
    w = weights if weights.device == states[0].device else weights.to(states[0].device)
    if route == 'mixsum':
        return MixSumFn.apply(w[offset:offset + n, prims.index('skip')], *states)
    rows = w if offset == 0 and n == w.shape[0] else w[offset:offset + n]
    return fc_edge_sum_apply(ops, states, rows, prims, offset)


def fc_edge_sum_apply(ops, states, rows, prims, offset=0):
    """FcEdgeSumFn over the FC modules of ops[offset : offset + len(states)]; rows: their (n, len(prims)) weights."""
    n = len(states)
    fcs = [[op for name, op in zip(prims, ops[offset + j]._ops) if name in FC_KINDS] for j in range(n)]
    params, buffers = [], []
    for row in fcs:
        for op in row:
            params += [op.linear.weight, op.linear.bias, op.bn.weight, op.bn.bias]
        buffers.append([(op.bn.running_mean, op.bn.running_var, op.bn.num_batches_tracked) for op in row])
    return FcEdgeSumFn.apply(n, tuple(prims), fcs[0][0].training, fcs[0][0].dropout.p, buffers, rows, *states, *params)


def found_fc_route(ops, xs):
    """How a found cell evaluates the FC edges `ops` (FC_Relu / FC_Mish modules) over their sources `xs`: 'fc'
    (FoundFcEdgesFn: one group of launches) or 'composed' (op(x) edge by edge — subclassed modules, shapes outside
    the kernels' limits, CPU tensors, modules in different modes).  Host logic only."""
    if not (FC_EDGES_NATIVE and len(ops) > 0 and len(ops) == len(xs)):
        return 'composed'
    if any(type(op) is not FC_Relu and type(op) is not FC_Mish for op in ops):
        return 'composed'
    x = xs[0]
    if not (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3
            and all(h.is_cuda and h.dtype == x.dtype and h.shape == x.shape for h in xs)):
        return 'composed'
    t = ops[0].training
    same_mode = all(op.training == t and op.bn.training == t and op.dropout.training == t
                    and op.dropout.p == ops[0].dropout.p and op.bn.track_running_stats and op.bn.affine
                    and op.bn.momentum == 0.1 and op.bn.eps == 1e-5 and op.bn.running_mean is not None
                    for op in ops)
    b, Cc, L = x.shape
    if not same_mode or not lib.fc_edges_ok(len(ops), 1, 1, b, Cc, L):
        return 'composed'
    return 'fc'


def found_fc_apply(ops, xs):
    """FoundFcEdgesFn over the FC modules `ops` and their sources `xs` -> one output per edge."""
    params, buffers = [], []
    for op in ops:
        params += [op.linear.weight, op.linear.bias, op.bn.weight, op.bn.bias]
        buffers.append((op.bn.running_mean, op.bn.running_var, op.bn.num_batches_tracked))
    kinds = tuple(1 if type(op) is FC_Mish else 0 for op in ops)
    return FoundFcEdgesFn.apply(len(ops), kinds, ops[0].training, ops[0].dropout.p, buffers, *xs, *params)
