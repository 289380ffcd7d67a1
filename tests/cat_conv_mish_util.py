"""Shared by the tests/test_cat_conv_mish_*.py files: the CatConvMish step-node primitive (reference
models/search/darts/node_operations.py:58-82, cat -> Conv1d(2C, C, 1) -> BatchNorm1d(C) -> Mish -> Dropout) restated
over the oracle's helpers and registered in STEP_STEP_OPS the way a user registers it.

Its parameters have ConcatFC's shapes and keys, so shapes and synthetic parameters come from the existing helpers with
'ConcatFC' substituted for the name; every case passes its own seed to make_case (node_prims_util.case_seed and its
salts exist to keep ReLU inputs away from zero, which Mish does not need)."""
import contextlib

import torch
import torch.nn.functional as F

import node_prims_util as npu
from oracle import fusion_oracle as fo

MISH = 'CatConvMish'
PREFIX = npu.PREFIX
BUILTIN4 = ['Sum', 'ScaleDotAttn', 'LinearGLU', MISH]
# the 8 subsets that hold CatConvMish, in canonical order
SUBSETS = [[k for i, k in enumerate(BUILTIN4) if m >> i & 1] for m in range(8, 16)]
PERMUTATIONS = [[MISH, 'Sum'], ['ScaleDotAttn', MISH, 'Sum'], ['LinearGLU', MISH, 'ScaleDotAttn', 'Sum']]
LIVE = [MISH, 'ScaleDotAttn', 'Sum', 'LinearGLU']
list_id = npu.list_id
edited_step_prims = npu.edited_step_prims


def substituted(prims):
    return ['ConcatFC' if p == MISH else p for p in prims]


@contextlib.contextmanager
def registered():
    """STEP_STEP_OPS['CatConvMish'] for the duration, the one line a user of the reference adds."""
    import models.search.darts.node_operations as no
    assert MISH not in no.STEP_STEP_OPS
    no.STEP_STEP_OPS[MISH] = lambda C, L, args: no.CatConvMish(C, args)
    try:
        yield
    finally:
        del no.STEP_STEP_OPS[MISH]


@contextlib.contextmanager
def mish_list(prims):
    with registered(), edited_step_prims(prims):
        yield


def mish(u):
    return u * torch.tanh(F.softplus(u))


def op_cat_conv_mish(x, y, p, prefix, training, drpt):
    """CatConvMish.forward (node_operations.py:74-82)."""
    cat = torch.cat([x, y], dim=1)
    u = fo._conv_bn(cat, p[prefix + '.conv.weight'], p[prefix + '.conv.bias'], p[prefix + '.bn.weight'],
                    p[prefix + '.bn.bias'], p[prefix + '.bn.running_mean'], p[prefix + '.bn.running_var'], training)
    return fo._dropout(mish(u), drpt, training)


def op_param_shapes(prims, C, L, prefix):
    return npu.op_param_shapes(substituted(prims), C, L, prefix)


def node_mixed_general(x, y, gamma_row, p, prefix, prims, training, drpt, attn_drop=fo.ATTN_DROP):
    """node_prims_util.node_mixed_general with CatConvMish among the names."""
    acc = 0
    for i, name in enumerate(prims):
        if name == MISH:
            o = op_cat_conv_mish(x, y, p, f'{prefix}.{i}', training, drpt)
        else:
            o = _one(name, x, y, p, f'{prefix}.{i}', training, drpt, attn_drop)
        acc = acc + gamma_row[i] * o
    return acc


def _one(name, x, y, p, pre, training, drpt, attn_drop):
    if name == 'Sum':
        return fo.op_sum(x, y)
    if name == 'ScaleDotAttn':
        return fo.op_scaled_dot_attn(x, y, p[pre + '.ln.weight'], p[pre + '.ln.bias'], training, attn_drop)
    if name == 'LinearGLU':
        return fo.op_linear_glu(x, y, p, pre, training, drpt)
    if name == 'ConcatFC':
        return fo.op_concat_fc(x, y, p, pre, training, drpt)
    raise KeyError(name)


def make_case(prims, b, C, L, same, seed):
    return npu.make_case(substituted(prims), b, C, L, same, seed=seed)


def oracle_op(prims, p, x, y, gamma, g, same, training, drpt=0.0, attn_drop=0.0, masks=None, double=False):
    """One evaluation of the restated op and its backward -> (out, dgamma, dx, dy | None, params with .grad / buffers);
    double: in float64."""
    f = (lambda t: t.double() if t.is_floating_point() else t) if double else (lambda t: t)
    po = {k: (f(v).clone() if fo.is_buffer(k) else f(v).clone().requires_grad_(True)) for k, v in p.items()}
    xo = f(x).clone().requires_grad_(True)
    yo = xo if same else f(y).clone().requires_grad_(True)
    wo = f(gamma).clone().requires_grad_(True)
    inj = fo.injected_masks(masks) if masks else contextlib.nullcontext()
    with inj:
        out = node_mixed_general(xo, yo, wo, po, PREFIX, prims, training, drpt, attn_drop)
    if masks:
        assert inj.used == len(masks)
    out.backward(f(g))
    return out.detach(), wo.grad, xo.grad, None if same else yo.grad, po


# ------------------------------------------------------------------------------------- whole networks
def net_param_shapes(cfg, prims):
    """node_prims_util.net_param_shapes for a hypernet whose NodeMixedOps hold `prims`."""
    return npu.net_param_shapes(cfg, substituted(prims))


def patch_oracle(monkeypatch, prims):
    """node_prims_util.patch_oracle with CatConvMish among the names: fo.node_cell resolves node_mixed_op and
    STEP_STEP_PRIMITIVES (arch shapes, genotype names) by name at call time."""
    def mixed(x, y, gamma_row, p, prefix, training, drpt, attn_drop=fo.ATTN_DROP):
        # fo.node_cell counts the BatchNorms at list positions 2 and 3 itself; one at position 0 or 1 is counted here
        for i, name in enumerate(prims):
            if name in ('LinearGLU', 'ConcatFC', MISH) and i not in (2, 3):
                fo._bump_nbt(p, f'{prefix}.{i}.bn.num_batches_tracked', training)
        return node_mixed_general(x, y, gamma_row, p, prefix, prims, training, drpt, attn_drop)
    monkeypatch.setattr(fo, 'node_mixed_op', mixed)
    monkeypatch.setattr(fo, 'STEP_STEP_PRIMITIVES', list(prims))


def substituted_genotype(g):
    """The genotype with ConcatFC named where CatConvMish is: fo.found_param_shapes of it are the network's."""
    return fo.Genotype(edges=g.edges, concat=g.concat,
                       steps=[fo.StepGenotype(s.inner_edges, substituted(s.inner_steps), s.inner_concat)
                              for s in g.steps])


def patch_found_oracle(monkeypatch):
    """fo.found_node_cell resolves _found_node_op by name at call time: teach it the name."""
    plain = fo._found_node_op

    def found_node_op(name, x, y, p, prefix, training, drpt, attn_drop):
        if name != MISH:
            return plain(name, x, y, p, prefix, training, drpt, attn_drop)
        r = op_cat_conv_mish(x, y, p, prefix, training, drpt)
        fo._bump_nbt(p, prefix + '.bn.num_batches_tracked', training)
        return r
    monkeypatch.setattr(fo, '_found_node_op', found_node_op)
