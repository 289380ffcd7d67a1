"""Shared by tests/test_node_prims_host.py, test_node_prims_gpu.py and test_node_prims_network_gpu.py: an edited
STEP_STEP_PRIMITIVES list (the fusion primitives a step node mixes) in the modules and in the oracle."""
import contextlib

import numpy as np
import torch

from oracle import fusion_oracle as fo

KINDS = ['Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC']
# the 15 non-empty subsets, in canonical (default-list) order
SUBSETS = [[k for i, k in enumerate(KINDS) if m >> i & 1] for m in range(1, 16)]
PERMUTATIONS = [['ConcatFC', 'Sum'], ['ScaleDotAttn', 'ConcatFC', 'Sum'], ['LinearGLU', 'ScaleDotAttn']]
NEAR = 2e-5


def list_id(prims):
    return '+'.join(prims)


@contextlib.contextmanager
def edited_step_prims(prims):
    """STEP_STEP_PRIMITIVES edited in place (every module holds the same list object) and restored."""
    import models.search.darts.genotypes as gt
    saved = list(gt.STEP_STEP_PRIMITIVES)
    gt.STEP_STEP_PRIMITIVES[:] = prims
    try:
        yield
    finally:
        gt.STEP_STEP_PRIMITIVES[:] = saved


def op_param_shapes(prims, C, L, prefix):
    """state_dict key -> shape of one NodeMixedOp over `prims` (keys `{prefix}.{list position}.…`, registration order:
    node_operations.py:88-90, 25-27, 44-46)."""
    out = {}

    def conv(pre, M):
        out[pre + '.conv.weight'] = (M, 2 * C, 1)
        out[pre + '.conv.bias'] = (M,)
        for k in ('weight', 'bias', 'running_mean', 'running_var'):
            out[f'{pre}.bn.{k}'] = (M,)
        out[pre + '.bn.num_batches_tracked'] = ()

    for i, name in enumerate(prims):
        if name == 'ScaleDotAttn':
            out[f'{prefix}.{i}.ln.weight'] = (C, L)
            out[f'{prefix}.{i}.ln.bias'] = (C, L)
        elif name == 'LinearGLU':
            conv(f'{prefix}.{i}', 2 * C)
        elif name == 'ConcatFC':
            conv(f'{prefix}.{i}', C)
    return out


def node_mixed_general(x, y, gamma_row, p, prefix, prims, training, drpt, attn_drop=fo.ATTN_DROP):
    """NodeMixedOp.forward (node_operations.py:118-120) for an edited STEP_STEP_PRIMITIVES list: sum(w * op(x, y))
    over `prims` in list order (Python's sum starts from 0), parameters under `{prefix}.{list position}`.  Like
    fo.node_mixed_op it leaves num_batches_tracked alone (fo.node_cell counts one level up)."""
    acc = 0
    for i, name in enumerate(prims):
        if name == 'Sum':
            o = fo.op_sum(x, y)
        elif name == 'ScaleDotAttn':
            o = fo.op_scaled_dot_attn(x, y, p[f'{prefix}.{i}.ln.weight'], p[f'{prefix}.{i}.ln.bias'], training, attn_drop)
        elif name == 'LinearGLU':
            o = fo.op_linear_glu(x, y, p, f'{prefix}.{i}', training, drpt)
        elif name == 'ConcatFC':
            o = fo.op_concat_fc(x, y, p, f'{prefix}.{i}', training, drpt)
        else:
            raise KeyError(name)
        acc = acc + gamma_row[i] * o
    return acc


def fc_preactivation(x, y, p, prefix, training):
    """The ReLU input of ConcatFC (node_operations.py:52-54) without touching the running statistics."""
    cat = torch.cat([x, y], dim=1)
    return fo._conv_bn(cat, p[prefix + '.conv.weight'], p[prefix + '.conv.bias'], p[prefix + '.bn.weight'],
                       p[prefix + '.bn.bias'], p[prefix + '.bn.running_mean'].clone(),
                       p[prefix + '.bn.running_var'].clone(), training).detach()


def net_param_shapes(cfg, prims):
    """fo.param_shapes for a network whose NodeMixedOps hold `prims`: the default entries of every `…node_ops.{t}._ops`
    replaced by those of the edited list, in place (registration order)."""
    base = fo.param_shapes(cfg)
    out = {}
    done = set()
    for k, s in base.items():
        if '.node_ops.' in k and '._ops.' in k:
            pre = k[:k.index('._ops.') + len('._ops')]
            if pre not in done:
                done.add(pre)
                out.update(op_param_shapes(prims, cfg.C, cfg.L, pre))
        else:
            out[k] = s
    return out


def patch_oracle(monkeypatch, prims):
    """Swap the edited list into the oracle for whole-network evaluations: fo.node_cell resolves node_mixed_op and
    STEP_STEP_PRIMITIVES (arch shapes, genotype names) by name at call time."""
    def mixed(x, y, gamma_row, p, prefix, training, drpt, attn_drop=fo.ATTN_DROP):
        # fo.node_cell bumps num_batches_tracked of the list positions 2 and 3 (where the default list has its
        # BatchNorms) when those keys exist; a BatchNorm at position 0 or 1 is counted here
        for i, name in enumerate(prims):
            if name in ('LinearGLU', 'ConcatFC') and i not in (2, 3):
                fo._bump_nbt(p, f'{prefix}.{i}.bn.num_batches_tracked', training)
        return node_mixed_general(x, y, gamma_row, p, prefix, prims, training, drpt, attn_drop)
    monkeypatch.setattr(fo, 'node_mixed_op', mixed)
    monkeypatch.setattr(fo, 'STEP_STEP_PRIMITIVES', list(prims))


# ------------------------------------------------------------------------------------- one NodeMixedOp
PREFIX = 'op._ops'
# (list, b, C, L, same) whose first seed(s) put a ConcatFC pre-activation within 4 NEAR of zero in the fp32 or the
# float64 oracle: those cases draw from a later seed instead (checked on the CPU, see test_node_prims_gpu's docstring)
SEED_SALT = {('ConcatFC+Sum', 3, 32, 16, True): 1, ('ConcatFC+Sum', 6, 192, 16, True): 6,
             ('ConcatFC+Sum', 7, 128, 8, False): 1, ('ScaleDotAttn+ConcatFC+Sum', 6, 192, 16, True): 2,
             ('ConcatFC+ScaleDotAttn+Sum+LinearGLU', 8, 32, 16, True): 1}


def case_seed(prims, b, C, L, same):
    code = sum((i + 1) * (KINDS.index(q) + 1) for i, q in enumerate(prims))
    return 700 + 13 * code + b + C + L + SEED_SALT.get((list_id(prims), b, C, L, same), 0)


def make_case(prims, b, C, L, same, seed=None):
    """-> (p, x, y, gamma, g): synthetic parameters of one NodeMixedOp over `prims` (keys PREFIX.{i}.…), inputs
    (y is x when same), a softmaxed weight row of len(prims) and the output gradient."""
    from oracle import synth
    seed = case_seed(prims, b, C, L, same) if seed is None else seed
    p = synth.make_params(None, seed, op_param_shapes(prims, C, L, PREFIX))
    rng = np.random.Generator(np.random.PCG64(seed + 77))
    r = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))
    x = r(b, C, L)
    y = x if same else r(b, C, L)
    gamma = torch.softmax(r(len(prims)), -1)
    return p, x, y, gamma, r(b, C, L)


def oracle_op(prims, p, x, y, gamma, g, same, training, drpt=0.0, attn_drop=0.0, masks=None, flips=(), double=False):
    """One oracle evaluation of the op and its backward -> (out, dgamma, dx, dy | None, params with .grad / buffers)."""
    f = (lambda t: t.double() if t.is_floating_point() else t) if double else (lambda t: t)
    po = {k: (f(v).clone() if fo.is_buffer(k) else f(v).clone().requires_grad_(True)) for k, v in p.items()}
    xo = f(x).clone().requires_grad_(True)
    yo = xo if same else f(y).clone().requires_grad_(True)
    wo = f(gamma).clone().requires_grad_(True)
    inj = fo.injected_masks(masks) if masks else contextlib.nullcontext()
    with inj, fo.relu_decisions(0.0, flips):
        out = node_mixed_general(xo, yo, wo, po, PREFIX, prims, training, drpt, attn_drop)
    if masks:
        assert inj.used == len(masks)
    out.backward(f(g))
    return out.detach(), wo.grad, xo.grad, None if same else yo.grad, po


def min_fc_margin(prims, p, x, y, training):
    """min |ConcatFC pre-activation| of the fp32 and of the float64 oracle (inf without ConcatFC)."""
    if 'ConcatFC' not in prims:
        return float('inf')
    pre = f'{PREFIX}.{prims.index("ConcatFC")}'
    u32 = fc_preactivation(x, y, p, pre, training)
    p64 = {k: (v.double() if v.is_floating_point() else v) for k, v in p.items()}
    u64 = fc_preactivation(x.double(), y.double(), p64, pre, training)
    return min(float(u32.abs().min()), float(u64.abs().min()))
