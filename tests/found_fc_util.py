"""Shared by the found-network FC-edge tests (tests/test_found_fc_*.py) and tests/golden/make_golden_r11_found_fc.py.

A genotype found over PRIMITIVES = ['none', 'fc_relu', 'fc_mish', 'skip'] names cell-level edges 'fc_relu' / 'fc_mish'
(reference model_search.py:149-155); Found_FusionCell builds them as OPS[name](C, L, args) under `cell._ops.{e}` and
calls them edge by edge (model.py:140-148).  The oracle's found cell knows the default primitives only, so the CPU
restatement lives here: its own step loop over fo.found_node_cell with the oracle's FC op (fo.op_fc).  It is pinned by
the reference's own outputs (tests/golden/fcfound_*.npz, tests/test_found_fc_oracle.py)."""
import glob
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fusion_oracle as fo
from oracle import synth

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
FC = ('fc_relu', 'fc_mish')
MIN_ABS_U = 1e-4            # every stored case keeps its fc_relu pre-activations this far from zero (see the generator)

# cell-level edges of the four genotypes (steps = 2); the step nodes come from the reference's own genotype()
EDGES = {
    # both kinds, two edges reading input 0, every edge FC
    'a': (3, [('fc_relu', 0), ('fc_mish', 0), ('fc_mish', 1), ('fc_relu', 2)]),
    # fc_mish only
    'b': (4, [('fc_mish', 0), ('fc_mish', 3), ('fc_mish', 1), ('fc_mish', 2)]),
    # one FC edge beside a skip edge in each step; input 1 feeds an FC edge and a skip edge
    'c': (3, [('fc_relu', 1), ('skip', 1), ('skip', 2), ('fc_mish', 0)]),
    # hand-written: the fc_relu edge of step 1 reads step 0's output (index N + 0)
    'd': (3, [('skip', 0), ('fc_mish', 1), ('fc_relu', 3), ('skip', 2)]),
}
# (tag, C, L, batch, node_steps, node_multiplier)
SHAPES = {
    's': (16, 4, 3, 1, 1),
    'm': (32, 16, 5, 1, 1),
    'n': (32, 8, 6, 2, 2),
}
# which genotype at which shape: (a) everywhere, the others at the smallest
CASES = [('a', 's'), ('a', 'm'), ('a', 'n'), ('b', 's'), ('c', 's'), ('d', 's'), ('d', 'm')]


def fixture_files():
    return sorted(glob.glob(os.path.join(GOLDEN, 'fcfound_*.npz')))


def load(path):
    z = np.load(path, allow_pickle=False)
    return json.loads(str(z['meta'])), z


def case_cfg(geno, shape, drpt=0.1):
    C, L, batch, ns, nm = SHAPES[shape]
    return fo.make_cfg(N=EDGES[geno][0], C=C, L=L, S=2, M=2, ns=ns, nm=nm, drpt=drpt), batch


def found_fc_param_shapes(cfg, genotype):
    """state_dict() key -> shape of a Found_FusionNetwork whose genotype has FC edges: fo.found_param_shapes plus, per
    fc_relu / fc_mish edge e, the module's tensors under cell._ops.{e} (reference operations.py:22-28, 48-54)."""
    C = cfg.C
    out = {}
    for e, (name, _) in enumerate(genotype.edges):
        if name in FC:
            pre = f'cell._ops.{e}'
            out[pre + '.linear.weight'] = (C, C)
            out[pre + '.linear.bias'] = (C,)
            out[pre + '.bn.weight'] = (C,)
            out[pre + '.bn.bias'] = (C,)
            out[pre + '.bn.running_mean'] = (C,)
            out[pre + '.bn.running_var'] = (C,)
            out[pre + '.bn.num_batches_tracked'] = ()
    out.update(fo.found_param_shapes(cfg, genotype))
    return out


def found_fc_cell(inputs, genotype, p, cfg, training, attn_drop=fo.ATTN_DROP, drpt=None, pre_acts=None):
    """Found_Random_FusionCell.forward (model.py:133-160) with OPS over all four primitives, in the reference's
    execution order: step i's two edges (dropout sites included), then step i's node.  pre_acts: a list that
    receives (edge, |linear output|.min()) of every fc_relu edge."""
    drpt = cfg.drpt if drpt is None else drpt
    names, idx = zip(*genotype.edges)
    states = list(inputs)

    def edge(e):
        x = states[idx[e]]
        if names[e] in FC:
            if pre_acts is not None and names[e] == 'fc_relu':
                u = F.linear(x.transpose(1, 2), p[f'cell._ops.{e}.linear.weight'], p[f'cell._ops.{e}.linear.bias'])
                pre_acts.append((e, float(u.detach().abs().min())))
            return fo.op_fc(x, p, f'cell._ops.{e}', names[e], training, drpt)
        return fo._edge_op(names[e], x)

    node_cfg = fo.Cfg({**cfg, 'drpt': drpt})
    for i in range(cfg.S):
        h1, h2 = edge(2 * i), edge(2 * i + 1)
        states.append(fo.found_node_cell(h1, h2, genotype.steps[i], p, f'cell._step_nodes.{i}.node_cell', node_cfg,
                                         training, attn_drop))
    M = len(genotype.concat)
    out = torch.cat(states[-M:], dim=1)
    ln_w, ln_b = p['cell.ln.weight'], p['cell.ln.bias']
    out = fo._relu(F.layer_norm(out, tuple(ln_w.shape), ln_w, ln_b, fo.EPS))
    return out.view(out.size(0), -1)


def cotangent(seed, shape):
    """The PCG64(seed) cotangent of test_found_network_matches_reference_golden."""
    return torch.from_numpy(np.random.Generator(np.random.PCG64(seed)).standard_normal(tuple(shape))
                            .astype(np.float32))


def restate(cfg, genotype, params, xs, mode, seed, masks=None, dtype=torch.float32):
    """One forward + backward of the restatement -> (feat, {grad:...}, params after the pass).  mode: 'eval' |
    'train_nodrop' | 'train' (live dropout: `masks` are injected in the reference's execution order)."""
    training = mode != 'eval'
    drpt, attn = (0.0, 0.0) if mode == 'train_nodrop' else (cfg.drpt, fo.ATTN_DROP)
    p = {k: (v.clone().to(dtype) if v.is_floating_point() else v.clone()) for k, v in params.items()}
    for k, v in p.items():
        if v.is_floating_point() and not fo.is_buffer(k):
            v.requires_grad_(True)
    xs = [x.clone().to(dtype).requires_grad_(True) for x in xs]
    pre = []
    if masks is not None:
        with fo.injected_masks(masks) as inj:
            feat = found_fc_cell(xs, genotype, p, cfg, training, attn, drpt, pre)
        assert inj.used == len(masks), (inj.used, len(masks))
    else:
        feat = found_fc_cell(xs, genotype, p, cfg, training, attn, drpt, pre)
    (feat * cotangent(seed, feat.shape).to(dtype)).sum().backward()
    grads = {}
    for k, v in p.items():
        if v.requires_grad:
            grads['grad:' + k] = v.grad if v.grad is not None else torch.zeros_like(v)
    for i, x in enumerate(xs):
        grads[f'grad:input.{i}'] = x.grad if x.grad is not None else torch.zeros_like(x)
    return feat.detach(), grads, p, pre


def roundoff_zero_gradients(cfg, genotype, params, xs, mode, seed, masks=None):
    """Keys of the gradients that are mathematically zero without being identically zero.  A BatchNorm in training mode
    removes every per-channel constant of its input, so the bias of a conv in front of it has a zero gradient (the
    'conv.bias' rule of the existing comparisons) — and so has the BatchNorm bias of an FC edge whose output only
    reaches such a conv (the second input of a LinearGLU / ConcatFC step).  What any fp32 evaluation stores there is
    round-off of ~1e-6, the reference's included: a relative comparison of two such tensors says nothing.  Found from
    the math alone: the restatement in float64 leaves them below 1e-9 of the largest gradient (round-off there is
    ~1e-16), every genuine gradient far above.  They are compared with the absolute 1e-4 of the conv.bias rule."""
    _, g64, _, _ = restate(cfg, genotype, params, xs, mode, seed, masks, dtype=torch.float64)
    top = max(float(v.abs().max()) for v in g64.values())
    return {k for k, v in g64.items() if 0.0 < float(v.abs().max()) <= 1e-9 * top}


def assert_gradient(key, got, want, zero, mode, close):
    """One gradient the way test_found_network_matches_reference_golden compares it (rel = 2e-4; a conv bias in front
    of a training-mode BatchNorm in absolute terms), with roundoff_zero_gradients treated like those conv biases."""
    if (key.endswith('conv.bias') and mode != 'eval') or key in zero:
        assert float(got.abs().max()) < 1e-4, key
    else:
        close(key, got, want, rel=2e-4)


def mirror_genotype(genotype):
    from models.search.darts.genotypes import Genotype, StepGenotype
    return Genotype(edges=[tuple(e) for e in genotype.edges],
                    steps=[StepGenotype(inner_edges=[tuple(e) for e in s.inner_edges],
                                        inner_steps=list(s.inner_steps), inner_concat=list(s.inner_concat))
                           for s in genotype.steps],
                    concat=list(genotype.concat))


def build_mirror(cfg, genotype, params, mode, device=None):
    """The project's Found_FusionNetwork over `genotype` with `params` loaded (gpu_util.build_found_net knows no FC
    edge: its parameter shapes come from the oracle)."""
    from gpu_util import Args, set_mode
    from models.search.darts.model import Found_FusionNetwork
    net = Found_FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), None, mirror_genotype(genotype))
    net.load_state_dict(params)
    if device is not None:
        net.to(device)
    set_mode(net, mode)
    return net


def reference_site_order(genotype, cfg):
    """The mirror issues the dropout sites of group 0 (FC edges that read a cell input, genotype order) first, then
    per step: a late FC edge's site, the step node's sites.  The reference runs step i's two edge sites, then step i's
    node sites.  -> perm with reference_order[k] = mirror_order[perm[k]], given the number of live sites of each
    step node."""
    def perm(node_sites):
        names, idx = zip(*genotype.edges)
        fc = [e for e in range(len(names)) if names[e] in FC]
        group0 = [e for e in fc if idx[e] < cfg.N]
        pos, k = {}, 0
        for e in group0:
            pos[('edge', e)] = k
            k += 1
        for i in range(cfg.S):
            for e in (2 * i, 2 * i + 1):
                if e in fc and e not in group0:
                    pos[('edge', e)] = k
                    k += 1
            for t in range(node_sites[i]):
                pos[('node', i, t)] = k
                k += 1
        order = []
        for i in range(cfg.S):
            order += [pos[('edge', e)] for e in (2 * i, 2 * i + 1) if e in fc]
            order += [pos[('node', i, t)] for t in range(node_sites[i])]
        assert sorted(order) == list(range(k))
        return order
    return perm


def node_live_sites(step_genotype, cfg):
    """Live dropout sites of one found step node, in execution order: per inner step one for ScaleDotAttn / LinearGLU /
    ConcatFC, none for Sum; then the out_conv's (node_multiplier != 1)."""
    n = sum(name != 'Sum' for name in step_genotype.inner_steps[:cfg.ns])
    return n + (1 if cfg.nm != 1 else 0)
