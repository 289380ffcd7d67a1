"""float64 statement of torch.optim.SGD (momentum, dampening, nesterov, L2 weight decay; maximize off) as the one-launch
SGD step computes it (include/bmnas_hip.h: bmnas_sgd_multi; bmnas.optim.SGD), in numpy, written from the definition:

    g   = c * grad                      clipping (tests/clip_ref.py), over all tensors together, before the decay
    g   = g + wd * p                    only if wd != 0
    buf = g                             a tensor's FIRST step with momentum (no dampening)
    buf = buf * mu + (1 - damp) * g     every later one
    g   = g + mu * buf  (nesterov)  or  buf
    p   = p - lr * g

and pinned to torch itself by tests/test_sgd_ref.py.  `dtype=np.float32` evaluates the same sequence with every operation
rounded to fp32 on its own — what the kernel does (no fused multiply-add): the bit-for-bit reference of the GPU tests.

Also here, shared by tests/test_sgd_ref.py and tests/test_sgd_gpu.py: the layout of tests/test_adam_variants_gpu.py
(SHAPES, two groups, the second with lr 3e-3, parameter 2 joining at step 2, lr *= 0.9 per step, 6 steps, step s's
gradients times MULT[s]), the configurations compared, and torch's float64 run of each."""
import numpy as np
import torch

import clip_ref

SHAPES = [(384, 384, 1), (384,), (7,), (1,), (13, 2), (3, 5, 11), (4099,), (192, 16)]
MULT = [10, 10, 1, 0.1, 0.1, 1]
LR, LR2, STEPS = 1e-2, 3e-3, 6

# name -> constructor arguments (+ max_norm, + what the second group overrides)
CASES = {
    'plain': dict(momentum=0.0),
    'momentum': dict(momentum=0.9),
    'dampening': dict(momentum=0.9, dampening=0.5),
    'nesterov': dict(momentum=0.9, nesterov=True),
    'decay': dict(momentum=0.9, weight_decay=0.1),
    'clipped': dict(momentum=0.9, max_norm=5.0),
    'groups': dict(momentum=0.9, dampening=0.5, group2=dict(momentum=0.5, dampening=0.1)),
}
# the configuration each one could be confused with
NEIGHBOUR = {'momentum': 'plain', 'dampening': 'momentum', 'nesterov': 'momentum', 'decay': 'momentum',
             'clipped': 'momentum', 'groups': 'momentum'}


def _arr(t, dtype):
    return np.asarray(t.detach().cpu().numpy() if hasattr(t, 'detach') else t, dtype=dtype)


def sgd_step(p, g, buf, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, dtype=np.float64, plain_terms=False):
    """One torch.optim.SGD update of one tensor -> (p, buf).  buf None: the tensor's first step (or no momentum, then
    None comes back).  The scalars are formed in double and cast to `dtype`, as the host stages them.
    plain_terms: leave the dampening product out of the sequence altogether (buf * mu + g) — what dampening == 0 must
    equal bit for bit."""
    p, g = _arr(p, dtype), _arr(g, dtype)
    s = lambda x: dtype(x)
    if wd != 0:
        g = g + s(wd) * p
    if momentum != 0:
        if buf is None:
            buf = g.copy()
        elif plain_terms:
            assert dampening == 0
            buf = _arr(buf, dtype) * s(momentum) + g
        else:
            buf = _arr(buf, dtype) * s(momentum) + s(1 - dampening) * g
        g = g + s(momentum) * buf if nesterov else buf
    return p + s(-lr) * g, (buf if momentum != 0 else None)


def clipped_sgd_step(params, grads, bufs, lrs, max_norm=None, momenta=0.0, dampenings=0.0, wds=0.0, nesterov=False,
                     dtype=np.float64, plain_terms=False):
    """Clip over ALL tensors together (max_norm None: no clipping), then SGD tensor by tensor; lrs / momenta / dampenings /
    wds per tensor (or one value for all).  A tensor whose gradient is None is returned unchanged — parameter AND buffer:
    its first step is still to come.  -> (params, bufs, pre-clip norm or None)"""
    n = len(params)
    per = lambda x: list(x) if isinstance(x, (list, tuple)) else [x] * n
    lrs, momenta, dampenings, wds = per(lrs), per(momenta), per(dampenings), per(wds)
    norm = None
    if max_norm is not None:
        grads, norm = clip_ref.clip(grads, max_norm)
    out_p, out_b = [], []
    for i in range(n):
        if grads[i] is None:
            out_p.append(_arr(params[i], dtype))
            out_b.append(bufs[i])
            continue
        p, b = sgd_step(params[i], grads[i], bufs[i], lrs[i], momenta[i], dampenings[i], wds[i], nesterov, dtype,
                        plain_terms)
        out_p.append(p)
        out_b.append(b)
    return out_p, out_b, norm


# ------------------------------------------------------------------------------------------------------------ the layout
def make(seed, shapes=SHAPES, mult=1.0):
    g = torch.Generator().manual_seed(seed)
    return [mult * torch.randn(*s, generator=g) for s in shapes]


def groups(ps, cfg=None):
    """two groups, the second with lr 3e-3 (and the overrides of cfg['group2'])"""
    return [{'params': ps[:3]}, dict({'params': ps[3:], 'lr': LR2}, **(cfg or {}).get('group2', {}))]


def ctor_args(cfg):
    return {k: v for k, v in cfg.items() if k not in ('max_norm', 'group2')}


def grads_of(step, shapes=SHAPES, seed=100, late=True):
    """step's fp32 gradients; parameter 2 has none before step 2"""
    gs = make(seed + step, shapes, MULT[step % len(MULT)])
    if late and step < 2:
        gs[2] = None
    return gs


def decay_lr(*opts):
    for grps in zip(*[o.param_groups for o in opts]):
        lr = grps[0]['lr'] * 0.9
        for g in grps:
            g['lr'] = lr


def torch_run(cfg, seed=1, steps=STEPS):
    """torch.optim.SGD on the CPU in float64 over the layout -> (parameters, optimizer)"""
    cpu = [t.double().requires_grad_(True) for t in make(seed)]
    ref = torch.optim.SGD(groups(cpu, cfg), lr=LR, **ctor_args(cfg))
    for step in range(steps):
        for p, g in zip(cpu, grads_of(step)):
            p.grad = None if g is None else g.double()
        decay_lr(ref)
        if cfg.get('max_norm') is not None:
            torch.nn.utils.clip_grad_norm_(cpu, cfg['max_norm'])
        ref.step()
    return cpu, ref


_TORCH = {}


def torch_cached(name):
    """One float64 run per configuration of CASES, shared and left unchanged."""
    if name not in _TORCH:
        _TORCH[name] = torch_run(CASES[name])
    return _TORCH[name]


def ref_run(cfg, seed=1, steps=STEPS, dtype=np.float64, plain_terms=False):
    """The statement above over the same layout -> (parameters, buffers (None: not stepped), pre-clip norms)"""
    P = [_arr(t, dtype) for t in make(seed)]
    B = [None] * len(P)
    g2 = cfg.get('group2', {})
    pick = lambda k: [cfg.get(k, 0.0)] * 3 + [g2.get(k, cfg.get(k, 0.0))] * (len(P) - 3)
    lrs = [LR] * 3 + [LR2] * (len(P) - 3)
    norms = []
    for step in range(steps):
        lrs = [lr * 0.9 for lr in lrs]
        P, B, n = clipped_sgd_step(P, grads_of(step), B, lrs, cfg.get('max_norm'), pick('momentum'), pick('dampening'),
                                   pick('weight_decay'), cfg.get('nesterov', False), dtype, plain_terms)
        norms.append(n)
    return P, B, norms


def distance(a, b):
    """worst |a - b| / scale over the parameters of two float64 torch runs"""
    return max(float((x.detach() - y.detach()).abs().max()) / (float(y.detach().abs().max()) + 1e-3) for x, y in zip(a, b))
