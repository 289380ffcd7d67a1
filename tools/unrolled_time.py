#!/usr/bin/env python3
"""One eager unrolled (second-order) architecture step — models.search.darts.architect.Architect with args.unrolled, the
weight-side arithmetic on the kernels of csrc/unroll.hip (bmnas.optim.UnrolledStep) — beside the same step COMPOSED from
torch ops on the same commit and the same live model, the way DARTS' architect.py writes it:

    kernels    Architect.step(valid batch, input_train=..., target_train=...)
    composed   theta = _concat(w); moment = _concat(momentum_buffer).mul_(mu); dtheta = _concat(g) + wd * theta;
               theta.sub(moment + dtheta, alpha=eta) copied back tensor by tensor; a copy_ backup and restore per tensor;
               R = r / _concat(v).norm(); p.data.addcmul_(v, R) / addcmul_(v, R, value=-2) per tensor (one launch each, R
               stays on the device: no host synchronisation, which DARTS' own `p.data.add_(R, v)` would add);
               (x - y).div_(2 * R); g.sub_(ig, alpha=eta) per alpha tensor

Both run the same four forward / backward passes (K.weight_grads_only / K.arch_grads_only as the Architect sets them, the
+ and - passes over the same dropout masks) and end in the same bmnas.optim.Adam step on alpha: what differs is the
weight-side arithmetic.  The weight optimizer is bmnas.optim.SGD(lr 1e-2, momentum 0.9, weight_decay 3e-4) after one real
step (the momentum buffers exist).

    python tools/unrolled_time.py      # MM-IMDB b128 and NTU b64.  A case = one child process; the two versions ALTERNATE
                                       # region by region, five timed regions of 20 steps each (device events, after
                                       # warm-up): medians, spreads (max - min), device events per step of both
No time is a pass / fail criterion: the composed version is the yardstick, and a kernel-side version that does not use
fewer device events and less wall time than it is a finding to report.  Every case is a child process under its own time
limit, and the tool stops at the first one that does not exit with 0: nothing more is started on the GPU after it.  A
step = train mode with dropout on, bench.CONFIGS shapes, bench.synth_batch data (train batch seed 0, valid batch seed 1).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))

CASES = [('mmimdb', 128), ('ntu', 64)]
CASE_SECONDS = 420
REGIONS, WARMUP, PER = 5, 3, 20
ETA, MU, WD, R0 = 1e-2, 0.9, 3e-4, 1e-2


def _concat(xs):
    import torch
    return torch.cat([x.reshape(-1) for x in xs])


class _Args:
    weight_decay = WD
    hip_graph = False
    unrolled = True
    unrolled_r = R0


def build(cname, batch):
    """-> (architect, weights, arch, (xt, yt), (xv, yv)) on a fresh model: the weight optimizer has taken one real step."""
    import torch
    import bench as B
    from bmnas import nn as bnn
    from bmnas.optim import SGD, Adam
    from models.search.darts.architect import Architect
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    torch.manual_seed(2)
    model = B.HyperNet(c, 'F', cname).to(dev).train()
    crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
    batches = []
    for seed in (0, 1):
        xs, y = B.synth_batch(c, batch, dev, seed)
        batches.append(([x.detach() for x in xs], y))
    arch = list(model.arch_parameters())
    crit(model(batches[0][0]), batches[0][1]).backward()
    # (the tensors the loss reaches: DARTS' _concat has no place for a missing gradient)
    weights = [p for p in model.parameters() if p.grad is not None and not any(p is a for a in arch)]
    w_opt = SGD(weights, lr=ETA, momentum=MU, weight_decay=WD)
    a_opt = Adam(arch, lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-3)
    w_opt.step()
    w_opt.zero_grad()
    for a in arch:
        a.grad = None
    architect = Architect(model, _Args(), crit, a_opt, network_optimizer=w_opt)
    return architect, weights, arch, batches[0], batches[1]


def composed_step(architect, weights, arch, train, valid, backups):
    """DARTS' statements with torch ops on the live model (module docstring)."""
    import torch
    from bmnas import cell as K
    w_opt = architect.network_optimizer
    group = w_opt.param_groups[0]
    eta, mu, wd = group['lr'], group['momentum'], group['weight_decay']
    xt, yt = train
    xv, yv = valid
    loss = architect._loss(xt, yt)
    with K.weight_grads_only(True):
        g = torch.autograd.grad(loss, weights, allow_unused=True)
    with torch.no_grad():
        theta = _concat(weights)
        try:
            moment = _concat([w_opt.state[p]['momentum_buffer'] for p in weights]).mul_(mu)
        except KeyError:
            moment = torch.zeros_like(theta)
        dtheta = _concat(g) + wd * theta
        new = theta.sub(moment + dtheta, alpha=eta)
        off = 0
        for p, b in zip(weights, backups):
            b.copy_(p)
            n = p.numel()
            p.copy_(new[off:off + n].view_as(p))
            off += n
    del g, loss
    loss = architect._loss(xv, yv)
    both = torch.autograd.grad(loss, arch + weights, allow_unused=True)
    del loss
    dalpha, v = both[:len(arch)], both[len(arch):]
    with torch.no_grad():
        R = R0 / _concat(v).norm()
        for p, b, vv in zip(weights, backups, v):
            p.copy_(b)
            p.addcmul_(vv, R)
    drop_offset = K.DROP.offset
    gp = architect._arch_grads(arch, xt, yt)
    with torch.no_grad():
        for p, vv in zip(weights, v):
            p.addcmul_(vv, R, value=-2.0)
    K.DROP.offset = drop_offset
    gn = architect._arch_grads(arch, xt, yt)
    with torch.no_grad():
        for p, b in zip(weights, backups):
            p.copy_(b)
        for a, d, x, y in zip(arch, dalpha, gp, gn):
            ig = (x - y).div_(2 * R)
            a.grad = d.sub_(ig, alpha=eta)
    architect.optimizer.step()


def case(cname, batch):
    """One child: the two versions on one live model, alternating region by region.  Prints one JSON line."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    architect, weights, arch, train, valid = build(cname, batch)
    backups = [torch.empty_like(p) for p in weights]
    versions = {
        'kernels': lambda: architect.step(valid[0], valid[1], None, input_train=train[0], target_train=train[1]),
        'composed': lambda: composed_step(architect, weights, arch, train, valid, backups),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3            # us

    for step in versions.values():
        for _ in range(WARMUP):
            step()
    torch.cuda.synchronize()
    t = {k: [] for k in versions}
    for _ in range(REGIONS):
        for k, step in versions.items():
            t[k].append(timed(lambda: [step() for _ in range(PER)]) / PER)
    out = {'case': f'{cname} b{batch}', 'parameters': sum(p.numel() for p in weights), 'tensors': len(weights),
           'uploads_per_step': None}
    before = architect._unrolled.uploads
    for _ in range(4):
        versions['kernels']()
    out['uploads_per_step'] = (architect._unrolled.uploads - before) / 4
    for k, step in versions.items():
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[k] = {'regions_us': t[k], 'device_events': len(names), 'aten_events': sum('at::native' in n for n in names),
                  'unroll_events': sum('unroll_' in n for n in names)}
    finite = all(bool(torch.isfinite(a).all()) for a in arch)
    out['alpha_finite'] = finite
    print('RESULT ' + json.dumps(out), flush=True)


def run_case(cname, batch):
    """-> the child's result.  Any ending but exit status 0 — an exception, a time limit, a signal — stops the tool:
    nothing more is started on the GPU."""
    cmd = [sys.executable, os.path.abspath(__file__), '--case', f'{cname}:{batch}']
    try:
        p = subprocess.run(cmd, timeout=CASE_SECONDS, stdout=subprocess.PIPE, text=True)
        rc, text = p.returncode, p.stdout
    except subprocess.TimeoutExpired:
        rc, text = 124, ''
    if rc != 0:
        raise SystemExit(f'case {cname}:{batch} ended with {rc}: stopping')
    line = [ln for ln in text.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', help='CNAME:BATCH — one case (what the children run)')
    a = ap.parse_args()
    if a.case:
        cname, batch = a.case.split(':')
        return case(cname, int(batch))
    for cname, batch in CASES:
        r = run_case(cname, batch)
        print(f"{r['case']}: {r['parameters']} weight parameters in {r['tensors']} tensors; staging uploads per kernel-side "
              f"step {r['uploads_per_step']:.2f}; alpha finite: {r['alpha_finite']}")
        med = {}
        for v in ('kernels', 'composed'):
            ts = r[v]['regions_us']
            med[v] = statistics.median(ts)
            print(f"  {v:<9} median {med[v]:9.1f} us per step (spread {max(ts) - min(ts):.1f} over {len(ts)} regions of {PER} "
                  f"steps), {r[v]['device_events']} device events ({r[v]['aten_events']} aten, {r[v]['unroll_events']} "
                  f"unroll_*_k)", flush=True)
        print(f"  kernels against composed: {med['kernels'] - med['composed']:+.1f} us per step "
              f"({med['kernels'] / med['composed']:.3f} x), "
              f"{r['kernels']['device_events'] - r['composed']['device_events']:+d} device events", flush=True)


if __name__ == '__main__':
    main()
