#!/usr/bin/env python3
"""The captured search step (forward + criterion + backward + optimizer as one hipGraph replay,
bmnas.graph.GraphedTrainStep) with the one-launch SGD step (bmnas_sgd_multi) beside the Adam step of the same run:

    adam       bmnas.optim.Adam(lr, weight_decay)                          (bmnas_adam_multi: 28 B per parameter)
    sgd        bmnas.optim.SGD(lr, momentum=0.9, weight_decay)             (bmnas_sgd_multi: 20 B per parameter)
    sgd_clip   SGD(..., max_grad_norm=5)                                   (+ the norm launch)

and, for reference, the optimizer step ALONE, eagerly, over the same model's gradients: torch.optim.SGD(momentum=0.9)
(torch's foreach launches per parameter group) and bmnas.optim.SGD (one H2D copy + one launch).

    python tools/sgd_time.py        # MM-IMDB b128 and NTU b64.  A case = one child process that builds the three captured
                                    # steps, which ALTERNATE region by region, five timed regions each (device events,
                                    # after warm-up): medians, spreads (max - min), device events per step, and each
                                    # variant against `adam` of the same process
No time is a pass / fail criterion.  The expectation to compare against: the SGD launch moves 20 B per parameter where
Adam's moves 28, in a launch that is a small part of the step; clipping adds its norm launch.  Every case is a child
process under its own time limit, and the tool stops at the first one that does not exit with 0: nothing more is started
on the GPU after it.  A step = train mode with dropout on, bench.CONFIGS shapes, bench.synth_batch data.
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
REGIONS, WARMUP, PER = 5, 3, 200
MAX_NORM = 5.0
VARIANTS = ('adam', 'sgd', 'sgd_clip')
EAGER = ('torch_sgd_step', 'bmnas_sgd_step')


def make_optimizer(name, params):
    from bmnas.optim import SGD, Adam
    if name == 'adam':
        return Adam(params, lr=1e-3, weight_decay=1e-4)
    return SGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4, max_grad_norm=MAX_NORM if name == 'sgd_clip' else None)


def case(cname, batch):
    """One child: the three captured steps, alternating region by region, then the two eager optimizer steps alone.
    Prints one JSON line."""
    import torch
    import bench as B
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import SGD
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    steps, n_params = {}, 0
    for name in VARIANTS:
        torch.manual_seed(2)
        model = B.HyperNet(c, 'F', cname).to(dev).train()
        crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
        xs, y = B.synth_batch(c, batch, dev, 0)
        xs = [x.detach() for x in xs]
        g = GraphedTrainStep(model, crit, make_optimizer(name, model.parameters()), xs, y)
        steps[name] = (lambda g=g, xs=xs, y=y: g(xs, y))
        n_params = sum(p.numel() for p in model.parameters())

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3            # us

    for k in steps:
        for _ in range(WARMUP):
            steps[k]()
    torch.cuda.synchronize()
    t = {k: [] for k in steps}
    for _ in range(REGIONS):
        for k, step in steps.items():
            t[k].append(timed(lambda: [step() for _ in range(PER)]) / PER)
    out = {'case': f'{cname} b{batch}', 'parameters': n_params}
    for k in steps:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            steps[k]()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[k] = {'regions_us': t[k], 'device_events': len(names), 'aten_events': sum('at::native' in n for n in names),
                  'sgd_events': sum('sgd_multi_k' in n for n in names)}
    # the optimizer step alone, eagerly, over constant gradients of the model's own shapes
    torch.manual_seed(2)
    model = B.HyperNet(c, 'F', cname).to(dev).train()
    params = [p for p in model.parameters()]
    for p in params:
        p.grad = torch.randn_like(p) * 1e-3
    eager = {'torch_sgd_step': torch.optim.SGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4),
             'bmnas_sgd_step': SGD(params, lr=1e-3, momentum=0.9, weight_decay=1e-4)}
    for k, opt in eager.items():
        for _ in range(WARMUP):
            opt.step()
    torch.cuda.synchronize()
    te = {k: [] for k in eager}
    for _ in range(REGIONS):
        for k, opt in eager.items():
            te[k].append(timed(lambda: [opt.step() for _ in range(PER)]) / PER)
    for k, opt in eager.items():
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[k] = {'regions_us': te[k], 'device_events': len(names)}
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
        print(f"{r['case']}: {r['parameters']} parameters (SGD with momentum: {20 * r['parameters'] / 1e6:.2f} MB of "
              f"traffic per step, Adam: {28 * r['parameters'] / 1e6:.2f} MB)")
        med = {}
        for v in VARIANTS:
            ts = r[v]['regions_us']
            med[v] = statistics.median(ts)
            line = (f"  {v:<15} median {med[v]:8.1f} us (spread {max(ts) - min(ts):.1f} over {len(ts)} regions), "
                    f"{r[v]['device_events']} device events ({r[v]['aten_events']} aten, {r[v]['sgd_events']} sgd_multi_k)")
            if v != 'adam':
                line += (f"; against adam {med[v] - med['adam']:+.2f} us, "
                         f"{r[v]['device_events'] - r['adam']['device_events']:+d} device events")
            print(line, flush=True)
        for v in EAGER:
            ts = r[v]['regions_us']
            print(f"  {v:<15} median {statistics.median(ts):8.1f} us per eager optimizer step alone (spread "
                  f"{max(ts) - min(ts):.1f}), {r[v]['device_events']} device events", flush=True)


if __name__ == '__main__':
    main()
