#!/usr/bin/env python3
"""The captured search step (forward + criterion + backward + Adam as one hipGraph replay, bmnas.graph.GraphedTrainStep)
with the Adam variants of the one-launch optimizer step (bmnas_adam_multi_ex) beside the plain step of the same run:

    plain              bmnas.optim.Adam                                  (bmnas_adam_multi: the code path as it always was)
    amsgrad            Adam(amsgrad=True)                                (+ 8 B of traffic per parameter, no launch)
    adamw              bmnas.optim.AdamW                                 (one multiply per parameter, no traffic, no launch)
    adamw_amsgrad_clip AdamW(amsgrad=True, max_grad_norm=5)              (+ 8 B per parameter, + the norm launch)

    python tools/adam_variants_time.py        # MM-IMDB b128 and NTU b64.  A case = one child process that builds the four
                                              # captured steps, which ALTERNATE region by region, five timed regions each
                                              # (device events, after warm-up): medians, spreads (max - min), device events
                                              # per step, and each variant against `plain` of the same process
No time is a pass / fail criterion.  The expectation to compare against: AMSGrad adds one float4 load and one float4
store per lane (28 -> 36 B per parameter) to a launch that is a small part of the step, and no variant adds a launch
but clipping (its norm launch).  Every case is a child process under its own time limit, and the tool stops at the first
one that does not exit with 0: nothing more is started on the GPU after it.  A step = train mode with dropout on,
bench.CONFIGS shapes, bench.synth_batch data.
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
VARIANTS = ('plain', 'amsgrad', 'adamw', 'adamw_amsgrad_clip')


def make_optimizer(name, params):
    from bmnas.optim import Adam, AdamW
    if name == 'plain':
        return Adam(params, lr=1e-3, weight_decay=1e-4)
    if name == 'amsgrad':
        return Adam(params, lr=1e-3, weight_decay=1e-4, amsgrad=True)
    if name == 'adamw':
        return AdamW(params, lr=1e-3, weight_decay=1e-4)
    return AdamW(params, lr=1e-3, weight_decay=1e-4, amsgrad=True, max_grad_norm=MAX_NORM)


def case(cname, batch):
    """One child: the four captured steps, alternating region by region.  Prints one JSON line."""
    import torch
    import bench as B
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
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
                  'adam_ex_events': sum('adam_multi_ex_k' in n for n in names)}
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
        print(f"{r['case']}: {r['parameters']} parameters (AMSGrad: +{8 * r['parameters'] / 1e6:.2f} MB of traffic per step)")
        med = {}
        for v in VARIANTS:
            ts = r[v]['regions_us']
            med[v] = statistics.median(ts)
            spread = max(ts) - min(ts)
            line = (f"  {v:<19} median {med[v]:8.1f} us (spread {spread:.1f} over {len(ts)} regions), "
                    f"{r[v]['device_events']} device events ({r[v]['aten_events']} aten, {r[v]['adam_ex_events']} "
                    f"adam_multi_ex_k)")
            if v != 'plain':
                line += (f"; against plain {med[v] - med['plain']:+.2f} us, "
                         f"{r[v]['device_events'] - r['plain']['device_events']:+d} device events")
            print(line, flush=True)


if __name__ == '__main__':
    main()
