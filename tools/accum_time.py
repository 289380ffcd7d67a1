#!/usr/bin/env python3
"""Gradient accumulation of the captured found-stage training step (bench.FoundNet: forward + criterion + backward + Adam
over every parameter), m micro-batches per optimizer step, in three forms on the same build:

    accum    bmnas.graph.GraphedTrainStep(accumulate=m): m passes, ONE bmnas_grad_combine_multi launch, ONE Adam launch —
             one replay per optimizer step
    singles  m replays of the one-step graph over the same micro-batches (m optimizer steps: what a user without
             accumulation runs; the same forward / backward work, m - 1 Adam launches more, no combine)
    eager    eager torch accumulation: m x ((criterion(model(x), y) * w).backward()) — autograd's AccumulateGrad adds —
             and one bmnas.optim.Adam step

    python tools/accum_time.py      # MM-IMDB 4 x b32 and NTU 8 x b8.  A case = one child process that builds the three
                                    # forms, which ALTERNATE region by region, five timed regions each (device events,
                                    # after warm-up): medians, spreads (max - min), device events per optimizer step and
                                    # how many of them are aten's, and each form against `accum`.
Then the combine launch alone: R launches over the model's own tensors captured in one graph, replayed and timed with
device events — us per launch and the rate of its 4 (m + 1) B per parameter of traffic.
No time is a pass / fail criterion.  Every case is a child process under its own time limit, and the tool stops at the
first one that does not exit with 0: nothing more is started on the GPU after it.  A step = train mode with dropout
on, bench.CONFIGS shapes, bench.synth_batch data.
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

CASES = [('mmimdb', 4, 32), ('ntu', 8, 8)]
CASE_SECONDS = 420
REGIONS, WARMUP = 5, 3
PER = {'accum': 100, 'singles': 100, 'eager': 10}       # optimizer steps (accum, eager) / groups of m steps (singles)
COMBINE_LAUNCHES = 50
VARIANTS = ('accum', 'singles', 'eager')


def case(cname, m, batch):
    """One child: the three forms, alternating region by region, then the combine launch alone.  One JSON line."""
    import torch
    import bench as B
    from bmnas import lib, nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam, GradAccumulator, accum_weights
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    micro = []
    for i in range(m):
        xs, y = B.synth_batch(c, batch, dev, i)
        micro.append(([x.detach() for x in xs], y))
    steps, n_param = {}, 0
    for name in VARIANTS:
        torch.manual_seed(2)
        model = B.FoundNet(c, cname).to(dev).train()
        crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        n_param = sum(p.numel() for p in model.parameters())
        if name == 'accum':
            g = GraphedTrainStep(model, crit, opt, *micro[0], accumulate=m)
            assert g.accumulator is not None and g.accum_plan is not None

            def step(g=g):
                for i, (xs, y) in enumerate(micro):
                    g.stage(i, xs, y)
                g.replay_staged()
        elif name == 'singles':
            g = GraphedTrainStep(model, crit, opt, *micro[0])

            def step(g=g):
                for xs, y in micro:
                    g(xs, y)
        else:
            ws = accum_weights([batch] * m, 'mean')

            def step(model=model, crit=crit, opt=opt, ws=ws):
                opt.zero_grad()
                for (xs, y), w in zip(micro, ws):
                    (crit(model(xs), y) * w).backward()
                opt.step()
        steps[name] = step

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
            t[k].append(timed(lambda: [step() for _ in range(PER[k])]) / PER[k])
    out = {'case': f'{cname} {m} x b{batch}', 'm': m, 'parameters': n_param}
    with profile(activities=[ProfilerActivity.CUDA]):       # (the first profile of a process misses replayed kernels)
        steps['singles']()
        torch.cuda.synchronize()
    for k in steps:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            steps[k]()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[k] = {'regions_us': t[k], 'device_events': len(names), 'aten_events': sum('at::native' in n for n in names),
                  'combine_events': sum('grad_combine_multi_k' in n for n in names)}

    # the combine launch alone, over this model's tensors: R launches in one graph (a replay is not host-bound)
    torch.manual_seed(2)
    model = B.FoundNet(c, cname).to(dev).train()
    acc = GradAccumulator(Adam(model.parameters(), lr=1e-3))
    parts = [[torch.randn_like(p) for p in acc.tensors] for _ in range(m)]
    for row in parts:
        acc.add(row, 1.0 / m)
    acc.combine()                                   # builds the eager plan and uploads its tables
    torch.cuda.synchronize()
    pl = acc._eager
    ws = [1.0 / m] * m
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for _ in range(COMBINE_LAUNCHES):
            lib.grad_combine_multi(pl['dev_tab'], pl['dev_chunks'], pl['n_chunks'], pl['dev_parts'], m, ws)
    for _ in range(WARMUP):
        graph.replay()
    torch.cuda.synchronize()
    out['combine_alone'] = {'regions_us': [timed(lambda: [graph.replay() for _ in range(20)]) / (20 * COMBINE_LAUNCHES)
                                           for _ in range(REGIONS)],
                            'workgroups': pl['n_chunks'], 'bytes': 4 * (m + 1) * n_param}
    print('RESULT ' + json.dumps(out), flush=True)


def run_case(cname, m, batch):
    """-> the child's result.  Any ending but exit status 0 — an exception, a time limit, a signal — stops the tool:
    nothing more is started on the GPU."""
    cmd = [sys.executable, os.path.abspath(__file__), '--case', f'{cname}:{m}:{batch}']
    try:
        p = subprocess.run(cmd, timeout=CASE_SECONDS, stdout=subprocess.PIPE, text=True)
        rc, text = p.returncode, p.stdout
    except subprocess.TimeoutExpired:
        rc, text = 124, ''
    if rc != 0:
        raise SystemExit(f'case {cname}:{m}:{batch} ended with {rc}: stopping')
    line = [ln for ln in text.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', help='CNAME:M:BATCH — one case (what the children run)')
    a = ap.parse_args()
    if a.case:
        cname, m, batch = a.case.split(':')
        return case(cname, int(m), int(batch))
    for cname, m, batch in CASES:
        r = run_case(cname, m, batch)
        print(f"{r['case']}: {r['parameters']} parameters, one optimizer step over {m} micro-batches")
        med = {}
        for v in VARIANTS:
            ts = r[v]['regions_us']
            med[v] = statistics.median(ts)
            line = (f"  {v:<8} median {med[v]:9.1f} us (spread {max(ts) - min(ts):.1f} over {len(ts)} regions), "
                    f"{r[v]['device_events']} device events ({r[v]['aten_events']} aten, "
                    f"{r[v]['combine_events']} grad_combine_multi_k)")
            if v != 'accum':
                line += f"; against accum {med[v] - med['accum']:+.1f} us ({med[v] / med['accum']:.2f} x)"
            print(line, flush=True)
        ca = r['combine_alone']
        ts = ca['regions_us']
        us = statistics.median(ts)
        print(f"  combine launch alone: median {us:.2f} us (spread {max(ts) - min(ts):.2f}), {ca['workgroups']} workgroups, "
              f"{ca['bytes'] / 1e6:.2f} MB = 4 (m + 1) B per parameter -> {ca['bytes'] / us / 1e3:.1f} GB/s", flush=True)


if __name__ == '__main__':
    main()
