#!/usr/bin/env python3
"""The captured found-stage training step (forward + criterion + backward + Adam as one hipGraph replay,
bmnas.graph.GraphedTrainStep) with weight averaging in three forms:

    plain       no averaging
    ema_replay  bmnas.optim.AveragedModel(decay=0.999, use_buffers=True) updated INSIDE the replay (one bmnas_avg_multi
                launch behind the Adam launch; its 32-byte row rides in the batch-copy launch's blob)
    ema_torch   torch.optim.swa_utils.AveragedModel(get_ema_multi_avg_fn(0.999), use_buffers=True).update_parameters()
                called after each replay of the plain step, on the same build

    python tools/avg_time.py        # MM-IMDB b128 and NTU b64.  A case = one child process that builds the captured
                                    # steps, which ALTERNATE region by region, five timed regions each (device events,
                                    # after warm-up): medians, spreads (max - min), device events per step (replay + what
                                    # follows it), how many of them are aten's, and each variant against `plain`
No time is a pass / fail criterion.  The expectation to confirm or refute: `ema_replay` is one device event more than
`plain` and none of aten.  Every case is a child process under its own time limit, and the tool stops at the first one
that does not exit with 0: nothing more is started on the GPU after it.  A step = train mode with dropout on,
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
DECAY = 0.999
VARIANTS = ('plain', 'ema_replay', 'ema_torch')


def case(cname, batch):
    """One child: the three forms, alternating region by region.  Prints one JSON line."""
    import torch
    import bench as B
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam, AveragedModel
    from torch.optim import swa_utils
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    steps, n_avg = {}, 0
    for name in VARIANTS:
        torch.manual_seed(2)
        model = B.HyperNet(c, 'F', cname).to(dev).train()
        crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
        xs, y = B.synth_batch(c, batch, dev, 0)
        xs = [x.detach() for x in xs]
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        if name == 'ema_replay':
            avg = AveragedModel(model, decay=DECAY, use_buffers=True)
            g = GraphedTrainStep(model, crit, opt, xs, y, averaged=avg)
            assert g.averaged is avg
            n_avg = sum(t.numel() for t in list(model.parameters()) + list(model.buffers()) if t.is_floating_point())
            steps[name] = (lambda g=g, xs=xs, y=y: g(xs, y))
        elif name == 'ema_torch':
            avg = swa_utils.AveragedModel(model, multi_avg_fn=swa_utils.get_ema_multi_avg_fn(DECAY), use_buffers=True)
            g = GraphedTrainStep(model, crit, opt, xs, y)
            steps[name] = (lambda g=g, xs=xs, y=y, avg=avg, model=model: (g(xs, y), avg.update_parameters(model)))
        else:
            g = GraphedTrainStep(model, crit, opt, xs, y)
            steps[name] = (lambda g=g, xs=xs, y=y: g(xs, y))

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
    out = {'case': f'{cname} b{batch}', 'averaged_elements': n_avg}
    for k in steps:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            steps[k]()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[k] = {'regions_us': t[k], 'device_events': len(names), 'aten_events': sum('at::native' in n for n in names),
                  'avg_events': sum('avg_multi_k' in n for n in names)}
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
        print(f"{r['case']}: {r['averaged_elements']} averaged fp32 elements ({12 * r['averaged_elements'] / 1e6:.2f} MB of "
              f"traffic per update)")
        med = {}
        for v in VARIANTS:
            ts = r[v]['regions_us']
            med[v] = statistics.median(ts)
            line = (f"  {v:<11} median {med[v]:8.1f} us (spread {max(ts) - min(ts):.1f} over {len(ts)} regions), "
                    f"{r[v]['device_events']} device events ({r[v]['aten_events']} aten, {r[v]['avg_events']} avg_multi_k)")
            if v != 'plain':
                line += (f"; against plain {med[v] - med['plain']:+.2f} us, "
                         f"{r[v]['device_events'] - r['plain']['device_events']:+d} device events")
            print(line, flush=True)


if __name__ == '__main__':
    main()
