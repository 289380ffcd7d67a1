#!/usr/bin/env python3
"""The captured search step (forward + criterion + backward + Adam as one hipGraph replay, bmnas.graph.GraphedTrainStep)
with gradient-norm clipping inside the optimizer step (bmnas.optim.Adam(max_grad_norm=...)) against the same step
without it, and against what clipping costs without that argument: torch.nn.utils.clip_grad_norm_ between backward()
and step(), which only an eager step can hold.

    python tools/grad_clip_time.py                        # MM-IMDB b128 and NTU b64.  A leg = one child process for one
                                                          # case on one tree: it builds the variants the tree has —
                                                          # `unclipped` and `clipped` captured steps, `eager_torch_clip`
                                                          # (zero_grad, backward, torch's clip_grad_norm_, step) — which
                                                          # ALTERNATE region by region, five timed regions each (device
                                                          # events, after warm-up).  Two legs per case; regions pooled:
                                                          # medians, spreads (max - min), device events per step
    python tools/grad_clip_time.py --tree PARENT_CHECKOUT # additionally the same user code imported from another checkout
                                                          # (the parent commit: no max_grad_norm, so no `clipped` variant).
                                                          # The legs of the two trees ALTERNATE; then the comparisons:
                                                          #   (a) clipped vs unclipped on this tree (same processes)
                                                          #   (b) unclipped on this tree vs unclipped on the other tree
                                                          #   (c) clipped on this tree vs eager_torch_clip on the other
                                                          # (b) and (c) compare different processes, interleaved in time
Every leg is a child process under its own time limit, and the tool stops at the first leg that does not exit with 0:
nothing more is started on the GPU after it.  A step = train mode with dropout on, bench.CONFIGS shapes,
bench.synth_batch data; max_grad_norm = 5 (DARTS' --grad_clip).
"""
import argparse
import inspect
import json
import os
import statistics
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = HERE
if '--import-from' in sys.argv:              # (children) the checkout of the project to import
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--import-from') + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))

CASES = [('mmimdb', 128), ('ntu', 64)]
LEG_SECONDS = 300
REGIONS, WARMUP = 5, 3
PER = {'unclipped': 200, 'clipped': 200, 'eager_torch_clip': 30}       # steps per timed region
ROUNDS = 2                                    # legs per case and tree
MAX_NORM = 5.0
VARIANTS = ('unclipped', 'clipped', 'eager_torch_clip')


def leg(cname, batch):
    """One child: the variants this checkout has, alternating region by region.  Prints one JSON line."""
    import torch
    import bench as B
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    has_clip = 'max_grad_norm' in inspect.signature(Adam.__init__).parameters
    steps = {}
    for name in VARIANTS:
        if name == 'clipped' and not has_clip:
            continue
        torch.manual_seed(2)
        model = B.HyperNet(c, 'F', cname).to(dev).train()
        crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
        xs, y = B.synth_batch(c, batch, dev, 0)
        xs = [x.detach() for x in xs]
        kw = {'max_grad_norm': MAX_NORM} if name == 'clipped' else {}
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4, **kw)
        if name == 'eager_torch_clip':
            params = list(model.parameters())

            def eager(model=model, crit=crit, opt=opt, xs=xs, y=y, params=params):
                opt.zero_grad()
                crit(model(xs), y).backward()
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                opt.step()
            steps[name] = eager
        else:
            g = GraphedTrainStep(model, crit, opt, xs, y)
            steps[name] = (lambda g=g, xs=xs, y=y: g(xs, y))
    # the captured steps were built before the first eager backward (GraphedTrainStep refuses to capture next to a live
    # autograd graph); from here on the variants alternate

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
    out = {'case': f'{cname} b{batch}', 'tree': ROOT}
    for k in steps:
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            steps[k]()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[k] = {'regions_us': t[k], 'device_events': len(names), 'aten_events': sum('at::native' in n for n in names)}
    print('RESULT ' + json.dumps(out), flush=True)


def run_leg(cname, batch, tree):
    """-> the child's result.  Any ending but exit status 0 — an exception, a time limit, a signal — stops the tool:
    nothing more is started on the GPU."""
    cmd = [sys.executable, os.path.abspath(__file__), '--leg', f'{cname}:{batch}', '--import-from', tree]
    try:
        p = subprocess.run(cmd, timeout=LEG_SECONDS, stdout=subprocess.PIPE, text=True)
        rc, text = p.returncode, p.stdout
    except subprocess.TimeoutExpired:
        rc, text = 124, ''
    if rc != 0:
        raise SystemExit(f'leg {cname}:{batch} on {tree} ended with {rc}: stopping')
    line = [ln for ln in text.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def pooled(legs, name):
    """The legs' figures for one variant with their regions pooled; None: the tree has no such variant."""
    rs = [leg_.get(name) for leg_ in legs]
    if any(r is None for r in rs):
        return None
    t = [v for r in rs for v in r['regions_us']]
    return {'median_us': statistics.median(t), 'spread_us': max(t) - min(t), 'regions': len(t),
            'device_events': rs[0]['device_events'], 'aten_events': rs[0]['aten_events']}


def fmt(r):
    if r is None:
        return 'not available on this tree'
    return (f"median {r['median_us']:.1f} us (spread {r['spread_us']:.1f} over {r['regions']} regions, "
            f"{r['device_events']} device events, {r['aten_events']} aten)")


def within(a, b):
    """medians differ by no more than the larger spread"""
    return abs(a['median_us'] - b['median_us']) <= max(a['spread_us'], b['spread_us'])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tree', help='another checkout of the project (the parent commit) to run the same user code on')
    ap.add_argument('--leg', help='CNAME:BATCH — one leg (what the children run)')
    ap.add_argument('--import-from', help='(children) the checkout to import the project from')
    a = ap.parse_args()
    if a.leg:
        cname, batch = a.leg.split(':')
        return leg(cname, int(batch))
    for cname, batch in CASES:
        trees = [HERE] + ([os.path.abspath(a.tree)] if a.tree else [])
        legs = {t: [] for t in trees}
        for _ in range(ROUNDS):                      # the trees' legs alternate
            for t in trees:
                legs[t].append(run_leg(cname, batch, t))
        here = {v: pooled(legs[HERE], v) for v in VARIANTS}
        print(f'{cname} b{batch} this tree: ' + ' | '.join(f'{v} {fmt(here[v])}' for v in VARIANTS))
        cl, un = here['clipped'], here['unclipped']
        print(f"  (a) clipped vs unclipped, this tree: {cl['median_us']:.1f} vs {un['median_us']:.1f} us "
              f"({cl['median_us'] - un['median_us']:+.2f} us; within the larger spread: {within(cl, un)}), "
              f"{cl['device_events']} vs {un['device_events']} device events", flush=True)
        if a.tree:
            other = {v: pooled(legs[trees[1]], v) for v in VARIANTS}
            print(f'{cname} b{batch} other tree {trees[1]}: ' + ' | '.join(f'{v} {fmt(other[v])}' for v in VARIANTS))
            uo, eo = other['unclipped'], other['eager_torch_clip']
            print(f"  (b) unclipped, this tree vs other tree: {un['median_us']:.1f} vs {uo['median_us']:.1f} us, "
                  f"{un['device_events']} vs {uo['device_events']} device events; not slower (within the larger spread or "
                  f"below): {un['median_us'] <= uo['median_us'] or within(un, uo)}")
            print(f"  (c) clipped captured step, this tree, vs eager step with torch's clip_grad_norm_, other tree: "
                  f"{cl['median_us']:.1f} vs {eo['median_us']:.1f} us, {cl['device_events']} vs {eo['device_events']} "
                  f"device events ({eo['aten_events']} of them aten)", flush=True)


if __name__ == '__main__':
    main()
