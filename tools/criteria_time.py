#!/usr/bin/env python3
"""The captured search step (forward + criterion + backward + Adam as one hipGraph replay, bmnas.graph.GraphedTrainStep)
with a class-weighted / label-smoothed criterion against the same step with the bare criterion.

    python tools/criteria_time.py                        # MM-IMDB b128 with pos_weight, NTU b64 with class weights and
                                                         # label_smoothing=0.1.  A leg = one child process for one case on
                                                         # one tree: it builds the unweighted and the weighted step, which
                                                         # ALTERNATE region by region, five timed regions each (device
                                                         # events, after warm-up).  Two legs per case; their regions are
                                                         # pooled: medians, spreads (max - min), device events per replay
    python tools/criteria_time.py --tree PARENT_CHECKOUT # additionally the same user code imported from another checkout
                                                         # (the parent commit, where a weighted criterion runs torch's
                                                         # kernels inside the step).  The legs of the two trees ALTERNATE
                                                         # (this, other, this, other); then the comparisons:
                                                         #   (a) weighted vs unweighted on this tree (same processes)
                                                         #   (b) weighted on this tree vs weighted on the other tree
                                                         #   (c) unweighted on this tree vs unweighted on the other tree
                                                         # (b) and (c) compare different processes, interleaved in time
Every leg is a child process under its own time limit, and the tool stops at the first leg that does not exit with 0:
nothing more is started on the GPU after it.  One refusal is expected and is reported by the child itself, not through
its exit status: GraphedTrainStep's dress rehearsal refusing a step whose criterion synchronises with the host (torch's
weighted cross entropy on the other tree) — that variant is "not measured", the other one of the leg still is.
A step = train mode with dropout on, bench.CONFIGS shapes, bench.synth_batch data.
"""
import argparse
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
REGIONS, WARMUP, PER = 5, 3, 200
ROUNDS = 2                                    # legs per case and tree


def criterion(cname, nout, weighted, device):
    import torch
    from bmnas import nn as bnn
    g = torch.Generator().manual_seed(7)
    vec = lambda: (0.25 + 2.0 * torch.rand(nout, generator=g)).to(device)
    if cname == 'mmimdb':
        return bnn.BCEWithLogitsLoss(pos_weight=vec()) if weighted else bnn.BCEWithLogitsLoss()
    return bnn.CrossEntropyLoss(weight=vec(), label_smoothing=0.1) if weighted else bnn.CrossEntropyLoss()


def leg(cname, batch):
    """One child: the unweighted and the weighted captured step of this checkout, alternating region by region.
    Prints one JSON line."""
    import warnings

    import torch
    import bench as B
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    steps, off_path, refused = {}, {}, {}
    for weighted in (False, True):
        torch.manual_seed(2)
        model = B.HyperNet(c, 'F', cname).to(dev).train()
        crit = criterion(cname, c['nout'], weighted, dev)
        xs, y = B.synth_batch(c, batch, dev, 0)
        xs = [x.detach() for x in xs]
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter('always')
            try:
                g = GraphedTrainStep(model, crit, opt, xs, y)
            except RuntimeError as e:
                # the ONE expected refusal (raised before anything is captured); every other error ends the child
                if 'called a synchronizing' not in str(e):
                    raise
                refused[weighted] = str(e).splitlines()[0]
                continue
        off_path[weighted] = any('stock torch ops' in str(w.message) for w in seen)
        steps[weighted] = (lambda g=g, xs=xs, y=y: g(xs, y))

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
    out = {'case': f'{cname} b{batch}', 'tree': ROOT}
    for k in (True, False):
        name = 'weighted' if k else 'unweighted'
        if k in refused:
            out[name] = {'refused': refused[k]}
            continue
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            steps[k]()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        out[name] = {'regions_us': t[k], 'device_events': len(names),
                     'aten_events': sum('at::native' in n for n in names), 'criterion_on_torch': off_path[k]}
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
    """The legs' figures for one variant with their regions pooled, or the refusal."""
    rs = [leg_[name] for leg_ in legs]
    if any('refused' in r for r in rs):
        return {'refused': next(r['refused'] for r in rs if 'refused' in r)}
    t = [v for r in rs for v in r['regions_us']]
    return {'median_us': statistics.median(t), 'spread_us': max(t) - min(t), 'regions': len(t),
            'device_events': rs[0]['device_events'], 'aten_events': rs[0]['aten_events'],
            'criterion_on_torch': rs[0]['criterion_on_torch']}


def fmt(r):
    if 'refused' in r:
        return f"not measured, the step cannot be captured: {r['refused']}"
    return (f"median {r['median_us']:.1f} us (spread {r['spread_us']:.1f} over {r['regions']} regions, "
            f"{r['device_events']} device events, {r['aten_events']} aten"
            + (', criterion on torch' if r['criterion_on_torch'] else '') + ')')


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
        w, u = pooled(legs[HERE], 'weighted'), pooled(legs[HERE], 'unweighted')
        print(f'{cname} b{batch} this tree: weighted {fmt(w)} | unweighted {fmt(u)}')
        print(f'  (a) weighted vs unweighted, this tree: medians within the larger spread: {within(w, u)}; device events '
              f"equal: {w['device_events'] == u['device_events']}", flush=True)
        if a.tree:
            wo, uo = pooled(legs[trees[1]], 'weighted'), pooled(legs[trees[1]], 'unweighted')
            print(f'{cname} b{batch} other tree {trees[1]}: weighted {fmt(wo)} | unweighted {fmt(uo)}')
            if 'refused' in wo:
                print(f"  (b) weighted, this tree vs other tree: {w['median_us']:.1f} us, {w['device_events']} device events "
                      'vs no captured step')
            else:
                print(f"  (b) weighted, this tree vs other tree: {w['median_us']:.1f} vs {wo['median_us']:.1f} us, "
                      f"{w['device_events']} vs {wo['device_events']} device events")
            print(f"  (c) unweighted, this tree vs other tree: {u['median_us']:.1f} vs {uo['median_us']:.1f} us; not slower "
                  f"(within the larger spread or below): {u['median_us'] <= uo['median_us'] or within(u, uo)}", flush=True)


if __name__ == '__main__':
    main()
