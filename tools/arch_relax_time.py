#!/usr/bin/env python3
"""What the relaxation of the architecture weights (bmnas.nn.ArchRelaxation, csrc/relax.hip) costs in the captured search
step: the weight step and the architecture step of the search loop, each ONE hipGraph replay (bmnas.graph.GraphedTrainStep
over bench.HyperNet), in three forms that ALTERNATE region by region inside one process:

    none         no relaxation set: the step as it always was (the only form a checkout without the feature can run)
    tau          ArchRelaxation(tau=0.7): one launch in front of the cell prologue; in the architecture step one more
                 behind the arch-softmax backward (the weight step differentiates no architecture tensor: none)
    tau+gumbel   ... with Gumbel noise: the same launches, plus Philox and two logarithms per element

    python tools/arch_relax_time.py                      # MM-IMDB b128 and NTU b64
    python tools/arch_relax_time.py --baseline-only      # the `none` form alone: runs on a checkout without the feature

Per form and step: median and spread (max - min) of the timed regions, in us of device-event time per replay after warm-up,
and the difference to `none`.  What to compare it with: one launch floor per added launch (profiles/r05_launch_floor.txt:
1.92 us), i.e. + 1.92 us for the weight step and + 3.84 us for the architecture step.  To compare two checkouts (this one
and its parent commit) run the tool in both, alternating — `none` against the parent's `--baseline-only` is the cost of
the feature to a run that does not use it.  No time is a pass / fail criterion.  Every case is a child process under its
own time limit, and the tool stops at the first one that does not exit with 0: nothing more is started on the GPU after it.
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
CASE_SECONDS = 240
REGIONS, WARMUP, PER = 7, 300, 300
FORMS = {'none': None, 'tau': dict(tau=0.7, gumbel=False), 'tau+gumbel': dict(tau=0.7, gumbel=True)}


def case(cname, batch, baseline_only):
    import torch
    import bench as B
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    xs, y = B.synth_batch(c, batch, dev, 0)
    xv, yv = B.synth_batch(c, batch, dev, 1000)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3            # us

    steps = {}
    for form, opts in FORMS.items():
        if baseline_only and opts is not None:
            continue
        torch.manual_seed(2)
        model = B.HyperNet(c, 'F', cname).to(dev)
        model.train()
        if opts is not None:
            model.fusion_net.set_relaxation(bnn.ArchRelaxation(seed=5, **opts))
        crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
        w_opt = Adam(list(model.parameters()), lr=1e-3, weight_decay=1e-4)
        a_opt = Adam(model.arch_parameters(), lr=3e-4, betas=(0.5, 0.999), weight_decay=1e-3)
        gw = GraphedTrainStep(model, crit, w_opt, xs, y)
        ga = GraphedTrainStep(model, crit, a_opt, xv, yv)
        steps[form] = {'w_step': (lambda gw=gw: gw(xs, y)), 'a_step': (lambda ga=ga: ga(xv, yv))}
    for form in steps:
        for fn in steps[form].values():
            for _ in range(WARMUP):
                fn()
    torch.cuda.synchronize()
    t = {form: {k: [] for k in fns} for form, fns in steps.items()}
    for _ in range(REGIONS):
        for form, fns in steps.items():
            for k, fn in fns.items():
                t[form][k].append(timed(lambda: [fn() for _ in range(PER)]) / PER)
    print('RESULT ' + json.dumps({'case': f'{cname} b{batch}', 'regions_us': t}), flush=True)


def run_case(cname, batch, baseline_only):
    """-> the child's result.  Any ending but exit status 0 — an exception, a time limit, a signal — stops the tool:
    nothing more is started on the GPU."""
    cmd = [sys.executable, os.path.abspath(__file__), '--case', f'{cname}:{batch}']
    if baseline_only:
        cmd.append('--baseline-only')
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
    ap.add_argument('--baseline-only', action='store_true', help='the `none` form alone (a checkout without the feature)')
    a = ap.parse_args()
    if a.case:
        cname, batch = a.case.split(':')
        return case(cname, int(batch), a.baseline_only)
    for cname, batch in CASES:
        r = run_case(cname, batch, a.baseline_only)
        print(r['case'])
        t = r['regions_us']
        for form, by_step in t.items():
            for k, ts in by_step.items():
                line = (f'  {form:<11} {k:<7} median {statistics.median(ts):8.2f} us per replay '
                        f'(spread {max(ts) - min(ts):.2f} over {len(ts)} regions)')
                if form != 'none':
                    line += f"; against none {statistics.median(ts) - statistics.median(t['none'][k]):+.2f} us"
                print(line, flush=True)


if __name__ == '__main__':
    main()
