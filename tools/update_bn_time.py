#!/usr/bin/env python3
"""Time per batch of a bmnas.optim.update_bn pass — the cumulative BatchNorm-statistics pass that ends the SWA recipe
(BatchNorm momentum None: factor 1 / num_batches_tracked from the device counter) — over a found-stage network in two
forms:

    graphed   update_bn(loader, model, unpack=..., criterion=...): the forwards are replays of one private
              bmnas.graph.GraphedForward captured under momentum None
    eager     the same call with graph=False: one gradient-free eager forward per batch

    python tools/update_bn_time.py   # MM-IMDB b128 and NTU b64.  A case = one child process; the two forms ALTERNATE
                                     # region by region, five timed regions each (device events around a whole pass of
                                     # BATCHES equal batches, after a warm-up pass): medians and spreads (max - min) per
                                     # batch.  A graphed pass includes its capture (once per pass, as in the loop).
No time is a pass / fail criterion.  Every case is a child process under its own time limit, and the tool stops at the
first one that does not exit with 0: nothing more is started on the GPU after it.  Shapes: bench.CONFIGS, data:
bench.synth_batch; the model is in eval mode before the pass (update_bn puts it in training mode and back).
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
REGIONS, BATCHES = 5, 100
VARIANTS = ('graphed', 'eager')


def case(cname, batch):
    """One child: the two forms, alternating region by region.  Prints one JSON line."""
    import torch
    import bench as B
    from bmnas import nn as bnn
    from bmnas.optim import update_bn
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    torch.manual_seed(2)
    model = B.HyperNet(c, 'F', cname).to(dev).eval()
    crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
    data = []
    for i in range(4):
        xs, y = B.synth_batch(c, batch, dev, i)
        data.append(([x.detach() for x in xs], y))
    loader = [data[i % len(data)] for i in range(BATCHES)]
    unpack = lambda b, device: b

    def one_pass(graph):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        report = update_bn(loader, model, dev, unpack=unpack, criterion=crit, graph=graph)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3 / BATCHES, report          # us per batch

    for graph in (True, False):
        one_pass(graph)
    t, reports = {k: [] for k in VARIANTS}, {}
    for _ in range(REGIONS):
        for k in VARIANTS:
            us, reports[k] = one_pass(k == 'graphed')
            t[k].append(us)
    counters = sorted({int(m.num_batches_tracked) for m in model.modules()
                       if isinstance(m, torch.nn.modules.batchnorm._BatchNorm)})
    print('RESULT ' + json.dumps({'case': f'{cname} b{batch}', 'counters': counters,
                                  **{k: {'regions_us': t[k], 'report': reports[k]} for k in VARIANTS}}), flush=True)


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
        print(f"{r['case']}: {BATCHES} batches per pass, BatchNorm counters after a pass {r['counters']}")
        med = {}
        for v in VARIANTS:
            ts = r[v]['regions_us']
            med[v] = statistics.median(ts)
            print(f"  {v:<8} median {med[v]:8.1f} us per batch (spread {max(ts) - min(ts):.1f} over {len(ts)} passes), "
                  f"{r[v]['report']}", flush=True)
        print(f"  eager / graphed: {med['eager'] / med['graphed']:.2f}", flush=True)


if __name__ == '__main__':
    main()
