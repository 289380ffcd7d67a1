#!/usr/bin/env python3
"""One search step with PRIMITIVES = ['none', 'fc_relu', 'fc_mish', 'skip']: the grouped FC-edge kernels
(csrc/fcedge.hip, bmnas.functions.FcEdgeSumFn) against the composed fallback (FusionMixedOp op by op through aten).

    python tools/fc_edges_time.py                      # MM-IMDB b128, NTU b64, NTU b8: both paths ALTERNATING in this
                                                       # call, five timed regions each (device events, after warm-up):
                                                       # medians, spreads (max - min), device launches per step
    rocprofv3 --kernel-trace --stats -d DIR -o fc -- python tools/fc_edges_time.py --trace mmimdb:128
    python tools/fc_edges_time.py --stats DIR/.../fc_results.db --trace mmimdb:128      # (or ..._kernel_stats.csv)
                                                       # achieved FLOP/s of the two GEMM launches from that trace
    python tools/fc_edges_time.py --composed-only --tree PARENT_CHECKOUT
                                                       # the composed path alone, imported from another checkout (the
                                                       # parent commit, whose only path it is): has the fallback got slower?

    python tools/fc_edges_time.py --stage found        # the FOUND stage: a found network whose four cell-level edges are
                                                       # fc_relu / fc_mish (both kinds, two edges reading one input;
                                                       # bmnas.functions.FoundFcEdgesFn) at MM-IMDB b128 and NTU b64, one
                                                       # eager and one captured training step (forward + criterion +
                                                       # backward + Adam); native and composed alternate, five regions
                                                       # each; every leg is a child process under its own time limit
    python tools/fc_edges_time.py --stage found --composed-only --tree PARENT_CHECKOUT

A step = forward + criterion + backward in train mode with dropout on, bench.CONFIGS shapes, bench.synth_batch data.
"""
import argparse
import csv
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if '--tree' in sys.argv:                   # another checkout of the project (the parent commit) to import from
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))

import torch

PRIMS = ['none', 'fc_relu', 'fc_mish', 'skip']
CASES = [('mmimdb', 128), ('ntu', 64), ('ntu', 8)]
PEAK_FP32_MFMA = 157.3e12


def gemm_flops(c, batch):
    """(forward, backward) FLOP of the GEMM launches of one step: cell-level sums carry 2 FC primitives per edge, the
    inner sums 1 (their two-column rows reach 'none' + 'fc_relu' only); the backward launch does the data- and the
    weight-gradient product."""
    per = 2 * c['C'] * c['C'] * batch * c['L']
    fwd = 0
    for i in range(c['S']):
        fwd += (c['N'] + i) * 2 * per
        fwd += sum(2 + t for t in range(c['ns'])) * per
    return fwd, 2 * fwd


def build(cname, batch):
    import bench as B
    import models.search.darts.genotypes as gt
    from bmnas import nn as bnn
    c = B.CONFIGS[cname]
    saved = list(gt.PRIMITIVES)
    gt.PRIMITIVES[:] = PRIMS
    try:
        torch.manual_seed(2)
        model = B.HyperNet(c, 'F', cname).to('cuda:0').train()
    finally:
        gt.PRIMITIVES[:] = saved
    crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
    xs, y = B.synth_batch(c, batch, torch.device('cuda:0'), 0)
    params = [p for p in model.parameters()] + list(model.arch_parameters()) + xs

    def step():
        for p in params:
            p.grad = None
        loss = crit(model(xs), y)
        loss.backward()
        return loss
    return c, step


def set_native(on):
    from models.search.darts import operations as ops_mod
    if hasattr(ops_mod, 'FC_EDGES_NATIVE'):
        ops_mod.FC_EDGES_NATIVE = bool(on)
    elif on:
        raise RuntimeError('this checkout has no native FC-edge path')


def measure_composed(cname, batch, regions=5, warmup=3):
    c, step = build(cname, batch)
    set_native(False)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t = [timed(step) for _ in range(regions)]
    print(f'{cname} b{batch}: composed alone, tree {ROOT}: median {statistics.median(t):.1f} us (spread '
          f'{max(t) - min(t):.1f}, {launches(step)} launches)', flush=True)


def launches(step):
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def timed(step):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3            # us


def measure(cname, batch, regions=5, warmup=3):
    c, step = build(cname, batch)
    for on in (True, False):
        set_native(on)
        for _ in range(warmup):
            step()
    torch.cuda.synchronize()
    t = {True: [], False: []}
    for _ in range(regions):
        for on in (True, False):
            set_native(on)
            t[on].append(timed(step))
    n = {}
    for on in (True, False):
        set_native(on)
        n[on] = launches(step)
    set_native(True)
    med = {k: statistics.median(v) for k, v in t.items()}
    spr = {k: max(v) - min(v) for k, v in t.items()}
    ok = med[True] < med[False] - max(spr.values())
    print(f'{cname} b{batch}: native median {med[True]:.1f} us (spread {spr[True]:.1f}, {n[True]} launches) | composed '
          f'median {med[False]:.1f} us (spread {spr[False]:.1f}, {n[False]} launches) | ratio '
          f'{med[False] / med[True]:.2f}x | native below composed by more than the larger spread: {ok}', flush=True)
    return ok


def trace(cname, batch, steps=5):
    set_native(True)
    c, step = build(cname, batch)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    f, b = gemm_flops(c, batch)
    print(f'{cname} b{batch}: {steps} native steps; GEMM FLOP per step: forward {f / 1e9:.3f} G, backward {b / 1e9:.3f} G')


def stats(path, cname, batch):
    import bench as B
    c = B.CONFIGS[cname]
    f, b = gemm_flops(c, batch)
    sums = c['S'] * (1 + c['ns'])
    if path.endswith('.db'):                    # rocprofv3's default output: the rocpd database of the run
        import sqlite3
        db = sqlite3.connect(path)
        rows = [{'Name': n, 'Calls': c, 'TotalDurationNs': d} for n, c, d in
                db.execute('select name, count(*), sum(duration) from kernels group by name')]
    else:                                       # --output-format csv: ..._kernel_stats.csv
        with open(path) as fh:
            rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: -float(r['TotalDurationNs']))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    print(f'device time of the traced run: {total / 1e3:.1f} us in {sum(int(r["Calls"]) for r in rows)} launches; top kernels:')
    for r in rows[:8]:
        print(f'  {float(r["TotalDurationNs"]) / 1e3:9.1f} us  {int(r["Calls"]):4d} calls  {r["Name"][:110]}')
    for key, flop in (('fc_gemm_fwd_k', f), ('fc_bwd_gemm_k', b)):
        hit = [r for r in rows if key in r.get('Name', '')]
        if not hit:
            print(f'{key}: not in {path}')
            continue
        calls = sum(int(r['Calls']) for r in hit)
        total_ns = sum(float(r['TotalDurationNs']) for r in hit)
        per_step_ns = total_ns / (calls / sums)
        rate = flop / (per_step_ns * 1e-9)
        print(f'{cname} b{batch} {key}: {calls} calls, {total_ns / calls / 1e3:.1f} us each, {per_step_ns / 1e3:.1f} us per '
              f'step for {flop / 1e9:.3f} GFLOP = {rate / 1e12:.2f} TFLOP/s = {100 * rate / PEAK_FP32_MFMA:.1f}% of the '
              f'{PEAK_FP32_MFMA / 1e12:.1f} TF fp32-MFMA peak')


# ------------------------------------------------------------------------------------------------- the found stage
FOUND_CASES = [('mmimdb', 128), ('ntu', 64)]
FOUND_EDGES = [('fc_relu', 0), ('fc_mish', 0), ('fc_mish', 1), ('fc_relu', 2)]      # both kinds, input 0 read twice
LEG_SECONDS = 300


def build_found(cname, batch):
    """-> model, criterion, batch: bench.FoundNet's wiring over bench's fixed step nodes with FOUND_EDGES as the
    cell-level edges."""
    import bench as B
    from bmnas import nn as bnn
    from models.search.darts.genotypes import Genotype
    from models.search.darts.model import Found_FusionNetwork
    c = B.CONFIGS[cname]
    base = B.found_genotype(cname)
    geno = Genotype(edges=list(FOUND_EDGES), steps=base.steps, concat=base.concat)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.fusion_net = Found_FusionNetwork(c['S'], c['M'], c['N'], 2, B.make_args(c), None, geno)
            self.central_classifier = bnn.Linear(c['M'] * c['C'] * c['L'], c['nout'])

        def forward(self, xs):
            return self.fusion_net.forward_classified(list(xs), self.central_classifier)
    torch.manual_seed(2)
    model = Net().to('cuda:0').train()
    crit = bnn.BCEWithLogitsLoss() if c['loss'] == 'bce' else bnn.CrossEntropyLoss()
    xs, y = B.synth_batch(c, batch, torch.device('cuda:0'), 0)
    return model, crit, [x.detach() for x in xs], y


def found_leg(cname, batch, kind, composed_only, regions=5, warmup=3):
    """One child: `kind` = 'eager' | 'captured'.  Both routes in this process, alternating region by region."""
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    routes = (False,) if composed_only else (True, False)
    steps = {}
    for on in routes:
        set_native(on)
        model, crit, xs, y = build_found(cname, batch)
        opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
        if kind == 'captured':
            g = GraphedTrainStep(model, crit, opt, xs, y)           # the route is taken at capture
            steps[on] = (lambda g=g, xs=xs, y=y: g(xs, y))
        else:
            def eager(model=model, crit=crit, opt=opt, xs=xs, y=y, on=on):
                set_native(on)
                opt.zero_grad()
                loss = crit(model(xs), y)
                loss.backward()
                opt.step()
                return loss
            steps[on] = eager
    for on in routes:
        for _ in range(warmup):
            steps[on]()
    torch.cuda.synchronize()
    per = 200 if kind == 'captured' else 20                 # steps per timed region; times are per step
    t = {on: [] for on in routes}
    for _ in range(regions):
        for on in routes:
            step = steps[on]
            t[on].append(timed(lambda: [step() for _ in range(per)]) / per)
    out = []
    for on in routes:
        n = launches(steps[on])
        out.append(f"{'native' if on else 'composed'} median {statistics.median(t[on]):.1f} us (spread "
                   f'{max(t[on]) - min(t[on]):.1f}, {n} device events)')
    line = f'found {cname} b{batch} {kind} ({per} steps per region), tree {ROOT}: ' + ' | '.join(out)
    if not composed_only:
        med = {on: statistics.median(v) for on, v in t.items()}
        spread = max(max(v) - min(v) for v in t.values())
        line += (f' | ratio {med[False] / med[True]:.2f}x | native below composed by more than the larger spread: '
                 f'{med[True] < med[False] - spread}')
    if not composed_only:
        set_native(True)
    print(line, flush=True)


def found_stage(a):
    """Every leg a child process under its own time limit; nothing more is started after a leg that did not end well."""
    for cname, batch in FOUND_CASES:
        for kind in ('eager', 'captured'):
            cmd = [sys.executable, os.path.abspath(__file__), '--stage', 'found', '--leg', f'{cname}:{batch}:{kind}']
            if a.composed_only:
                cmd.append('--composed-only')
            if a.tree:
                cmd += ['--tree', a.tree]
            try:
                rc = subprocess.run(cmd, timeout=LEG_SECONDS).returncode
            except subprocess.TimeoutExpired:
                rc = 124
            if rc != 0:
                raise SystemExit(f'leg {cname}:{batch}:{kind} ended with {rc}: stopping')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trace', help='CNAME:BATCH — run native steps only (for a rocprofv3 --kernel-trace --stats run)')
    ap.add_argument('--stats', help='kernel_stats.csv of such a run: FLOP/s of the GEMM launches')
    ap.add_argument('--tree', help='import the project from this checkout instead of the one the tool lies in')
    ap.add_argument('--composed-only', action='store_true', help='time the composed path alone')
    ap.add_argument('--stage', choices=['search', 'found'], default='search',
                    help="found: the FC edges of a found network (a training step, eager and captured)")
    ap.add_argument('--leg', help='CNAME:BATCH:eager|captured — one leg of --stage found (what the children run)')
    a = ap.parse_args()
    if a.stage == 'found':
        if a.leg:
            cname, batch, kind = a.leg.split(':')
            return found_leg(cname, int(batch), kind, a.composed_only)
        return found_stage(a)
    if a.composed_only:
        for cname, batch in CASES:
            measure_composed(cname, batch)
        return
    if a.trace:
        cname, batch = a.trace.split(':')
        if a.stats:
            return stats(a.stats, cname, int(batch))
        return trace(cname, int(batch))
    oks = [measure(cname, batch) for cname, batch in CASES]
    print('all configurations meet the criterion:', all(oks))


if __name__ == '__main__':
    main()
