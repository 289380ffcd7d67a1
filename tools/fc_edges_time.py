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

A step = forward + criterion + backward in train mode with dropout on, bench.CONFIGS shapes, bench.synth_batch data.
"""
import argparse
import csv
import os
import statistics
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--trace', help='CNAME:BATCH — run native steps only (for a rocprofv3 --kernel-trace --stats run)')
    ap.add_argument('--stats', help='kernel_stats.csv of such a run: FLOP/s of the GEMM launches')
    ap.add_argument('--tree', help='import the project from this checkout instead of the one the tool lies in')
    ap.add_argument('--composed-only', action='store_true', help='time the composed path alone')
    a = ap.parse_args()
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
