#!/usr/bin/env python3
"""What the trainer loop's phase statistics cost per batch, with the loop's meters and with `args.device_stats`
(bmnas.metrics.PhaseStats: one launch, or the last node of the captured forward), on the same build:

    tally    the phase-statistics launch alone: R launches captured in one graph, replayed and timed with device events
             (us per launch), and the device events of ONE eager PhaseStats.update (the structural condition: one, none
             of aten)
    eval     a found-stage eval batch (bench.FoundNet, eval mode): the GraphedForward replay plus the bookkeeping
    dev      a dev-phase metric batch (bench.HyperNet, train mode — dropout live, BatchNorm updating, as the reference's
             dev phase keeps it): the same
             ... each in two forms that ALTERNATE region by region:
             meter   replay; `loss_sum += loss.double() * n`; meter.update(output, labels) — the loop's own statements,
                     _loop.AccuracyMeter / _loop.F1Meter('weighted', 0.3)
             device  the replay of a GraphedForward(stats=PhaseStats): nothing else is issued

    python tools/phase_stats_time.py            # MM-IMDB b128 / O23 (F1) and NTU b64 / O60 (accuracy)
    python tools/phase_stats_time.py --meter-only     # the meter forms alone: runs on a checkout without bmnas.metrics

Per form: median and spread (max - min) of five timed regions of device-event time per batch, after warm-up; device
events per batch and how many of them are aten's.  The meter form's phase-end work (F1Meter: concatenation, the copy of
every prediction to the host, sklearn) is not in its per-batch time; it is timed once per region length and printed
beside it.  No time is a pass / fail criterion.  Every case is a child process under its own time limit, and the tool
stops at the first one that does not exit with 0: nothing more is started on the GPU after it.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))

CASES = [('mmimdb', 128), ('ntu', 64)]
CASE_SECONDS = 300
REGIONS, WARMUP, PER = 5, 3, 200
TALLY_LAUNCHES = 50


def case(cname, batch, meter_only):
    import torch
    import bench as B
    import models.search.train_searchable._loop as loop
    from bmnas import nn as bnn
    from bmnas.graph import GraphedForward
    from torch.profiler import ProfilerActivity, profile
    dev = torch.device('cuda:0')
    c = B.CONFIGS[cname]
    f1 = c['loss'] == 'bce'
    PhaseStats = None
    if not meter_only:
        from bmnas.metrics import PhaseStats
    xs, y = B.synth_batch(c, batch, dev, 0)
    xs = [x.detach() for x in xs]
    n = y.shape[0]

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e3            # us

    def events(fn):
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        return {'device_events': len(names), 'aten_events': sum('at::native' in k for k in names),
                'stats_events': sum('phase_stats_' in k for k in names)}

    out = {'case': f"{cname} b{batch} / O{c['nout']} ({'F1' if f1 else 'accuracy'})"}
    forms = {}
    for leg in ('eval', 'dev'):
        torch.manual_seed(2)
        model = (B.FoundNet(c, cname) if leg == 'eval' else B.HyperNet(c, 'F', cname)).to(dev)
        model.eval() if leg == 'eval' else model.train()
        crit = bnn.BCEWithLogitsLoss() if f1 else bnn.CrossEntropyLoss()
        meter = loop.F1Meter('weighted', 0.3) if f1 else loop.AccuracyMeter()
        meter.reset(dev)
        g = GraphedForward(model, crit, xs, y)
        state = {'loss_sum': torch.zeros((), device=dev, dtype=torch.float64)}

        def with_meter(g=g, meter=meter, state=state):
            loss, output = g(xs, y)
            state['loss_sum'] += loss.detach().double() * n
            meter.update(output.detach(), y)

        forms[leg + ' meter'] = (with_meter, meter)
        if PhaseStats is not None:
            stats = PhaseStats.from_meter(meter)
            stats.reset(dev)
            gs = GraphedForward(model, crit, xs, y, stats=stats)
            assert gs.stats is stats
            forms[leg + ' device'] = (lambda gs=gs: gs(xs, y), None)
    for k, (fn, _) in forms.items():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    ends = {k: [] for k in forms}
    for _ in range(REGIONS):
        for k, (fn, meter) in forms.items():
            if meter is not None:
                meter.reset(dev)                  # (a phase of PER batches: F1Meter keeps every one of them)
            t[k].append(timed(lambda: [fn() for _ in range(PER)]) / PER)
            if meter is not None:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                meter.compute(PER * n)
                ends[k].append((time.perf_counter() - t0) * 1e6)
    events(forms['eval meter'][0])                # (the first profile of a process misses replayed kernels)
    for k, (fn, meter) in forms.items():
        if meter is not None:
            meter.reset(dev)
        out[k] = dict(events(fn), regions_us=t[k], phase_end_us=ends[k])

    if PhaseStats is not None:
        # the tally alone, on logits and labels of the case's shape: R launches in one graph
        logits = torch.randn(n, c['nout'], device=dev)
        loss = torch.ones((), device=dev)
        stats = PhaseStats('f1', 'weighted', 0.3) if f1 else PhaseStats('acc')
        stats.reset(dev)
        stats.update(loss, logits, y)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            for _ in range(TALLY_LAUNCHES):
                stats.update(loss, logits, y)
        for _ in range(WARMUP):
            graph.replay()
        torch.cuda.synchronize()
        assert stats.fallbacks == 0
        out['tally'] = dict(events(lambda: stats.update(loss, logits, y)),
                            regions_us=[timed(lambda: [graph.replay() for _ in range(20)]) / (20 * TALLY_LAUNCHES)
                                        for _ in range(REGIONS)], phase_end_us=[])
    print('RESULT ' + json.dumps(out), flush=True)


def run_case(cname, batch, meter_only):
    """-> the child's result.  Any ending but exit status 0 — an exception, a time limit, a signal — stops the tool:
    nothing more is started on the GPU."""
    cmd = [sys.executable, os.path.abspath(__file__), '--case', f'{cname}:{batch}']
    if meter_only:
        cmd.append('--meter-only')
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
    ap.add_argument('--meter-only', action='store_true', help='the meter forms alone (a checkout without bmnas.metrics)')
    a = ap.parse_args()
    if a.case:
        cname, batch = a.case.split(':')
        return case(cname, int(batch), a.meter_only)
    for cname, batch in CASES:
        r = run_case(cname, batch, a.meter_only)
        print(r.pop('case'))
        for k, v in r.items():
            ts = v['regions_us']
            line = (f"  {k:<12} median {statistics.median(ts):8.2f} us per {'launch' if k == 'tally' else 'batch'} "
                    f"(spread {max(ts) - min(ts):.2f} over {len(ts)} regions), {v['device_events']} device events "
                    f"({v['aten_events']} aten, {v['stats_events']} phase_stats)")
            if v['phase_end_us']:
                line += f"; phase end after {PER} batches: median {statistics.median(v['phase_end_us']):.0f} us on the host"
            if k.endswith(' device'):
                base = statistics.median(r[k.replace(' device', ' meter')]['regions_us'])
                line += f"; against meter {statistics.median(ts) - base:+.2f} us"
            print(line, flush=True)


if __name__ == '__main__':
    main()
