#!/usr/bin/env python3
"""One eager search step with an edited STEP_STEP_PRIMITIVES list: the selected-term kernels (csrc/nodemix_sel.hip,
bmnas.functions.NodeMixedSelFn) against the composed sum (NodeMixedOp primitive by primitive through aten).

    python tools/node_prims_time.py                    # every list x (MM-IMDB b128, NTU b64, NTU b8): both paths
                                                       # ALTERNATING, five timed regions each (device events, after
                                                       # warm-up): medians, spreads (max - min), device launches per step
    python tools/node_prims_time.py --composed-only [--tree PARENT_CHECKOUT]
                                                       # the composed path alone, optionally imported from another
                                                       # checkout (the parent commit, whose only path it is for these
                                                       # lists): has the fallback got slower?
    rocprofv3 --kernel-trace --stats -d DIR -o np -- python tools/node_prims_time.py --trace mmimdb:128 --list Sum,LinearGLU,ConcatFC
    python tools/node_prims_time.py --stats DIR/.../np_results.db --trace mmimdb:128 --list Sum,LinearGLU,ConcatFC
                                                       # moved bytes / duration of the two new kernels from that trace

Lists with CatConvMish (reference node_operations.py:58-82; registered here the way a user registers it): "composed" is
what a user had before the primitive was mirrored — a plain-torch CatConvMish defined in this file, which routes
composed in any checkout — and "native" the project's class in the mix kernels' FC slot; the two models are built from
the same seed and timed alternating.  With --composed-only --tree PARENT the same plain-torch baseline runs on the parent
commit; --default-list times the unedited list's step alone (on either tree: it must not have moved).

Without --leg / --trace / --stats the tool is a driver: every (list, configuration) leg runs as a child process of its
own under a time limit, one after the other, and the first leg that fails (or runs out of time) ends the run.

A step = forward + criterion + backward in train mode with dropout on, bench.CONFIGS shapes, bench.synth_batch data.
"""
import argparse
import csv
import os
import statistics
import subprocess
import sys

HERE = os.path.abspath(__file__)
ROOT = os.path.dirname(os.path.dirname(HERE))
if '--tree' in sys.argv:                   # another checkout of the project (the parent commit) to import from
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))

MISH = 'CatConvMish'
DEFAULT = ['Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC']
LISTS = [['Sum', 'ScaleDotAttn'], ['Sum', 'LinearGLU', 'ConcatFC'], ['ScaleDotAttn', 'ConcatFC', 'Sum'], ['ConcatFC'],
         ['Sum', 'ScaleDotAttn', 'LinearGLU', MISH], [MISH]]
CASES = [('mmimdb', 128), ('ntu', 64), ('ntu', 8)]
PEAK_HBM = 8.0e12                          # bytes / s
LEG_SECONDS = 240


def plain_cat_conv_mish():
    """The module a user of the reference writes in plain torch (node_operations.py:58-82)."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class CatConvMish(nn.Module):
        def __init__(self, C, args):
            super().__init__()
            self.conv = nn.Conv1d(2 * C, C, 1, 1)
            self.bn = nn.BatchNorm1d(C)
            self.dropout = nn.Dropout(args.drpt)

        def forward(self, x, y):
            out = self.bn(self.conv(torch.cat([x, y], dim=1)))
            return self.dropout(out * torch.tanh(F.softplus(out)))
    return CatConvMish


def build(cname, batch, prims, plain=False):
    import torch
    import bench as B
    import models.search.darts.genotypes as gt
    import models.search.darts.node_operations as no
    from bmnas import nn as bnn
    c = B.CONFIGS[cname]
    saved = list(gt.STEP_STEP_PRIMITIVES)
    gt.STEP_STEP_PRIMITIVES[:] = prims
    if MISH in prims:
        cls = plain_cat_conv_mish() if plain else no.CatConvMish
        no.STEP_STEP_OPS[MISH] = lambda C, L, args: cls(C, args)
    try:
        torch.manual_seed(2)
        model = B.HyperNet(c, 'F', cname).to('cuda:0').train()
    finally:
        gt.STEP_STEP_PRIMITIVES[:] = saved
        no.STEP_STEP_OPS.pop(MISH, None)
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
    from models.search.darts import node_operations as no
    if hasattr(no, 'NODE_PRIMS_NATIVE'):
        no.NODE_PRIMS_NATIVE = bool(on)
    elif on:
        raise RuntimeError('this checkout has no native path for edited STEP_STEP_PRIMITIVES lists')


def launches(step):
    import torch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        step()
        torch.cuda.synchronize()
    return sum(1 for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA)


def timed(step):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    step()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3            # us


def measure_composed(cname, batch, prims, regions=5, warmup=3):
    """One path alone: the composed sum of an edited list (CatConvMish in plain torch), or the default list's step."""
    import torch
    c, step = build(cname, batch, prims, plain=True)
    what = 'default list alone' if prims == DEFAULT else 'composed alone'
    if prims != DEFAULT:
        set_native(False)
    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    t = [timed(step) for _ in range(regions)]
    print(f'{"+".join(prims)} {cname} b{batch}: {what}, tree {os.path.basename(ROOT)}: median {statistics.median(t):.1f} us '
          f'(spread {max(t) - min(t):.1f}, {launches(step)} launches)', flush=True)
    return True


def measure(cname, batch, prims, regions=5, warmup=3):
    import torch
    c, native_step = build(cname, batch, prims)
    # the baseline of a CatConvMish list: the plain-torch module (a model of its own, same seed)
    steps = {True: native_step, False: build(cname, batch, prims, plain=True)[1] if MISH in prims else native_step}
    for on in (True, False):
        set_native(on)
        for _ in range(warmup):
            steps[on]()
    torch.cuda.synchronize()
    t = {True: [], False: []}
    for _ in range(regions):
        for on in (True, False):
            set_native(on)
            t[on].append(timed(steps[on]))
    n = {}
    for on in (True, False):
        set_native(on)
        n[on] = launches(steps[on])
    set_native(True)
    med = {k: statistics.median(v) for k, v in t.items()}
    spr = {k: max(v) - min(v) for k, v in t.items()}
    ok = med[True] < med[False] - max(spr.values())
    print(f'{"+".join(prims)} {cname} b{batch}: native median {med[True]:.1f} us (spread {spr[True]:.1f}, {n[True]} '
          f'launches) | composed median {med[False]:.1f} us (spread {spr[False]:.1f}, {n[False]} launches) | ratio '
          f'{med[False] / med[True]:.2f}x | native below composed by more than the larger spread: {ok}', flush=True)
    return ok


def trace(cname, batch, prims, steps=5):
    import torch
    set_native(True)
    c, step = build(cname, batch, prims)
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    print(f'{"+".join(prims)} {cname} b{batch}: {steps} native steps')


def moved_bytes(c, batch, prims):
    """(forward, backward) bytes one launch of the two new kernels has to move: T = one (b, C, L) fp32 tensor.
    forward: reads z (Sum; x is y in a search step), p1 (attention), U (conv rows / C tensors), writes out;
    backward: reads g and the same operands, writes dV (conv rows / C tensors) and dx (Sum)."""
    T = batch * c['C'] * c['L'] * 4
    rows = (2 if 'LinearGLU' in prims else 0) + (1 if 'ConcatFC' in prims or MISH in prims else 0)
    ops = ('Sum' in prims) + ('ScaleDotAttn' in prims) + rows
    return (ops + 1) * T, (1 + ops + rows + ('Sum' in prims)) * T


def stats(path, cname, batch, prims):
    import bench as B
    c = B.CONFIGS[cname]
    if path.endswith('.db'):                    # rocprofv3's default output: the rocpd database of the run
        import sqlite3
        db = sqlite3.connect(path)
        rows = [{'Name': n, 'Calls': k, 'TotalDurationNs': d} for n, k, d in
                db.execute('select name, count(*), sum(duration) from kernels group by name')]
    else:                                       # --output-format csv: ..._kernel_stats.csv
        with open(path) as fh:
            rows = list(csv.DictReader(fh))
    rows.sort(key=lambda r: -float(r['TotalDurationNs']))
    total = sum(float(r['TotalDurationNs']) for r in rows)
    print(f'device time of the traced run: {total / 1e3:.1f} us in {sum(int(r["Calls"]) for r in rows)} launches; top kernels:')
    for r in rows[:8]:
        print(f'  {float(r["TotalDurationNs"]) / 1e3:9.1f} us  {int(r["Calls"]):4d} calls  {r["Name"][:110]}')
    for key, nbytes in zip(('node_mix_sel_fwd_k', 'node_mix_sel_bwd_k'), moved_bytes(c, batch, prims)):
        hit = [r for r in rows if key in r.get('Name', '')]
        if not hit:
            print(f'{key}: not in {path}')
            continue
        calls = sum(int(r['Calls']) for r in hit)
        each = sum(float(r['TotalDurationNs']) for r in hit) / calls
        rate = nbytes / (each * 1e-9)
        print(f'{"+".join(prims)} {cname} b{batch} {key}: {calls} calls, {each / 1e3:.1f} us each for {nbytes / 1e6:.2f} MB '
              f'= {rate / 1e12:.2f} TB/s = {100 * rate / PEAK_HBM:.1f}% of the {PEAK_HBM / 1e12:.0f} TB/s HBM peak')


def drive(a):
    """Every leg as a child process under its own time limit; the first failure ends the run."""
    lists = [DEFAULT] if a.default_list else [p for p in LISTS if not a.only or a.only in p]
    for prims in lists:
        for cname, batch in CASES:
            cmd = [sys.executable, HERE, '--leg', f'{cname}:{batch}', '--list', ','.join(prims)]
            if a.composed_only or a.default_list:
                cmd.append('--composed-only')
            if a.tree:
                cmd += ['--tree', a.tree]
            rc = subprocess.run(['timeout', '-k', '10', str(LEG_SECONDS)] + cmd).returncode
            if rc != 0:
                print(f'leg {" ".join(cmd[2:])} ended with status {rc}: stopping here', flush=True)
                return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--leg', help='CNAME:BATCH — time this one configuration in this process')
    ap.add_argument('--list', help='comma-separated primitive list of the leg / trace')
    ap.add_argument('--trace', help='CNAME:BATCH — run native steps only (for a rocprofv3 --kernel-trace --stats run)')
    ap.add_argument('--stats', help='results of such a run: moved bytes over duration of the two new kernels')
    ap.add_argument('--tree', help='import the project from this checkout instead of the one the tool lies in')
    ap.add_argument('--composed-only', action='store_true', help='time the composed path alone')
    ap.add_argument('--default-list', action='store_true', help='driver: time the default list\'s step alone')
    ap.add_argument('--only', help='driver: only the lists that hold this primitive')
    a = ap.parse_args()
    prims = a.list.split(',') if a.list else None
    if a.trace:
        cname, batch = a.trace.split(':')
        if a.stats:
            return stats(a.stats, cname, int(batch), prims)
        return trace(cname, int(batch), prims)
    if a.leg:
        cname, batch = a.leg.split(':')
        (measure_composed if a.composed_only else measure)(cname, int(batch), prims)
        return 0
    return drive(a)


if __name__ == '__main__':
    sys.exit(main() or 0)
