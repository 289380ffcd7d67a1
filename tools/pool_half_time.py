#!/usr/bin/env python3
"""The reshape layers' pooling launch (csrc/pool.hip) on bf16 feature maps against the fp32 ways, at the raw shapes of
SURVEY.md (tier X): NTU b8 / b64, MM-IMDB b128, Ego b48.  Forward, three forms on the same build:

    fp32     the launch on fp32 maps (what a backbone outside torch.autocast hands over)
    bf16     the launch on bf16 maps as they are (bmnas_adaptive_maxpool_fwd_group_ex, 16-byte loads)
    cast     the bf16 maps through .float() and then the fp32 launch — the only way there was before
    parent   (--parent-lib PATH: another build of libbmnas_hip.so) that build's bmnas_adaptive_maxpool_fwd_group on the
             fp32 maps

and backward (gather form, every dx element written once) as fp32 / bf16 / parent.  MM-IMDB's two text vectors stay
fp32 beside bf16 image maps, as under autocast of the image backbone alone; every other map is bf16.

    python tools/pool_half_time.py [--parent-lib PATH]

A case = one child process.  Every form is R launches captured in one graph (a replay is not host-bound) that walk over
enough copies of the maps to exceed the 256 MiB Infinity Cache between two reads of the same bytes; the forms ALTERNATE
region by region, five timed regions each (device events, after warm-up): medians, spreads (max - min), and the rate of
the launch's own bytes (maps read + pooled values and indices written; backward: indices and gradients read + dx
written) against the HBM peak.  Then one captured found-stage MM-IMDB step (reshape layers + found network + classifier
+ criterion + backward + Adam, b128) fed bf16 and fp32 raw maps, alternating likewise.
No time is a pass / fail criterion.  Every case is a child process under its own time limit, and the tool stops at the
first one that does not exit with 0: nothing more is started on the GPU after it."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))

HBM_PEAK_GBS = 8000.0
SHAPES = {
    'mmimdb': (16, 'mmimdb', [(512, 20, 32), (512, 20, 32), (512, 10, 16), (512, 5, 8), (64,), (128,)]),
    'ntu': (8, 'video', [(512, 8, 32, 32), (1024, 8, 16, 16), (2048, 8, 8, 8), (2048,), (128, 4, 4), (256, 2, 2),
                         (1024,), (512,)]),
    'ego': (8, 'video', [(512, 8, 14, 14), (1024, 4, 7, 7), (2048, 2, 4, 4), (2048, 1, 1, 1)] * 2),
}
CASES = [('ntu', 8), ('ntu', 64), ('mmimdb', 128), ('ego', 48)]
CASE_SECONDS = 300
REGIONS, WARMUP, LAUNCHES = 5, 2, 8
WORKING_SET = 768 << 20            # bytes of maps a form walks over before it reads the same ones again


def _timed(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3            # us


def _alternate(forms, per):
    """forms: name -> callable of `per` launches -> name -> [us per launch] over REGIONS alternating regions"""
    import torch
    for fn in forms.values():
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in forms}
    for _ in range(REGIONS):
        for k, fn in forms.items():
            t[k].append(_timed(fn) / per)
    return t


def _graph(body):
    import torch
    g = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()                                   # (first call outside the capture: lazy initialisation)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    with torch.cuda.graph(g):
        body()
    return g.replay


def pool_case(cname, batch, parent_lib):
    import torch
    import models.auxiliary.aux_models as aux
    from bmnas import lib
    dev = torch.device('cuda:0')
    L, kind, shapes = SHAPES[cname]
    cls = aux.ReshapeInputLayer_MMIMDB if kind == 'mmimdb' else aux.ReshapeInputLayer

    class A:
        drpt = 0.0

    metas = [torch.empty((batch,) + s, device='meta') for s in shapes]
    dims = [cls(s[0], 16, L, A()).pool_dims(m) for s, m in zip(shapes, metas)]
    half = [not (cname == 'mmimdb' and len(s) == 1) for s in shapes]
    n_in = sum(m.numel() for m in metas)
    n_out = sum(batch * d[0] * d[3] * d[4] for d in dims)
    copies = max(2, -(-WORKING_SET // (2 * n_in)))
    gen = torch.Generator(device=dev).manual_seed(0)
    maps32 = [[torch.relu(torch.randn((batch,) + s, device=dev, generator=gen)) for s in shapes]
              for _ in range(max(2, -(-WORKING_SET // (4 * n_in))))]
    maps16 = [[(torch.relu(torch.randn((batch,) + s, device=dev, generator=gen)).bfloat16() if h else
                torch.relu(torch.randn((batch,) + s, device=dev, generator=gen))) for s, h in zip(shapes, half)]
              for _ in range(copies)]
    outs = [torch.empty((batch, d[0], d[3] * d[4]), device=dev) for d in dims]
    idxs = [torch.empty((batch, d[0], d[3] * d[4]), device=dev, dtype=torch.int32) for d in dims]
    gs = [torch.randn_like(o) for o in outs]
    dx32 = [torch.empty_like(x) for x in maps32[0]]
    dx16 = [torch.empty_like(x) for x in maps16[0]]
    stream = lambda: torch.cuda.current_stream().cuda_stream

    parent = None
    if parent_lib:
        so = ctypes.CDLL(parent_lib)
        for name in ('bmnas_adaptive_maxpool_fwd_group', 'bmnas_adaptive_maxpool_bwd_group'):
            getattr(so, name).argtypes, getattr(so, name).restype = lib.SIGNATURES[name]

        def parent(direction, xs, dxs=None):
            probs = (lib.PoolProb * len(dims))()
            for i, (Cc, H, W, oh, ow) in enumerate(dims):
                probs[i] = lib.PoolProb(None if xs is None else xs[i].data_ptr(), outs[i].data_ptr(), idxs[i].data_ptr(),
                                        gs[i].data_ptr(), None if dxs is None else dxs[i].data_ptr(), Cc, H, W, oh, ow)
            rc = getattr(so, f'bmnas_adaptive_maxpool_{direction}_group')(probs, len(dims), batch, stream())
            assert rc == 0, rc

    def walk(maps, fn):
        return lambda: [fn(maps[i % len(maps)]) for i in range(LAUNCHES)]

    fwd = {'fp32': _graph(walk(maps32, lambda xs: lib.adaptive_maxpool_group(xs, dims, outs, idxs, batch))),
           'bf16': _graph(walk(maps16, lambda xs: lib.adaptive_maxpool_group(xs, dims, outs, idxs, batch))),
           'cast': _graph(walk(maps16, lambda xs: lib.adaptive_maxpool_group([x.float() for x in xs], dims, outs, idxs,
                                                                              batch)))}
    if parent:
        fwd['parent'] = _graph(walk(maps32, lambda xs: parent('fwd', xs)))
    out = {'case': f'{cname} b{batch}', 'elements': n_in, 'copies': {'fp32': len(maps32), 'bf16': len(maps16)}}
    half_in = sum(m.numel() * (2 if h else 4) for m, h in zip(metas, half))
    bytes_ = {'fp32': 4 * n_in + 8 * n_out, 'bf16': half_in + 8 * n_out, 'cast': half_in + 8 * n_out,
              'parent': 4 * n_in + 8 * n_out}
    t = _alternate(fwd, LAUNCHES)
    out['fwd'] = {k: {'regions_us': v, 'bytes': bytes_[k]} for k, v in t.items()}
    # backward: one launch per graph node over the same idx / g (small), dx of either type
    lib.adaptive_maxpool_group(maps32[0], dims, outs, idxs, batch)
    torch.cuda.synchronize()
    bwd = {'fp32': _graph(lambda: [lib.adaptive_maxpool_group_bwd(gs, idxs, dx32, dims, batch) for _ in range(LAUNCHES)]),
           'bf16': _graph(lambda: [lib.adaptive_maxpool_group_bwd(gs, idxs, dx16, dims, batch) for _ in range(LAUNCHES)])}
    if parent:
        bwd['parent'] = _graph(lambda: [parent('bwd', None, dx32) for _ in range(LAUNCHES)])
    t = _alternate(bwd, LAUNCHES)
    bytes_ = {'fp32': 4 * n_in + 8 * n_out, 'bf16': half_in + 8 * n_out, 'parent': 4 * n_in + 8 * n_out}
    out['bwd'] = {k: {'regions_us': v, 'bytes': bytes_[k]} for k, v in t.items()}
    print('RESULT ' + json.dumps(out), flush=True)


def step_case(batch):
    """one captured found-stage MM-IMDB step over raw maps, bf16 image maps against fp32 ones"""
    import torch
    import torch.nn as nn
    import bench as B
    import models.auxiliary.aux_models as aux
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    from models.search._common import HyperNetBase
    dev = torch.device('cuda:0')
    c = B.CONFIGS['mmimdb']
    args = B.make_args(c)
    genotype = B.found_genotype('mmimdb')
    _, _, shapes = SHAPES['mmimdb']

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.reshape_layers = HyperNetBase.make_reshape_layers(aux.ReshapeInputLayer_MMIMDB, B.C_INS['mmimdb'], args,
                                                                   genotype)
            self.found = B.FoundNet(c, 'mmimdb')

        def forward(self, raws):
            return self.found(aux.reshape_all(list(self.reshape_layers), list(raws)))

    gen = torch.Generator(device=dev).manual_seed(0)
    y = (torch.rand(batch, c['nout'], device=dev, generator=gen) < 0.2).float()
    steps = {}
    for name in ('fp32', 'bf16'):
        torch.manual_seed(2)
        model = Net().to(dev).train()
        xs = [torch.relu(torch.randn((batch,) + s, device=dev, generator=gen)) for s in shapes]
        if name == 'bf16':
            xs = [x.bfloat16() if x.dim() > 2 else x for x in xs]
        g = GraphedTrainStep(model, bnn.BCEWithLogitsLoss(), Adam(model.parameters(), lr=1e-3, weight_decay=1e-4), xs, y)
        steps[name] = (lambda g=g, xs=xs: [g(xs, y) for _ in range(20)])
    t = _alternate(steps, 20)
    print('RESULT ' + json.dumps({'case': f'found-stage step over raw maps, mmimdb b{batch}',
                                  'step': {k: {'regions_us': v} for k, v in t.items()}}), flush=True)


def run_case(spec, parent_lib):
    """-> the child's result.  Any ending but exit status 0 — an exception, a time limit, a signal — stops the tool:
    nothing more is started on the GPU."""
    cmd = [sys.executable, os.path.abspath(__file__), '--case', spec] + (['--parent-lib', parent_lib] if parent_lib else [])
    try:
        p = subprocess.run(cmd, timeout=CASE_SECONDS, stdout=subprocess.PIPE, text=True)
        rc, text = p.returncode, p.stdout
    except subprocess.TimeoutExpired:
        rc, text = 124, ''
    if rc != 0:
        raise SystemExit(f'case {spec} ended with {rc}: stopping')
    line = [ln for ln in text.splitlines() if ln.startswith('RESULT ')][-1]
    return json.loads(line[len('RESULT '):])


def _report(title, forms, base):
    print(f'  {title}')
    med = {k: statistics.median(v['regions_us']) for k, v in forms.items()}
    for k, v in forms.items():
        ts = v['regions_us']
        line = f'    {k:<7} median {med[k]:9.1f} us (spread {max(ts) - min(ts):.1f} over {len(ts)} regions)'
        if 'bytes' in v:
            rate = v['bytes'] / med[k] / 1e3
            line += f", {v['bytes'] / 1e6:.1f} MB -> {rate:.0f} GB/s = {100 * rate / HBM_PEAK_GBS:.0f}% of the HBM peak"
        if k != base:
            line += f'; against {base} {med[k] / med[base]:.2f} x'
        print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--case', help='CNAME:BATCH or step:BATCH — one case (what the children run)')
    ap.add_argument('--parent-lib', help='another build of libbmnas_hip.so to time the fp32 launches of')
    a = ap.parse_args()
    if a.case:
        cname, batch = a.case.split(':')
        return step_case(int(batch)) if cname == 'step' else pool_case(cname, int(batch), a.parent_lib)
    for cname, batch in CASES:
        r = run_case(f'{cname}:{batch}', a.parent_lib)
        print(f"{r['case']}: {r['elements'] / 1e6:.1f} M elements per launch, {r['copies']} copies of the maps in turn")
        _report('forward', r['fwd'], 'bf16')
        _report('backward', r['bwd'], 'bf16')
    r = run_case('step:128', None)
    print(r['case'])
    _report('one replay', r['step'], 'bf16')


if __name__ == '__main__':
    main()
