"""Timing of the MultiHeadAttn step-node primitive on cuda:0 (prints; profiles/r17_mha.txt keeps a run).

  A. one eager forward + backward of MultiHeadAttn(x, y) at the two flagship shapes (MM-IMDB b128 C192 L16, NTU b64
     C128 L8; heads = 2; train mode, the configuration's dropout live): the gfx950 kernels (bmnas.functions.MhaFn)
     against the composed route (operations.MHA_NATIVE = False: the reference's transposes around
     nn.MultiheadAttention) — same process, same module, same tensors, the two variants alternating round by round;
     median and minimum over the rounds.  Before the timing: the two routes' outputs and gradients at that size, with
     dropout off, as err / (|want| + max|want|).
  B. a found network whose genotype names the primitive (two step nodes, one MultiHeadAttn each, at the MM-IMDB cell
     size), forward + criterion + backward + Adam captured as one hipGraph replay (bmnas.graph.GraphedTrainStep): the
     native route, then — if torch's own attention captures — the composed one.

Times are host clocks around work that ends in a device synchronise; every timed window is warmed up first.  No GPU:
the script fails, it does not fall back.

    python tools/mha_time.py [rounds] [iterations per round]
"""
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'bm-nas_amd')):
    sys.path.insert(0, p)
import torch

import models.search.darts.node_operations as no
import models.search.darts.operations as ops

ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 9
ITERS = int(sys.argv[2]) if len(sys.argv) > 2 else 200
MHA = 'MultiHeadAttn'
SHAPES = [('mmimdb', 128, 192, 16, 0.1), ('ntu', 64, 128, 8, 0.2)]


class Args:
    def __init__(self, C, L, drpt, heads=2):
        self.C, self.L, self.drpt, self.num_heads = C, L, drpt, heads
        self.num_input_nodes, self.num_keep_edges = 2, 2
        self.node_steps = self.node_multiplier = 1
        self.steps = self.multiplier = 2
        self.parallel, self.weight_decay = False, 1e-4


def window(fn, n):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e6


def alternate(variants, rounds, iters):
    """variants: name -> fn.  -> name -> [us per call of each round], the variants taking turns inside every round."""
    for fn in variants.values():
        window(fn, max(10, iters // 10))
    out = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():
            out[k].append(window(fn, iters))
    return out


def report(title, res):
    for k, v in res.items():
        print(f'{title}: {k:9s} median {statistics.median(v):9.1f} us   min {min(v):9.1f} us   max {max(v):9.1f} us '
              f'  ({len(v)} rounds x {ITERS})')
    if 'native' in res and 'composed' in res:
        print(f'{title}: composed / native (medians) = '
              f'{statistics.median(res["composed"]) / statistics.median(res["native"]):.2f}')


def rel_err(got, want):
    w = want.double()
    return float(((got.double() - w).abs() / (w.abs() + w.abs().max())).max())


def with_route(native, fn):
    def run():
        ops.MHA_NATIVE = native
        try:
            return fn()
        finally:
            ops.MHA_NATIVE = True
    return run


def eager_primitive(name, b, C, L, drpt):
    torch.manual_seed(0)
    m = no.MultiHeadAttn(C, L, Args(C, L, drpt)).cuda().train()
    x = torch.randn(b, C, L, device='cuda', requires_grad=True)
    y = torch.randn(b, C, L, device='cuda', requires_grad=True)
    g = torch.randn(b, C, L, device='cuda')
    assert ops.attention_route(m, x, y, y) == 'native'

    def step():
        m.zero_grad(set_to_none=True)
        x.grad = y.grad = None
        out = m(x, y)
        out.backward(g)
        return out

    # the two routes compute the same thing at this size (dropout off)
    m.attn.dropout = 0.0
    res = []
    for native in (True, False):
        out = with_route(native, step)()
        torch.cuda.synchronize()
        res.append([out.detach().clone(), x.grad.clone(), y.grad.clone()] + [p.grad.clone() for p in m.parameters()])
    names = ['out', 'dx', 'dy'] + ['d' + k for k, _ in m.named_parameters()]
    print(f'A {name} b{b} C{C} L{L} h2: native vs composed, dropout off: ' +
          ', '.join(f'{n} {rel_err(a, c):.1e}' for n, a, c in zip(names, *res)))
    m.attn.dropout = drpt
    report(f'A {name} b{b} C{C} L{L} h2 eager fwd+bwd', alternate(
        {'native': with_route(True, step), 'composed': with_route(False, step)}, ROUNDS, ITERS))


def captured_found_step(b=128, C=192, L=16, drpt=0.1, nout=23):
    from bmnas import nn as bnn
    from bmnas.graph import GraphedTrainStep
    from bmnas.optim import Adam
    from models.search.darts.genotypes import Genotype, StepGenotype
    from models.search.darts.model import Found_FusionNetwork
    args = Args(C, L, drpt)
    geno = Genotype(edges=[('skip', 0), ('skip', 1), ('skip', 1), ('skip', 0)],
                    steps=[StepGenotype(inner_edges=[('skip', 0), ('skip', 1)], inner_steps=[MHA], inner_concat=[2]),
                           StepGenotype(inner_edges=[('skip', 1), ('skip', 0)], inner_steps=[MHA], inner_concat=[2])],
                    concat=[2, 3])

    class Model(torch.nn.Module):
        def __init__(self):
            super().__init__()
            no.STEP_STEP_OPS[MHA] = lambda C_, L_, a: no.MultiHeadAttn(C_, L_, a)     # the line a user adds
            try:
                self.fusion_net = Found_FusionNetwork(2, 2, 2, 2, args, None, geno)
            finally:
                del no.STEP_STEP_OPS[MHA]
            self.central_classifier = bnn.Linear(2 * C * L, nout)

        def forward(self, xs):
            return self.fusion_net.forward_classified(list(xs), self.central_classifier)

    torch.manual_seed(0)
    xs = [torch.randn(b, C, L, device='cuda') for _ in range(2)]
    y = (torch.rand(b, nout, device='cuda') < 0.3).float()
    for native in (True, False):
        route = 'native' if native else 'composed'
        title = f'B found net, 2 x MultiHeadAttn, b{b} C{C} L{L} h2, captured step'
        ops.MHA_NATIVE = native
        try:
            torch.manual_seed(1)
            model = Model().cuda().train()
            opt = Adam(model.parameters(), lr=1e-3, weight_decay=1e-4)
            g = GraphedTrainStep(model, bnn.BCEWithLogitsLoss(), opt, xs, y)
            report(title, {route: alternate({route: lambda: g(xs, y)}, ROUNDS, ITERS)[route]})
        except Exception as e:                                   # noqa: BLE001 — torch's attention may not capture
            if native:
                raise
            print(f'{title}: composed route not captured ({type(e).__name__}: {str(e)[:200]}): not measured')
        finally:
            ops.MHA_NATIVE = True


def main():
    assert torch.cuda.is_available(), 'tools/mha_time.py measures on the GPU: no device, no number'
    print(f'device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; rounds {ROUNDS} x {ITERS} calls')
    for shape in SHAPES:
        eager_primitive(*shape)
    captured_found_step()


if __name__ == '__main__':
    main()
