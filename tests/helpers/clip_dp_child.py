"""Child process of tests/test_grad_clip_network_gpu.py: ONE rank of a 2-rank data-parallel run with gradient-norm
clipping in the weight optimizer (args.grad_clip -> bmnas.optim.Adam(max_grad_norm=...)), both ranks on the same GPU over
gloo, as tests/helpers/dp_child.py does.  Started fresh; reads RANK / WORLD_SIZE / MASTER_* from the environment.

    python clip_dp_child.py <outdir> <grad_clip>

Also imported by the test for the model / argument builders (`build`), which the single-process reference shares."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, 'bm-nas_amd'), os.path.join(ROOT, 'tests'), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch
import torch.nn as nn

import dp_child as base

STEPS = 2


def build(grad_clip=None, arch_grad_clip=None, use_dataparallel=False):
    """The hypernet of dp_child.run_grads (fusion cell + classifier, identity reshape layers) through search_setup.
    -> model, criterion, optimizer, architect, args"""
    from gpu_util import set_mode
    from oracle import synth
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase, search_setup
    cfg = base.cfg_small()
    args = base.make_args(cfg)
    args.use_dataparallel = use_dataparallel
    if grad_clip is not None:
        args.grad_clip = grad_clip
    if arch_grad_clip is not None:
        args.arch_grad_clip = arch_grad_clip

    class Net(HyperNetBase):
        def __init__(self, criterion):
            super().__init__()
            self._build_head(args, criterion, nn.ModuleList([nn.Identity() for _ in range(cfg.N)]), cfg.N, 2)

        def forward(self, feats):
            return self.fuse(feats)

    crit = bnn.BCEWithLogitsLoss()
    model = Net(crit)
    model.fusion_net.load_state_dict(synth.make_params(cfg, base.SEED))
    for dst, src in zip(model.arch_parameters(), synth.make_arch(cfg, base.SEED, 0.5)):
        dst.data.copy_(src)
    cw, cb = synth.make_classifier(cfg, base.NOUT, base.SEED)
    model.central_classifier.weight.data.copy_(cw)
    model.central_classifier.bias.data.copy_(cb)
    optimizer, _, architect, _ = search_setup(model, args, crit, torch.device('cuda:0'), 1.0, args.weight_decay)
    set_mode(model, 'train_nodrop')
    return model, crit, optimizer, architect, args


def global_batch(device):
    from oracle import synth
    cfg = base.cfg_small()
    X = [x.to(device) for x in synth.make_inputs(cfg, base.GLOBAL_BATCH, base.SEED)]
    Y = synth.make_labels('bce', base.GLOBAL_BATCH, base.NOUT, base.SEED).to(device)
    return X, Y


def weight_names(model):
    return [n for grp in ('reshape_layers', 'fusion_net', 'central_classifier')
            for n, _ in getattr(model, grp).named_parameters(prefix=grp)]


def run(out, grad_clip):
    from bmnas import dist as bdist
    from bmnas.graph import GraphedTrainStep
    model, crit, optimizer, _, args = build(grad_clip=grad_clip, use_dataparallel=True)
    assert optimizer.max_grad_norm == grad_clip
    rank, world = torch.distributed.get_rank(), torch.distributed.get_world_size()
    device = next(model.parameters()).device
    X, Y = global_batch(device)
    xs = [bdist.shard(x, rank, world).contiguous() for x in X]
    y = bdist.shard(Y, rank, world).contiguous()
    wg = GraphedTrainStep(model, crit, optimizer, xs, y)
    assert wg.reducer is not None and wg.reducer.world == 2
    dump = {}
    for it in range(STEPS):
        wg(xs, y)
        dump[f'norm:{it}'] = optimizer.last_grad_norm.detach().cpu().clone()
    torch.cuda.synchronize()
    for n, p_ in model.named_parameters():
        dump['param:' + n] = p_.detach().cpu().clone()
    torch.save(dump, os.path.join(out, f'clip_rank{rank}.pt'))
    torch.distributed.barrier()
    torch.distributed.destroy_process_group()


if __name__ == '__main__':
    run(sys.argv[1], float(sys.argv[2]))
