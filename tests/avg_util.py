"""Shared by tests/test_avg_gpu.py and tests/test_avg_loop_gpu.py: the small MM-IMDB hypernet tests/test_sgd_loop_gpu.py
builds (dp_child.run_grads' fusion cell + classifier, C = 32, batch 8, through search_setup), its batch, and the walk
that turns a module's tensors into the numpy lists tests/avg_ref.py averages."""
import os
import sys

import torch
import torch.nn as nn

from gpu_util import dev, set_mode

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), 'helpers'))


def build(**extra):
    """-> model, criterion, optimizer, args (train mode, dropout off)"""
    import dp_child as base
    from oracle import synth
    from bmnas import nn as bnn
    from models.search._common import HyperNetBase, search_setup
    cfg = base.cfg_small()
    args = base.make_args(cfg)
    args.use_dataparallel = False
    for k, v in extra.items():
        setattr(args, k, v)

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
    optimizer, _, _, _ = search_setup(model, args, crit, dev(), 1.0, args.weight_decay)
    set_mode(model, 'train_nodrop')
    return model, crit, optimizer, args


def batch():
    import dp_child as base
    from oracle import synth
    cfg = base.cfg_small()
    xs = [x.to(dev()) for x in synth.make_inputs(cfg, base.GLOBAL_BATCH, base.SEED)]
    return xs, synth.make_labels('bce', base.GLOBAL_BATCH, base.NOUT, base.SEED).to(dev())


def tensors(module):
    """parameters, then buffers, as numpy arrays (the order torch's AveragedModel walks with use_buffers=True)"""
    torch.cuda.synchronize()
    return [t.detach().cpu().numpy().copy() for t in list(module.parameters()) + list(module.buffers())]


def same_bits(got, want):
    """-> the indices at which two lists of arrays differ in any bit"""
    bad = []
    for i, (a, b) in enumerate(zip(got, want)):
        if a.dtype != b.dtype or a.shape != b.shape or a.tobytes() != b.tobytes():
            bad.append(i)
    return bad
