"""CPU: the oracle reproduces the reference's outputs for the edited PRIMITIVES list at the production sizes
(tests/golden/fcedge_*.npz, summary form; written by tests/golden/make_golden_r07_prims.py from the reference itself),
and the rule that decides which primitives of a list a weight row reaches."""
import json

import pytest
import torch

from oracle import fusion_oracle as fo
from oracle import synth
from util import (assert_close, assert_summary_close, case_id, cfg_of, golden_files, grad_atol, load_npz, mode_flags)

TOL = dict(rtol=2e-5, atol=2e-6)     # as tests/test_oracle_golden.py: same aten ops, fp32 reassociation only


def test_participating_primitives_rule():
    from models.search.darts.genotypes import STEP_EDGE_PRIMITIVES
    from models.search.darts.operations import participating_primitives
    full = ['none', 'fc_relu', 'fc_mish', 'skip']
    assert participating_primitives(full, len(STEP_EDGE_PRIMITIVES)) == ['none', 'fc_relu']
    assert participating_primitives(full, 4) == full
    assert participating_primitives(['skip', 'fc_mish', 'none'], 2) == ['skip', 'fc_mish']
    assert participating_primitives(['none', 'skip', 'fc_relu'], 2) == ['none', 'skip']
    assert participating_primitives(['none', 'skip'], 4) == ['none', 'skip']        # a row longer than the list
    got = participating_primitives(full, 2)
    got.append('x')
    assert full == ['none', 'fc_relu', 'fc_mish', 'skip']                           # a copy, not a view of the registry


def test_fixture_set_is_complete():
    names = [case_id(p) for p in golden_files('fcedge_*.npz')]
    assert names == ['fcedge_mm_eval', 'fcedge_mm_train_nodrop', 'fcedge_nt_eval', 'fcedge_nt_train_nodrop']


@pytest.mark.parametrize('path', golden_files('fcedge_*.npz'), ids=case_id)
def test_oracle_matches_reference_at_production_size(path):
    meta, z = load_npz(path)
    cfg = cfg_of(meta)
    prims = meta['primitives']
    training, drpt, attn_drop = mode_flags(meta['mode'])
    if drpt is not None:
        cfg = fo.Cfg({**cfg, 'drpt': drpt})
    seed, batch, nout = meta['seed'], meta['batch'], meta['num_outputs']
    p = synth.make_params(cfg, seed, fo.param_shapes(cfg, prims))
    arch = synth.make_arch(cfg, seed, 0.5, prims)
    xs = synth.make_inputs(cfg, batch, seed)
    cw, cb = synth.make_classifier(cfg, nout, seed)
    y = synth.make_labels(meta['loss'], batch, nout, seed)
    if meta['has_grads']:
        logits, loss, grads = fo.search_step(xs, y, arch, p, cw, cb, cfg, meta['loss'], training=training,
                                             attn_drop=attn_drop, primitives=prims)
    else:
        with torch.no_grad():
            logits = fo.hypernet_logits(xs, arch, p, cw, cb, cfg, training, attn_drop, prims)
            loss = fo.loss_fn(meta['loss'])(logits, y)
        grads = {}
    assert_close('logits', logits, z['logits'], **TOL)
    assert_close('loss', loss, z['loss'], **TOL)
    for k in z.files:
        if k.startswith('grad:'):
            name = k[5:]
            g = grads[name]
            if name.startswith('arch.'):
                assert_close(k, g, z[k], rtol=1e-4, atol=grad_atol(k, 2e-6))
            else:
                g = g if g is not None else torch.zeros(1)
                if (name.endswith('conv.bias')) and training:
                    assert float(g.abs().max()) < 1e-4, k          # mathematically zero, round-off in both
                else:
                    assert_summary_close(k, g, z[k])
        elif k.startswith('buf:'):
            if p[k[4:]].dim() == 0:
                assert_close(k, p[k[4:]], z[k], **TOL)
            else:
                assert_summary_close(k, p[k[4:]], z[k])
    assert fo.genotype_to_jsonable(fo.network_genotype(arch, cfg, prims)) == json.loads(str(z['genotype']))
