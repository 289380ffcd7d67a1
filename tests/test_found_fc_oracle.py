"""CPU: the restatement of a found cell with fc_relu / fc_mish edges (tests/found_fc_util.py: its own step loop over
fo.found_node_cell with the oracle's FC op) against the reference's own outputs, tests/golden/fcfound_*.npz written by
tests/golden/make_golden_r11_found_fc.py.  Everything the GPU tests compare the kernels with rests on this."""
import numpy as np
import pytest
import torch

import found_fc_util as fu
from gpu_util import assert_close_scaled
from oracle import fusion_oracle as fo
from oracle import synth
from util import case_id

FILES = fu.fixture_files()


def test_the_fixture_set_is_complete():
    want = sorted(f'fcfound_{g}_{s}_{m}' for g, s in fu.CASES for m in ('eval', 'train_nodrop'))
    assert [case_id(p) for p in FILES] == want


@pytest.mark.parametrize('path', FILES, ids=case_id)
def test_restatement_matches_the_reference(path):
    meta, z = fu.load(path)
    cfg = fo.Cfg(meta['cfg'])
    g = fo.genotype_from_jsonable(meta['genotype'])
    seed = meta['seed']
    params = synth.make_params(cfg, seed, fu.found_fc_param_shapes(cfg, g))
    xs = [torch.from_numpy(z[f'input.{i}']) for i in range(cfg.N)]
    for a, b in zip(xs, synth.make_inputs(cfg, meta['batch'], seed)):
        assert torch.equal(a, b)
    if meta['has_grads']:
        feat, grads, after, _ = fu.restate(cfg, g, params, xs, meta['mode'], seed)
    else:
        # (eval with node_multiplier != 1: the reference itself runs this combination forward-only)
        with torch.no_grad():
            after = {k: v.clone() for k, v in params.items()}
            feat = fu.found_fc_cell(xs, g, after, cfg, False)
        grads = {}
    assert_close_scaled('feat', feat, z['feat'])
    zero = fu.roundoff_zero_gradients(cfg, g, params, xs, meta['mode'], seed) if meta['has_grads'] else set()
    for k in zero:
        assert float(np.abs(z[k]).max()) < 1e-5, k                  # round-off in the reference's own output too
    seen = 0
    for k in z.files:
        if k.startswith('grad:'):
            seen += 1
            fu.assert_gradient(k, grads[k], z[k], zero, meta['mode'], assert_close_scaled)
        elif k.startswith('buf:'):
            assert_close_scaled(k, after[k[4:]].float(), z[k])
    assert (seen > 0) == meta['has_grads']
    assert seen == (len(grads) if meta['has_grads'] else 0)
