"""CPU self-check of tests/attention_ref.py: the inputs tests/test_attention_channels_gpu.py feeds the attention
kernels are well conditioned, i.e. the reference evaluated in float32 agrees with its float64 evaluation to one
tenth of the bound the GPU test applies.  A GPU mismatch at those bounds is then the kernel's, not the reference's."""
import numpy as np
import torch

import attention_ref as ar
from gpu_util import assert_close_scaled
from oracle import philox

# one tenth of the GPU test's bounds (rel 1e-4 forward, 2e-4 gradients; absolute floor 1e-6)
FWD_REL, BWD_REL, FLOOR = 1e-5, 2e-5, 1e-7


def test_reference_is_well_conditioned():
    seen, worst = set(), {}
    for C, b, L, mode, have_gs, drop in ar.TABLE_A:
        same = mode.startswith('same')
        key = (C, b, L, same, drop)
        if key in seen:
            continue
        seen.add(key)
        t = ar.make_inputs(C, b, L, same)
        mask = None
        if drop:
            mask = torch.from_numpy(philox.dropout_multipliers(ar.DROP_P, ar.DROP_SEED, ar.DROP_OFFSET, b * C * L))
            assert 0.6 < float((mask > 0).float().mean()) < 0.9
        args = (t['x'], t['y'], t['ln_w'], t['ln_b'], t['g'], mask, ar.GSCALE, same)
        r64 = ar.attention_ref(*args, dtype=torch.float64)
        r32 = ar.attention_ref(*args, dtype=torch.float32)
        assert float(r64['stats'][:, 0].abs().min()) > 0.05          # the DC offset reaches the LayerNorm mean
        for name in ('out', 'xhat', 'stats', 'dx', 'dy'):
            if r64[name] is None:
                assert same and r32[name] is None
                continue
            assert r32[name].dtype == torch.float32 and r64[name].dtype == torch.float64
            w = r64[name].numpy()
            err = np.abs(r32[name].double().numpy() - w) / (np.abs(w) + np.abs(w).max())
            worst[name] = max(worst.get(name, 0.0), float(err.max()))
            assert_close_scaled(f'{name} {key}', r32[name], r64[name],
                                rel=FWD_REL if name in ('out', 'xhat', 'stats') else BWD_REL, floor=FLOOR)
    print('worst fp32-vs-fp64 error in units of |want| + max|want|:', worst)
    assert len(seen) >= 24
