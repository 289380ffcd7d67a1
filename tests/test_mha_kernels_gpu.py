"""-m gpu: the multi-head attention core kernels (csrc/mha.hip: bmnas_mha_core_fwd / bmnas_mha_core_bwd) through the C
ABI against the float64 statement in tests/mha_ref.py (itself pinned by tests/test_mha_ref.py).

Every shape of mha_ref.KERNEL_TABLE — d = 4 with the smallest L and a ragged last tile, d = 24 (not a multiple of the
16-channel chunk), one and eight heads, the two flagship shapes, the largest d — runs with q / k / v as rows of one
(b, 3C, L) buffer and as three separate buffers (sample strides 3 C L and C L; the gradients likewise), with dropout
off and on.  With dropout on the multipliers are exported with lib.dropout_mask and handed to the reference.  The
backward is fed the reference's P, so it is judged on its own.  Output buffers start as NaN between guards
(gpu_util.Pool): nothing may be left unwritten, nothing written outside.  Each case prints its worst
err / (|want| + max|want|) per tensor (pytest -s).  Tolerances are the project's: 1e-4 forward, 2e-4 gradients."""
import functools

import numpy as np
import pytest
import torch

import mha_ref as mr
from gpu_util import Pool, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

FWD_REL, BWD_REL = 1e-4, 2e-4


def _drop(on):
    from bmnas import lib
    return lib.make_dropout(mr.DROP_P, mr.DROP_SEED, mr.DROP_OFFSET) if on else lib.NO_DROP


@functools.lru_cache(maxsize=None)
def _case(C, heads, L, b, drop_on):
    """(fp32 inputs, float64 reference under the exported multipliers) of one case; shared, never written."""
    from bmnas import lib
    t = mr.make_core_inputs(C, heads, L, b)
    mask = None
    if drop_on:
        mask = lib.dropout_mask(_drop(True), b * heads * L * L, dev()).cpu()
        kept = float((mask > 0).float().mean())
        # 1 - p = 0.75; the smallest site has 256 elements (sigma 0.027)
        assert 0.63 < kept < 0.87, kept
        assert set(np.unique(mask.numpy())) <= {np.float32(0.0), np.float32(1.0 / (1.0 - mr.DROP_P))}
        mask = mask.view(b, heads, L, L)
    return t, mr.core_ref(t['Q'], t['K'], t['V'], heads, t['dO'], mask)


def _operands(t, stacked):
    """q, k, v on the device: rows of one (b, 3C, L) tensor, or three tensors."""
    if stacked:
        U = torch.cat([t['Q'], t['K'], t['V']], 1).to(dev())
        C = t['Q'].shape[1]
        return U[:, :C], U[:, C:2 * C], U[:, 2 * C:]
    return t['Q'].to(dev()), t['K'].to(dev()), t['V'].to(dev())


@pytest.mark.parametrize('drop_on', [False, True], ids=['nodrop', 'drop'])
@pytest.mark.parametrize('stacked', [True, False], ids=['stacked', 'separate'])
@pytest.mark.parametrize('C,heads,L,b', mr.KERNEL_TABLE)
def test_mha_core_fwd_bwd(C, heads, L, b, stacked, drop_on):
    from bmnas import lib
    assert lib.mha_ok(b, C, L, heads)
    t, ref = _case(C, heads, L, b, drop_on)
    q, k, v = _operands(t, stacked)
    pool = Pool()
    O, P = pool.new(b, C, L), pool.new(b, heads, L, L)
    lib.mha_core_fwd(q, k, v, O, P, b, C, L, heads, _drop(drop_on))
    if stacked:
        dU = pool.new(b, 3 * C, L)
        dq, dk, dv = dU[:, :C], dU[:, C:2 * C], dU[:, 2 * C:]
    else:
        dq, dk, dv = pool.new(b, C, L), pool.new(b, C, L), pool.new(b, C, L)
    lib.mha_core_bwd(t['dO'].to(dev()), q, k, v, ref['P'].float().to(dev()), dq, dk, dv, b, C, L, heads,
                     _drop(drop_on))
    pool.check()
    got = {'O': O, 'P': P, 'dQ': dq, 'dK': dk, 'dV': dv}
    case = f'C={C} h={heads} L={L} b={b} {"stacked" if stacked else "separate"} drop={int(drop_on)}'
    print(f'[{case}] worst err / (|want| + max|want|): ' +
          ', '.join(f'{n} {mr.rel_err(g, ref[n]):.2e}' for n, g in got.items()))
    for n, g in got.items():
        assert_close_scaled(f'{case} {n}', g.contiguous(), ref[n], rel=FWD_REL if n in ('O', 'P') else BWD_REL)


@pytest.mark.parametrize('b,C,L,heads', [(2, 1024, 8, 2), (2, 64, 32, 2), (2, 48, 8, 5), (2, 16, 8, 8), (2, 40, 8, 2)],
                         ids=['C>512', 'L=32', 'heads does not divide C', 'd=2', 'C%16'])
def test_refused_shape_returns_limit_and_writes_nothing(b, C, L, heads):
    from bmnas import lib
    assert not lib.mha_ok(b, C, L, heads)
    n = b * C * L
    x = torch.zeros(3 * n, device=dev())
    bufs = [torch.full((max(n, b * heads * L * L),), float('nan'), device=dev()) for _ in range(5)]
    so = lib.load()
    st = torch.cuda.current_stream().cuda_stream
    p = lambda i: x.data_ptr() + 4 * n * i
    rc = so.bmnas_mha_core_fwd(p(0), p(1), p(2), C * L, C * L, C * L, bufs[0].data_ptr(), bufs[1].data_ptr(), b, C, L,
                               heads, lib.NO_DROP, st)
    assert rc == -3                                               # BMNAS_E_LIMIT
    rc = so.bmnas_mha_core_bwd(p(0), p(0), p(1), p(2), C * L, C * L, C * L, x.data_ptr(), bufs[2].data_ptr(),
                               bufs[3].data_ptr(), bufs[4].data_ptr(), C * L, C * L, C * L, b, C, L, heads,
                               lib.NO_DROP, st)
    assert rc == -3
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in bufs)
    with pytest.raises(lib.BmnasError, match='limit exceeded'):
        lib.mha_core_fwd(x[:n].view(b, C, L), x[:n].view(b, C, L), x[:n].view(b, C, L), bufs[0][:n].view(b, C, L),
                         bufs[1][:b * heads * L * L].view(b, heads, L, L), b, C, L, heads, lib.NO_DROP)
