"""-m gpu: the C ABI of the selected-term mix with an activation argument (bmnas_node_mix_sel_act_fwd / _bwd,
csrc/nodemix_sel.hip) beyond what tests/test_cat_conv_mish_gpu.py holds: the backward entry point's refusal of an
unknown activation, `fc_act` without an FC slot in the list (nothing to activate: Mish and ReLU are the same launch),
and the legacy entry points bmnas_node_mix_sel_fwd / _bwd, which lib's wrappers no longer go through, against the new
ones with ReLU.  ['Sum'] needs no conv rows, no attention output and no BatchNorm: every buffer is (b, C, L)."""
import numpy as np
import pytest
import torch

from gpu_util import assert_close_scaled, dev

pytestmark = pytest.mark.gpu

B, C, L = 5, 16, 8


def _case(seed=11):
    rng = np.random.Generator(np.random.PCG64(seed))
    r = lambda: torch.from_numpy(rng.standard_normal((B, C, L)).astype(np.float32)).to(dev())
    return r(), r(), r(), torch.tensor([0.75], device=dev())


def _fwd(lib, x, y, w, sel, fc_act):
    out = torch.full_like(x, 7.0)
    lib.node_mix_sel_fwd(x, y, None, None, None, w, sel, out, B, C, L, fc_act=fc_act)
    return out


def _bwd(lib, g, x, y, w, sel, fc_act):
    dw, dx, dy = torch.zeros(1, device=dev()), torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    lib.node_mix_sel_bwd(g, x, y, None, None, None, w, sel, dw, dx, dy, 0, None, None, B, C, L, fc_act=fc_act)
    return dw, dx, dy


def test_backward_refuses_an_unknown_activation():
    from bmnas import lib
    x, y, g, w = _case()
    before = dict(lib.NODE_SEL_LAUNCHES)
    with pytest.raises(lib.BmnasError, match='bad argument'):
        _bwd(lib, g, x, y, w, lib.make_node_sel(['Sum']), 2)
    with pytest.raises(lib.BmnasError, match='bad argument'):
        _bwd(lib, g, x, y, w, lib.make_node_sel(['Sum']), -1)
    torch.cuda.synchronize()
    assert lib.NODE_SEL_LAUNCHES == before


def test_activation_is_ignored_without_the_fc_slot():
    from bmnas import lib
    x, y, g, w = _case()
    sel = lib.make_node_sel(['Sum'])
    o0, o1 = _fwd(lib, x, y, w, sel, lib.FC_ACT_RELU), _fwd(lib, x, y, w, sel, lib.FC_ACT_MISH)
    b0, b1 = _bwd(lib, g, x, y, w, sel, lib.FC_ACT_RELU), _bwd(lib, g, x, y, w, sel, lib.FC_ACT_MISH)
    torch.cuda.synchronize()
    assert torch.equal(o0, o1)
    assert_close_scaled('out', o1, 0.75 * (x + y))
    assert_close_scaled('dgamma', b1[0], (g * (x + y)).sum().reshape(1), rel=2e-4)
    assert_close_scaled('dgamma', b0[0], (g * (x + y)).sum().reshape(1), rel=2e-4)       # (atomics: not bit for bit)
    for a, b_ in zip(b0[1:], b1[1:]):
        assert torch.equal(a, b_)
        assert_close_scaled('dx', a, 0.75 * g, rel=2e-4)


def test_legacy_entry_points_are_the_relu_ones():
    """bmnas_node_mix_sel_fwd / _bwd keep their signatures and call the new entry points with ReLU."""
    from bmnas import lib
    x, y, g, w = _case()
    sel = lib.make_node_sel(['Sum'])
    so = lib._stream()
    out = torch.full_like(x, 7.0)
    lib._check(lib.load().bmnas_node_mix_sel_fwd(lib._ptr(x), lib._ptr(y), None, None, None, lib.NO_FIN, w.data_ptr(),
                                                 sel, lib._ptr(out), B, C, L, lib.NO_DROP, lib.NO_DROP, so), 'legacy fwd')
    dw, dx, dy = torch.zeros(1, device=dev()), torch.full_like(x, 7.0), torch.full_like(x, 7.0)
    lib._check(lib.load().bmnas_node_mix_sel_bwd(lib._ptr(g), lib._ptr(x), lib._ptr(y), None, None, None, w.data_ptr(),
                                                 sel, dw.data_ptr(), 1, 0, lib._ptr(dx), lib._ptr(dy), 0, None, None,
                                                 B, C, L, lib.NO_DROP, lib.NO_DROP, so), 'legacy bwd')
    torch.cuda.synchronize()
    assert torch.equal(out, _fwd(lib, x, y, w, sel, lib.FC_ACT_RELU))
    ref = _bwd(lib, g, x, y, w, sel, lib.FC_ACT_RELU)
    assert torch.equal(dx, ref[1]) and torch.equal(dy, ref[2])
    assert_close_scaled('dgamma', dw, ref[0], rel=2e-4)
