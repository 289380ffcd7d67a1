"""CPU: which criterion calls run on the gfx950 kernels (bmnas.nn.criterion_route — a decision over
shapes, dtypes, devices and the module's options, so stand-ins that carry just those decide it
without a GPU) and the search drivers' criterion helper (models/search/_common.make_criterion)."""
import types

import pytest
import torch

from bmnas import nn as bnn
from models.search import _common


class T:
    """what criterion_route reads of a tensor"""

    def __init__(self, shape, dtype=torch.float32, device='cuda', contiguous=True):
        self.shape, self.dtype, self.device = tuple(shape), dtype, torch.device(device)
        self._contiguous = contiguous

    def dim(self):
        return len(self.shape)

    def is_contiguous(self):
        return self._contiguous


def _bce(**kw):
    m = bnn.BCEWithLogitsLoss(reduction=kw.pop('reduction', 'mean'))
    # (stand-ins in the buffer slots: Module.__setattr__ takes tensors only)
    m._buffers['weight'], m._buffers['pos_weight'] = kw.pop('weight', None), kw.pop('pos_weight', None)
    assert not kw
    return m


def _ce(**kw):
    m = bnn.CrossEntropyLoss(reduction=kw.pop('reduction', 'mean'), label_smoothing=kw.pop('label_smoothing', 0.0),
                             ignore_index=kw.pop('ignore_index', -100))
    m._buffers['weight'] = kw.pop('weight', None)
    assert not kw
    return m


Z, Y = T((37, 23)), T((37, 23))
ZC, YC = T((64, 60)), T((64,), torch.int64)


@pytest.mark.parametrize('module,plan', [
    (_bce(), 'bare'),
    (_bce(pos_weight=T((23,))), 'crit'),
    (_bce(weight=T((23,))), 'crit'),
    (_bce(weight=T((23,)), pos_weight=T((23,)), reduction='sum'), 'crit'),
    (_bce(reduction='sum'), 'crit'),
])
def test_bce_on_path(module, plan):
    assert bnn.criterion_route(module, Z, Y) == 'native'
    assert bnn._criterion_plan(module, Z, Y) == plan


@pytest.mark.parametrize('module,z,y', [
    (_bce(reduction='none'), Z, Y),
    (_bce(pos_weight=T((22,))), Z, Y),                               # another length
    (_bce(pos_weight=T((37, 23))), Z, Y),                            # torch broadcasts it; the kernels take (O)
    (_bce(weight=T((23,), torch.float64)), Z, Y),
    (_bce(weight=T((23,), device='cpu')), Z, Y),
    (_bce(pos_weight=T((23,), contiguous=False)), Z, Y),
    (_bce(pos_weight=T((23,))), T((37, 23), device='cpu'), T((37, 23), device='cpu')),
    (_bce(), Z, T((37, 23), torch.float64)),
    (_bce(), Z, T((37, 1))),
    (_bce(), T((37, 23), torch.float16), Y),
])
def test_bce_off_path(module, z, y):
    assert bnn.criterion_route(module, z, y) == 'torch'


@pytest.mark.parametrize('module,plan', [
    (_ce(), 'bare'),                                                 # today's kernels, today's numbers
    (_ce(weight=T((60,))), 'crit'),
    (_ce(label_smoothing=0.1), 'crit'),
    (_ce(ignore_index=7), 'crit'),
    (_ce(ignore_index=-1), 'crit'),
    (_ce(reduction='sum'), 'crit'),
    (_ce(weight=T((60,)), label_smoothing=0.1, ignore_index=0, reduction='sum'), 'crit'),
])
def test_ce_on_path(module, plan):
    assert bnn.criterion_route(module, ZC, YC) == 'native'
    assert bnn._criterion_plan(module, ZC, YC) == plan


@pytest.mark.parametrize('module,z,y', [
    (_ce(reduction='none'), ZC, YC),
    (_ce(label_smoothing=0.1), ZC, T((64, 60))),                     # probability targets
    (_ce(weight=T((59,))), ZC, YC),
    (_ce(weight=T((60,), torch.float16)), ZC, YC),
    (_ce(weight=T((60,), device='cpu')), ZC, YC),
    (_ce(label_smoothing=1.0), ZC, YC),
    (_ce(), T((64, 60), device='cpu'), T((64,), torch.int64, device='cpu')),
    (_ce(), T((4, 60, 8)), T((4, 8), torch.int64)),                  # the (N, C, d1) form
    (_ce(), ZC, T((64,), torch.int32)),
    (_ce(label_smoothing=0.1), ZC, T((63,), torch.int64)),           # another batch size
])
def test_ce_off_path(module, z, y):
    assert bnn.criterion_route(module, z, y) == 'torch'


def test_bare_route_keeps_its_earlier_conditions():
    """What took the bare mean kernels before the options existed still does: the weighted route's extra conditions
    (targets on the device, at least one dimension) are not asked of it."""
    assert bnn._criterion_plan(_bce(), Z, T((37, 23), device='cpu')) == 'bare'
    assert bnn._criterion_plan(_bce(), T(()), T(())) == 'bare'
    assert bnn._criterion_plan(_ce(), ZC, T((64,), torch.int64, device='cpu')) == 'bare'
    assert bnn._criterion_plan(_bce(pos_weight=T((23,))), Z, T((37, 23), device='cpu')) is None


def test_route_on_real_cpu_tensors_is_torch():
    m = bnn.BCEWithLogitsLoss(pos_weight=torch.ones(3))
    assert bnn.criterion_route(m, torch.zeros(2, 3), torch.zeros(2, 3)) == 'torch'
    m = bnn.CrossEntropyLoss(label_smoothing=0.1)
    assert bnn.criterion_route(m, torch.zeros(2, 3), torch.zeros(2, dtype=torch.int64)) == 'torch'


def test_descriptor_carries_options_and_addresses():
    from bmnas import lib
    c = lib.Criterion('ce', label_smoothing=0.1, ignore_index=-1, reduction='sum')
    d = c.desc()
    assert (d.weight, d.pos_weight, d.ignore_index, d.reduction) == (None, None, -1, 1)
    assert abs(d.label_smoothing - 0.1) < 1e-7 and c.code == lib.CRIT_CE
    assert lib.Criterion('bce').code == lib.CRIT_BCE and lib.Criterion('bce').desc().reduction == 0


def _args(**kw):
    return types.SimpleNamespace(num_outputs=kw.pop('num_outputs', 4), **kw)


def test_make_criterion_without_optional_args_is_the_reference_criterion():
    bce = _common.make_criterion('bce', _args())
    assert type(bce) is bnn.BCEWithLogitsLoss and bce.weight is None and bce.pos_weight is None
    assert bce.reduction == 'mean' and not bce.state_dict()
    ce = _common.make_criterion('ce', _args())
    assert type(ce) is bnn.CrossEntropyLoss and ce.weight is None and ce.label_smoothing == 0.0
    assert ce.reduction == 'mean' and ce.ignore_index == -100 and not ce.state_dict()
    assert bnn._criterion_plan(bce, Z, Y) == 'bare' and bnn._criterion_plan(ce, ZC, YC) == 'bare'


def test_make_criterion_reads_the_optional_args():
    bce = _common.make_criterion('bce', _args(pos_weight=[1, 2, 3, 4], class_weight=(0.5, 1, 1, 2)))
    assert bce.pos_weight.dtype == torch.float32 and bce.pos_weight.tolist() == [1, 2, 3, 4]
    assert bce.weight.tolist() == [0.5, 1, 1, 2]
    assert set(bce.state_dict()) == {'weight', 'pos_weight'}        # buffers: they move with model.to(device)
    ce = _common.make_criterion('ce', _args(class_weight=[1, 2, 3, 4], label_smoothing=0.1, pos_weight=[9] * 4))
    assert ce.weight.tolist() == [1, 2, 3, 4] and ce.label_smoothing == 0.1 and not hasattr(ce, 'pos_weight')
    with pytest.raises(ValueError, match='4 outputs'):
        _common.make_criterion('bce', _args(pos_weight=[1, 2, 3]))
    with pytest.raises(ValueError):
        _common.make_criterion('mse', _args())
