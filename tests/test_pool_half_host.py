"""CPU: the host side of the bf16 / fp16 feature maps in the reshape layers' pooling — the layout of
bmnas_pool_prob_ex_t, which features aux.reshape_all sends through the grouped pooling launch, the drivers'
args.backbone_dtype, and a half feature off the device (computed instead of refused)."""
import ctypes
import os
import re
import types

import pytest
import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'bmnas_hip.h')


def _header_struct(name):
    """[(field, size)] of a typedef struct of pointers and ints, in declaration order"""
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    body = re.search(r'typedef struct \{([^}]*)\} ' + name + ';', text).group(1)
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(';'))):
        if '*' in decl:
            fields.append((decl.split('*')[-1].strip(), 8))
        else:
            assert decl.startswith('int '), decl
            fields += [(f.strip(), 4) for f in decl[4:].split(',')]
    return fields


def test_pool_prob_ex_layout_matches_the_header():
    from bmnas import lib
    fields = _header_struct('bmnas_pool_prob_ex_t')
    assert [f for f, _ in fields] == ['x', 'out', 'idx', 'g', 'dx', 'C', 'H', 'W', 'oh', 'ow', 'dtype']
    assert [f for f, _ in lib.PoolProbEx._fields_] == [f for f, _ in fields]
    off = 0
    for name, size in fields:
        off = (off + size - 1) // size * size                       # natural alignment
        assert getattr(lib.PoolProbEx, name).offset == off and getattr(lib.PoolProbEx, name).size == size, name
        off += size
    assert ctypes.sizeof(lib.PoolProbEx) == (off + 7) // 8 * 8 == 64
    # the untyped descriptor is the same without the type code, and a zeroed one is an fp32 problem
    assert [f for f, _ in _header_struct('bmnas_pool_prob_t')] == [f for f, _ in fields][:-1]
    assert lib.PoolProbEx().dtype == lib.DT_F32 == 0 and (lib.DT_BF16, lib.DT_F16) == (1, 2)
    text = open(HEADER).read()
    for name, code in (('F32', 0), ('BF16', 1), ('F16', 2)):
        assert re.search(rf'#define BMNAS_DT_{name} {code}\b', text)
    assert lib.POOL_DTYPES == {torch.float32: 0, torch.bfloat16: 1, torch.float16: 2}


def test_ex_entry_points_are_bound():
    from bmnas import lib
    for name in ('bmnas_adaptive_maxpool_fwd_group_ex', 'bmnas_adaptive_maxpool_bwd_group_ex'):
        argtypes, restype = lib.SIGNATURES[name]
        assert argtypes[0] == ctypes.POINTER(lib.PoolProbEx) and len(argtypes) == 4 and restype is ctypes.c_int
        assert hasattr(lib.load(), name)
    assert 'bmnas_adaptive_maxpool_fwd_group_ex' in open(os.path.join(ROOT, 'INTEGRATION.md')).read()


class _A:
    drpt = 0.0


def _layers(n, cls=None):
    import models.auxiliary.aux_models as aux
    return [(cls or aux.ReshapeInputLayer_MMIMDB)(16, 16, 16, _A()) for _ in range(n)]


def _meta(dtype, b=2, shape=(16, 4, 4)):
    return torch.empty((b,) + shape, dtype=dtype, device='meta')


def test_reshape_all_routing_decisions():
    """pool_groups on meta tensors, decided as if they lay on the device: nothing is launched"""
    import models.auxiliary.aux_models as aux
    from bmnas import lib
    f32, bf, fp = torch.float32, torch.bfloat16, torch.float16
    groups = lambda feats, layers=None: aux.pool_groups(layers or _layers(len(feats)), feats, on_device=True)
    # fp32 alone: today's rule — two or more with one batch size, else the torch pool
    assert groups([_meta(f32), _meta(f32), _meta(f32)]) == [[0, 1, 2]]
    assert groups([_meta(f32)]) == []
    assert groups([_meta(f32), _meta(f32, b=3)]) == []
    assert groups([_meta(f32), _meta(torch.float64)]) == []
    # a half feature always goes through the launch: mixed with fp32 in one group, or alone
    assert groups([_meta(bf), _meta(f32), _meta(fp), _meta(bf)]) == [[0, 1, 2, 3]]
    assert groups([_meta(bf)]) == [[0]]
    assert groups([_meta(fp), _meta(torch.float64), _meta(torch.int32)]) == [[0]]
    assert groups([_meta(f32), _meta(bf, b=3)]) == [[1]]                   # (the fp32 one stays on the torch pool)
    assert groups([_meta(bf), _meta(fp, b=3), _meta(bf)]) == [[0, 2], [1]]
    # placeholders of a found net and empty tensors are left out; more than MAX_GROUP members split
    assert groups([_meta(bf), _meta(bf)], [_layers(1)[0], nn.ReLU()]) == [[0]]
    assert groups([_meta(bf, b=0), _meta(f32)]) == []
    n = lib.MAX_GROUP + 1
    assert groups([_meta(bf)] * n) == [list(range(lib.MAX_GROUP)), [lib.MAX_GROUP]]
    # off the device nothing is eligible, half or not
    assert aux.pool_groups(_layers(2), [torch.zeros(2, 16, 4, 4, dtype=bf), torch.zeros(2, 16, 4, 4)]) == []
    assert aux.pool_groups(_layers(2), [_meta(bf), _meta(bf)]) == []


def test_backbone_dtype_option():
    from bmnas.lib import BmnasError
    from models.search import _common as c
    ns = types.SimpleNamespace
    assert c.backbone_dtype_option(ns()) is None and c.backbone_dtype_option(ns(backbone_dtype=None)) is None
    assert c.backbone_dtype_option(ns(backbone_dtype='bf16')) is torch.bfloat16
    assert c.backbone_dtype_option(ns(backbone_dtype='fp16')) is torch.float16
    for bad in ('fp32', 'bfloat16', torch.bfloat16, 16, ''):
        with pytest.raises(BmnasError, match='backbone_dtype'):
            c.backbone_dtype_option(ns(backbone_dtype=bad))


class _Args:
    C, L, drpt, num_input_nodes, node_steps, node_multiplier = 16, 8, 0.1, 3, 1, 1
    steps, multiplier, num_outputs, parallel, num_keep_edges = 2, 2, 5, False, 2


def _net(**kw):
    import models.auxiliary.aux_models as aux
    from models.search._common import HyperNetBase

    class Net(HyperNetBase):
        def __init__(self, args):
            super().__init__()
            self._build_head(args, None, self.make_reshape_layers(aux.ReshapeInputLayer, [16, 16, 16], args), 3, 2)

    args = _Args()
    for k, v in kw.items():
        setattr(args, k, v)
    return Net(args)


def test_backbone_dtype_is_checked_when_the_model_is_built():
    import contextlib
    from bmnas.lib import BmnasError
    assert isinstance(_net().backbone_autocast(), contextlib.nullcontext)
    assert isinstance(_net(backbone_dtype=None).backbone_autocast(), contextlib.nullcontext)
    with pytest.raises(BmnasError, match="'bf16', 'fp16'"):
        _net(backbone_dtype='half')
    net = _net(backbone_dtype='bf16')
    conv = nn.Conv1d(4, 4, 1)
    x = torch.randn(2, 4, 8)
    with net.backbone_autocast():
        assert conv(x).dtype == torch.bfloat16
    assert conv(x).dtype == torch.float32


@pytest.mark.parametrize('dtype', [torch.bfloat16, torch.float16], ids=str)
@pytest.mark.parametrize('kind', ['video', 'mmimdb'])
def test_half_cpu_feature_computes(kind, dtype):
    """a half feature off the device takes the torch pool and widens in front of the conv: the result is the layer's
    on the widened feature, bit for bit (max pooling selects, the widening is exact) — it used to be a TypeError on the
    device and a dtype mismatch in the conv here"""
    import models.auxiliary.aux_models as aux
    import pool_ref
    torch.manual_seed(3)
    cls, L, shape = (aux.ReshapeInputLayer, 8, (2, 16, 13, 3, 3)) if kind == 'video' else \
        (aux.ReshapeInputLayer_MMIMDB, 16, (2, 16, 5, 8))
    layer = cls(16, 16, L, _A()).eval()
    x = pool_ref.make_input((2, 16, shape[2], shape[3] * (shape[4] if len(shape) > 4 else 1)), 4, 1, dtype, 9,
                            several_nans=False).nan_to_num(0.0).view(shape)
    want = layer(x.float())
    got = layer(x)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    both = aux.reshape_all([layer, layer], [x, x.float()])
    assert torch.equal(both[0], want) and torch.equal(both[1], want)
    assert torch.equal(aux.reshape_tails([layer], [layer.pooled(x)])[0], want)
