"""CPU: the host logic that puts the fc_relu / fc_mish edges of a found network on the grouped kernels — the route
(operations.found_fc_route), the grouping of Found_FusionCell (group 0 in front of the step loop, late edges right
before their step), the state_dict layout, and the fixtures' distance from the ReLU kink.  No kernel runs."""
import types

import pytest
import torch

import found_fc_util as fu
from oracle import fusion_oracle as fo
from test_node_prims_host import fake, on_fake_device
from util import case_id

C, L, B = 16, 8, 4


class A:
    drpt = 0.1


@pytest.fixture(scope='module', autouse=True)
def library():
    from bmnas import build
    build.build()


def fc(kind, C_=C):
    from models.search.darts import operations as ops
    return on_fake_device(getattr(ops, kind)(C_, L, A()))


def route(mods, xs=None):
    from models.search.darts.operations import found_fc_route
    return found_fc_route(mods, [fake(B, C, L) for _ in mods] if xs is None else xs)


def test_builtin_modules_route_fc():
    assert route([fc('FC_Relu')]) == 'fc'
    assert route([fc('FC_Relu'), fc('FC_Mish'), fc('FC_Mish'), fc('FC_Relu')]) == 'fc'
    mods = [fc('FC_Mish'), fc('FC_Relu')]
    for m in mods:
        m.eval()
    assert route(mods) == 'fc'
    x = fake(B, C, L)
    assert route(mods, [x, x]) == 'fc'                      # a shared source


def test_everything_else_routes_composed():
    from models.search.darts import operations as ops
    two = lambda: [fc('FC_Relu'), fc('FC_Mish')]
    assert route(two(), [torch.zeros(B, C, L)] * 2) == 'composed'                   # CPU tensors
    assert route(two(), [fake(B, C, L), torch.zeros(B, C, L)]) == 'composed'
    assert route(two(), [fake(B, C, L).double(), fake(B, C, L).double()]) == 'composed'
    assert route(two(), [fake(B, C, L), fake(B + 1, C, L)]) == 'composed'           # not one shape
    assert route(two(), [fake(B, C * L), fake(B, C * L)]) == 'composed'             # not 3-D
    assert route([fc('FC_Relu', 24)], [fake(B, 24, L)]) == 'composed'               # C = 24
    assert route([fc('FC_Relu')], [fake(B, C, 32)]) == 'composed'                   # L = 32
    assert route([fc('FC_Relu')] * 16) == 'composed'                                # more edges than a launch takes
    assert route([]) == 'composed'

    class Mine(ops.FC_Relu):
        pass
    assert route([fc('FC_Mish'), on_fake_device(Mine(C, L, A()))]) == 'composed'    # a subclassed module
    mods = two()
    mods[1].eval()
    assert route(mods) == 'composed'                                                # mixed train / eval
    mods = two()
    mods[0].bn.eval()
    assert route(mods) == 'composed'                                                # a module out of step with itself
    mods = two()
    mods[0].dropout.eval()
    assert route(mods) == 'composed'
    mods = two()
    mods[1].dropout.p = 0.3
    assert route(mods) == 'composed'                                                # unequal dropout.p
    for change in (dict(momentum=0.2), dict(eps=1e-3), dict(affine=False), dict(track_running_stats=False)):
        mods = two()
        mods[0].bn = torch.nn.BatchNorm1d(C, **change)
        assert route(mods) == 'composed', change                                    # a non-default BatchNorm
    assert route(two()) == 'fc'
    ops.FC_EDGES_NATIVE = False
    try:
        assert route(two()) == 'composed'
    finally:
        ops.FC_EDGES_NATIVE = True


def _cell(geno, shape='s'):
    path = [p for p in fu.fixture_files() if case_id(p) == f'fcfound_{geno}_{shape}_eval'][0]
    meta, _ = fu.load(path)
    cfg = fo.Cfg(meta['cfg'])
    g = fo.genotype_from_jsonable(meta['genotype'])
    from gpu_util import Args
    from models.search.darts.model import Found_FusionNetwork
    return cfg, g, Found_FusionNetwork(cfg.S, cfg.M, cfg.N, 2, Args(cfg), None, fu.mirror_genotype(g))


def test_grouping_of_the_found_cell():
    cfg, g, net = _cell('a')
    assert net.cell.fc_groups(cfg.N) == ([0, 1, 2, 3], [])          # every source is a cell input: one group
    cfg, g, net = _cell('b')
    assert net.cell.fc_groups(cfg.N) == ([0, 1, 2, 3], [])
    cfg, g, net = _cell('c')
    assert net.cell.fc_groups(cfg.N) == ([0, 3], [])                # skip edges stay as they are
    cfg, g, net = _cell('d')
    assert g.edges[2] == ('fc_relu', cfg.N)
    assert net.cell.fc_groups(cfg.N) == ([1], [2])                  # a step-output source: a call of its own


def test_grouped_calls_are_issued_in_front_of_their_steps(monkeypatch):
    """Which edges reach found_fc_apply, in which calls, and where the step nodes run in between — with the kernels
    replaced by recorders (the cell's forward is host logic up to that call)."""
    from models.search.darts import model as model_mod
    cfg, g, net = _cell('d')
    log = []
    monkeypatch.setattr(model_mod, 'found_fc_route', lambda ops_, xs: 'fc')

    def apply(ops_, xs):
        log.append(('fc', [list(net.cell._ops).index(o) for o in ops_]))
        return tuple(torch.zeros_like(x) for x in xs)
    monkeypatch.setattr(model_mod, 'found_fc_apply', apply)
    for i, node in enumerate(net.cell._step_nodes):
        node.forward = types.MethodType(lambda self, h1, h2, i=i: (log.append(('node', i)), h1 + h2)[1], node)
    monkeypatch.setattr(model_mod.CatLnFn, 'apply', staticmethod(lambda relu, w, b, r, *s: torch.cat(s, dim=1)))
    xs = [torch.zeros(2, cfg.C, cfg.L) for _ in range(cfg.N)]
    net(xs)
    assert log == [('fc', [1]), ('node', 0), ('fc', [2]), ('node', 1)]
    # composed route: no grouped call, every edge op by op at its place
    log.clear()
    monkeypatch.setattr(model_mod, 'found_fc_route', lambda ops_, xs: 'composed')
    net.eval()
    net(xs)
    assert log == [('node', 0), ('node', 1)]


@pytest.mark.parametrize('geno', sorted(fu.EDGES))
def test_state_dict_keys_equal_found_fc_param_shapes(geno):
    cfg, g, net = _cell(geno)
    shapes = fu.found_fc_param_shapes(cfg, g)
    sd = net.state_dict()
    assert set(sd) == set(shapes), set(sd) ^ set(shapes)
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(shapes[k]), k
    assert any(k.startswith('cell._ops.') for k in sd)


@pytest.mark.parametrize('path', fu.fixture_files(), ids=case_id)
def test_fixtures_stay_away_from_the_relu_kink(path):
    """Re-asserts what the generator asserted: every fc_relu pre-activation of a stored case has |u| >= 1e-4, on the
    stored value and on the restatement's own pre-activations."""
    from oracle import synth
    meta, z = fu.load(path)
    cfg = fo.Cfg(meta['cfg'])
    g = fo.genotype_from_jsonable(meta['genotype'])
    has_relu = any(name == 'fc_relu' for name, _ in g.edges)
    assert (meta['min_abs_u'] is not None) == has_relu
    if not has_relu:
        return
    assert meta['min_abs_u'] >= fu.MIN_ABS_U
    params = synth.make_params(cfg, meta['seed'], fu.found_fc_param_shapes(cfg, g))
    xs = [torch.from_numpy(z[f'input.{i}']) for i in range(cfg.N)]
    pre = []
    with torch.no_grad():
        fu.found_fc_cell(xs, g, {k: v.clone() for k, v in params.items()}, cfg, meta['mode'] != 'eval',
                         attn_drop=0.0, drpt=0.0, pre_acts=pre)
    assert len(pre) == sum(name == 'fc_relu' for name, _ in g.edges)
    assert min(v for _, v in pre) >= fu.MIN_ABS_U
    assert abs(min(v for _, v in pre) - meta['min_abs_u']) <= 1e-6
