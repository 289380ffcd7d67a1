"""CPU: the host contract of csrc/conv1x1.hip — which return code every conv entry point gives for a refused
argument, and what the shape queries answer.

Every call here returns before any HIP call: b = 0 with valid arguments, or one refused argument (a call with
b > 0 is only ever made with an argument that is refused first).  The pointers are host buffers that are never
dereferenced as tensors.  The expected values in tests/golden/conv_host_contract.json were recorded from the build
of the commit BEFORE the host half was rewritten around one validation and one rule per kernel family, so the
table pins the differences between the entry points as they were (bmnas_conv1x1_bwd_data accepts an ldw that is no
multiple of 4, bmnas_conv1x1_fwd_sdpa a negative stat_shards, ...).  Regenerate with
    python tests/test_conv_host_contract.py > tests/golden/conv_host_contract.json
only when the contract is changed on purpose."""
import ctypes as C
import itertools
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'conv_host_contract.json')

_BUF = (C.c_float * 64)()          # one host buffer stands for every tensor argument
PTR = C.addressof(_BUF)
PTR2 = PTR + 64                    # a second address, for "is not the same tensor" checks


def _lib():
    from bmnas import build, lib
    build.build()
    return lib, lib.load()


def _arr(ptrs):
    return (C.c_void_p * max(1, len(ptrs)))(*ptrs)


def _base():
    """Arguments every single-problem entry point accepts (with b = 0: nothing is launched)."""
    return dict(n_src=2, C_src=32, M=48, ldw=64, fold_cols=0, b=0, L=8, stat_shards=0, dup_cols=0, ldw_grad=64,
                C=32, acc=0, bn_training=0,
                srcs=[PTR, PTR], dsrcs=[PTR, PTR], wsrcs=[PTR, PTR],
                W=PTR, U=PTR, dU=PTR, bias=PTR, part=PTR, dW=PTR, dbias=PTR,
                x=PTR, y=PTR, ln_w=PTR, ln_b=PTR, out=PTR, xhat=PTR, stats=PTR,
                g=PTR, gscale=None, dx=PTR2, dy=None,
                bn_U=None, bn_chan=None, bn_grad=None, mix=None)


def _list(v):
    return None if v is None else _arr(v)


def call_fwd(lib, so, a):
    return so.bmnas_conv1x1_fwd(_list(a['srcs']), a['n_src'], a['C_src'], a['W'], a['ldw'], a['fold_cols'], a['bias'],
                                a['U'], a['part'], a['stat_shards'], a['b'], a['L'], a['M'], None)


def call_bwd_data(lib, so, a):
    return so.bmnas_conv1x1_bwd_data(a['dU'], a['W'], a['ldw'], a['fold_cols'], _list(a['dsrcs']), a['n_src'],
                                     a['C_src'], a['acc'], a['b'], a['L'], a['M'], None)


def call_fwd_sdpa(lib, so, a):
    return so.bmnas_conv1x1_fwd_sdpa(_list(a['srcs']), a['n_src'], a['C_src'], a['W'], a['ldw'], a['fold_cols'],
                                     a['bias'], a['U'], a['part'], a['stat_shards'], a['b'], a['L'], a['M'], a['x'],
                                     a['y'], a['ln_w'], a['ln_b'], a['out'], a['xhat'], a['stats'], a['C'],
                                     lib.NO_DROP, None)


def call_bwd_weight(lib, so, a):
    return so.bmnas_conv1x1_bwd_weight(a['dU'], _list(a['wsrcs']), a['n_src'], a['C_src'], a['dW'], a['ldw_grad'],
                                       a['dbias'], a['dup_cols'], a['b'], a['L'], a['M'], None)


def call_bwd_all_sdpa(lib, so, a):
    return so.bmnas_conv1x1_bwd_all_sdpa(a['dU'], a['W'], a['ldw'], a['fold_cols'], _list(a['dsrcs']), a['n_src'],
                                         a['C_src'], a['acc'], a['b'], a['L'], a['M'], _list(a['wsrcs']), a['dW'],
                                         a['ldw_grad'], a['dbias'], a['dup_cols'], a['g'], a['gscale'], a['x'],
                                         a['y'], a['ln_w'], a['xhat'], a['stats'], a['dx'], a['dy'], 0, a['C'],
                                         lib.NO_DROP, a['bn_U'], a['bn_chan'], a['bn_grad'], a['bn_training'], None)


def _mix_struct(lib, m):
    if m is None:
        return None
    return C.byref(lib.MixEp(m['U'], m['chan'], m['x'], m['p1'], m['gamma'], m['dgamma'], m['dgamma_shards'], 0,
                             m['dx'], 0, m['dV'], m['bn_grad'], m['q'], lib.NO_DROP, lib.NO_DROP))


def call_bwd_all_mix(lib, so, a):
    return so.bmnas_conv1x1_bwd_all_mix(a['dU'], a['W'], a['ldw'], a['fold_cols'], _list(a['dsrcs']), a['n_src'],
                                        a['C_src'], a['acc'], a['b'], a['L'], a['M'], _list(a['wsrcs']), a['dW'],
                                        a['ldw_grad'], a['dbias'], a['dup_cols'], a['bn_U'], a['bn_chan'],
                                        a['bn_grad'], a['bn_training'], _mix_struct(lib, a['mix']), None)


def call_bwd_all(lib, so, a):
    return so.bmnas_conv1x1_bwd_all(a['dU'], a['W'], a['ldw'], a['fold_cols'], _list(a['dsrcs']), a['n_src'],
                                    a['C_src'], a['acc'], a['b'], a['L'], a['M'], _list(a['wsrcs']), a['dW'],
                                    a['ldw_grad'], a['dbias'], a['dup_cols'], a['bn_U'], a['bn_chan'], a['bn_grad'],
                                    a['bn_training'], None)


def _variants(names, lists, extra=()):
    """(case id, overrides) for one entry point: the valid call, every pointer of `names` NULL, every list of `lists`
    NULL or with a NULL entry, and the common bad values."""
    out = [('valid b=0', {})]
    out += [(f'{n}=NULL', {n: None}) for n in names]
    for n in lists:
        out += [(f'{n}=NULL', {n: None}), (f'{n}[1]=NULL b=0', {n: [PTR, None]})]
        if n != 'dsrcs':           # (a NULL entry of dsrcs means "skip this gradient": a valid call, which b = 4 would launch)
            out += [(f'{n}[1]=NULL b=4', {n: [PTR, None], 'b': 4})]
    out += [('b=-1', {'b': -1}), ('L=5', {'L': 5}), ('L=32', {'L': 32}), ('C_src=24', {'C_src': 24}),
            ('C_src=0', {'C_src': 0}), ('M=24', {'M': 24}), ('M=0', {'M': 0}), ('n_src=5', {'n_src': 5}),
            ('n_src=0', {'n_src': 0})]
    out += list(extra)
    return out


_LDW = [('ldw=60 (too small)', {'ldw': 60}), ('ldw=66 (% 4)', {'ldw': 66}), ('fold_cols=2', {'fold_cols': 2}),
        ('fold_cols=-4', {'fold_cols': -4}), ('fold_cols=32 with ldw=64', {'fold_cols': 32}),
        ('fold_cols=32 with ldw=96', {'fold_cols': 32, 'ldw': 96})]
_SHARDS = [('stat_shards=-1', {'stat_shards': -1}), ('stat_shards=4', {'stat_shards': 4})]
_WGRAD = [('ldw_grad=60 (too small)', {'ldw_grad': 60}), ('ldw_grad=66', {'ldw_grad': 66}),
          ('dup_cols=-1', {'dup_cols': -1}), ('dup_cols=32 with ldw_grad=64', {'dup_cols': 32}),
          ('dup_cols=32 with ldw_grad=96', {'dup_cols': 32, 'ldw_grad': 96})]
_BN = [('bn_U without bn_chan', {'bn_U': PTR}), ('bn_U eval without bn_grad', {'bn_U': PTR, 'bn_chan': PTR}),
       ('bn_U training without bn_grad', {'bn_U': PTR, 'bn_chan': PTR, 'bn_training': 1}),
       ('bn_U training', {'bn_U': PTR, 'bn_chan': PTR, 'bn_grad': PTR, 'bn_training': 1})]
_SDPA_C = [('C=24', {'C': 24}), ('C=0', {'C': 0}), ('C=528', {'C': 528})]


def _mix(**over):
    m = dict(U=PTR, chan=PTR, x=PTR, p1=PTR, gamma=PTR, dgamma=PTR, dgamma_shards=1, dx=PTR, dV=PTR, bn_grad=PTR, q=1)
    m.update(over)
    return m


_MIX = ([('mix valid b=0', {'mix': _mix()}), ('mix dgamma=NULL', {'mix': _mix(dgamma=None)})] +
        [(f'mix {f}=NULL', {'mix': _mix(**{f: None})}) for f in ('U', 'chan', 'x', 'p1', 'gamma', 'dx', 'dV', 'bn_grad')] +
        [('mix q=-1', {'mix': _mix(q=-1)}), ('mix q=n_src', {'mix': _mix(q=2)}),
         ('mix dgamma_shards=0', {'mix': _mix(dgamma_shards=0)}),
         ('mix dsrcs[q]=NULL', {'mix': _mix(), 'dsrcs': [PTR, None]}),
         ('mix dsrcs=NULL', {'mix': _mix(), 'dsrcs': None}),
         ('mix fold_cols=32', {'mix': _mix(), 'fold_cols': 32, 'ldw': 96}),
         ('mix M=320 (outside the one-launch form)', {'mix': _mix(), 'M': 320}),
         ('mix L=5', {'mix': _mix(), 'L': 5}), ('mix C_src=24', {'mix': _mix(), 'C_src': 24}),
         ('mix b=-1', {'mix': _mix(), 'b': -1})])

# bmnas_conv1x1_bwd_weight, and every entry point that sizes weight-gradient splits, divides by a split size of zero
# when b = 0 reaches that arithmetic (SIGFPE; a defect as old as the split rule, left for an issue of its own).  So the
# ACCEPTED calls of those entry points cannot be made here, only the refused ones; bmnas_conv1x1_bwd_all_sdpa is
# called with dW = NULL (no weight gradient wanted) wherever the weight-gradient arguments are not what is tested.
_ACCEPTED_WITH_WGRAD = {'valid b=0', 'dbias=NULL', 'dsrcs[1]=NULL b=0', 'ldw=66 (% 4)', 'fold_cols=32 with ldw=96',
                        'ldw_grad=66', 'dup_cols=32 with ldw_grad=96', 'bn_U eval without bn_grad', 'bn_U training',
                        'mix valid b=0', 'mix dgamma=NULL', 'probs[0]: dsrc=NULL',
                        'probs[0]: dbias=NULL', 'probs[0]: bn_U eval without bn_grad'}


def _refused(variants):
    return [(cid, over) for cid, over in variants if cid not in _ACCEPTED_WITH_WGRAD]


_BWD_ALL_SDPA = (
    [(cid, {'dW': None, **over}) for cid, over in
     _variants(['dU', 'W', 'dbias', 'g', 'x', 'y', 'ln_w', 'xhat', 'stats', 'dx'], ['dsrcs'],
               _LDW + _BN + _SDPA_C + [('dsrcs[1] is dx', {'dsrcs': [PTR, PTR2]}),
                                       ('dsrcs[0] is dy', {'dsrcs': [PTR2 + 64, PTR], 'dy': PTR2 + 64}),
                                       ('wsrcs=NULL', {'wsrcs': None}), ('dup_cols=-1', {'dup_cols': -1})])] +
    [(f'dW given, {cid}', over) for cid, over in
     _refused(_WGRAD) + [('wsrcs=NULL', {'wsrcs': None}), ('wsrcs[1]=NULL b=0', {'wsrcs': [PTR, None]}),
                         ('wsrcs[1]=NULL b=4', {'wsrcs': [PTR, None], 'b': 4}), ('L=5', {'L': 5}), ('M=24', {'M': 24})]])

SINGLE = {
    'bmnas_conv1x1_fwd': (call_fwd, _variants(['W', 'U', 'bias', 'part'], ['srcs'], _LDW + _SHARDS)),
    'bmnas_conv1x1_bwd_data': (call_bwd_data, _variants(['dU', 'W'], ['dsrcs'], _LDW)),
    'bmnas_conv1x1_fwd_sdpa': (call_fwd_sdpa,
                               _variants(['W', 'U', 'bias', 'part', 'x', 'y', 'ln_w', 'ln_b', 'out', 'xhat', 'stats'],
                                         ['srcs'], _LDW + _SHARDS + _SDPA_C)),
    'bmnas_conv1x1_bwd_weight': (call_bwd_weight, _refused(_variants(['dU', 'dW', 'dbias'], ['wsrcs'], _WGRAD))),
    'bmnas_conv1x1_bwd_all_sdpa': (call_bwd_all_sdpa, _BWD_ALL_SDPA),
    'bmnas_conv1x1_bwd_all_mix': (call_bwd_all_mix,
                                  _refused(_variants(['dU', 'W', 'dW', 'dbias'], ['dsrcs', 'wsrcs'],
                                                     _LDW + _WGRAD + _BN + _MIX))),
    'bmnas_conv1x1_bwd_all': (call_bwd_all,
                              _refused(_variants(['dU', 'W', 'dW', 'dbias'], ['dsrcs', 'wsrcs'], _LDW + _WGRAD + _BN))),
}


def _single_codes(fn):
    lib, so = _lib()
    call, variants = SINGLE[fn]
    got = {}
    for cid, over in variants:
        a = _base()
        a.update(over)
        got[cid] = call(lib, so, a)
    return got


# ---- the grouped entry points -------------------------------------------------------------------------------------
def _fwd_prob(**over):
    p = dict(src=PTR, W=PTR, bias=PTR, U=PTR, stat=PTR, C_in=64, ldw=64)
    p.update(over)
    return p


def _bwd_prob(**over):
    p = dict(dV=PTR, W=PTR, src=PTR, dsrc=PTR, dW=PTR, dbias=PTR, bn_U=None, bn_chan=None, bn_grad=None, C_in=64,
             ldw=64, ldw_grad=64, accumulate=0)
    p.update(over)
    return p


_GROUP_ARGS = [('valid b=0', {}), ('probs=NULL', {'null': True}), ('n=0', {'n': 0}), ('n=9', {'n': 9}),
               ('b=-1', {'b': -1}), ('M=24', {'M': 24}), ('M=0', {'M': 0}), ('M=400', {'M': 400}), ('L=5', {'L': 5})]
_GROUP_PROB = [('C_in=8', {'C_in': 8}), ('C_in=24', {'C_in': 24, 'ldw': 24}), ('ldw=60 (too small)', {'ldw': 60}),
               ('ldw=66 (% 4)', {'ldw': 66})]
GROUP = {
    'bmnas_conv1x1_fwd_group': (
        'ConvFwdProb', _fwd_prob,
        _GROUP_ARGS + [('stat_shards=-1', {'flag': -1}), ('stat_shards=4', {'flag': 4})] +
        [(f'probs[0]: {k}', {'prob': v}) for k, v in
         [(f'{f}=NULL', {f: None}) for f in ('src', 'W', 'bias', 'U', 'stat')] + _GROUP_PROB] +
        [('probs[0]: stat=NULL with stat_shards=4', {'prob': {'stat': None}, 'flag': 4})]),
    'bmnas_conv1x1_bwd_group': (
        'ConvBwdProb', _bwd_prob,
        _refused(_GROUP_ARGS + [(f'probs[0]: {k}', {'prob': v}) for k, v in
                                [(f'{f}=NULL', {f: None}) for f in ('dV', 'W', 'src', 'dsrc', 'dW', 'dbias')] +
                                _GROUP_PROB +
                                [('ldw_grad=60 (too small)', {'ldw_grad': 60}), ('bn_U without bn_chan', {'bn_U': PTR}),
                                 ('bn_U eval without bn_grad', {'bn_U': PTR, 'bn_chan': PTR})]] +
                 [('probs[0]: bn_U training without bn_grad', {'prob': {'bn_U': PTR, 'bn_chan': PTR}, 'flag': 1})])),
}


def _group_codes(fn):
    lib, so = _lib()
    struct, make, variants = GROUP[fn]
    cls = getattr(lib, struct)
    names = [f for f, _ in cls._fields_]
    got = {}
    for cid, over in variants:
        probs = [make(**over.get('prob', {}))] + [make() for _ in range(8)]
        arr = (cls * len(probs))(*[cls(*[p[f] for f in names]) for p in probs])
        got[cid] = getattr(so, fn)(None if over.get('null') else arr, over.get('n', 1 if 'prob' in over else 2), over.get('flag', 0),
                                   over.get('b', 0), over.get('L', 8), over.get('M', 64), None)
    return got


# ---- the shape queries --------------------------------------------------------------------------------------------
MIX_OK_GRID = list(itertools.product((1, 2, 6, 8, 16, 48, 64, 128, 256, 512, 1024), (4, 8, 16),
                                     (32, 48, 64, 96, 128, 192, 256, 320), (1, 2, 3, 4)))
MIX_OK_EXTRA = [(0, 8, 64, 2, 64), (-1, 8, 64, 2, 64), (8, 5, 64, 2, 64), (8, 8, 24, 2, 64), (8, 8, 64, 2, 24),
                (8, 8, 64, 0, 64), (8, 8, 48, 2, 64), (256, 16, 48, 2, 64), (190, 16, 48, 1, 64), (192, 16, 48, 1, 64)]
GROUP_OK = [(2, [64, 32], 4, 8, 32), (1, [2048], 64, 8, 128), (8, [64] * 8, 6, 16, 384), (9, [64] * 9, 6, 16, 384),
            (0, [64], 6, 16, 64), (2, [64, 8], 4, 8, 32), (2, [64, 24], 4, 8, 32), (2, [64, 32], 0, 8, 32),
            (2, [64, 32], 4, 5, 32), (2, [64, 32], 4, 8, 24), (2, [64, 32], 4, 8, 400), (2, [64, 32], 4, 8, 0),
            (2, None, 4, 8, 32)]
NUM_PARTIALS = [(1, 4), (1, 8), (1, 16), (3, 4), (4, 4), (5, 4), (128, 8), (129, 8), (6, 16), (0, 8), (-1, 8),
                (8, 5), (8, 32)]


def _query_codes():
    lib, so = _lib()
    return {
        'mix_ok': ''.join(str(so.bmnas_conv1x1_bwd_all_mix_ok(b, L, c, n, c)) for b, L, c, n in MIX_OK_GRID),
        'mix_ok_extra': [so.bmnas_conv1x1_bwd_all_mix_ok(*a) for a in MIX_OK_EXTRA],
        'group_ok': [so.bmnas_conv1x1_group_ok(n, None if cs is None else (C.c_int * len(cs))(*cs), b, L, M)
                     for n, cs, b, L, M in GROUP_OK],
        'num_partials': [so.bmnas_conv1x1_num_partials(b, L) for b, L in NUM_PARTIALS],
    }


def record():
    out = {fn: _single_codes(fn) for fn in SINGLE}
    out.update({fn: _group_codes(fn) for fn in GROUP})
    out.update(_query_codes())
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _diff(got, want):
    assert sorted(got) == sorted(want), 'the case list and the recorded table differ: regenerate on purpose only'
    return {k: (got[k], want[k]) for k in got if got[k] != want[k]}


@pytest.mark.parametrize('fn', sorted(SINGLE))
def test_single_problem_entry_point_return_codes(fn):
    bad = _diff(_single_codes(fn), _golden()[fn])
    assert not bad, f'{fn}: case -> (returned, recorded): {bad}'


@pytest.mark.parametrize('fn', sorted(GROUP))
def test_group_entry_point_return_codes(fn):
    bad = _diff(_group_codes(fn), _golden()[fn])
    assert not bad, f'{fn}: case -> (returned, recorded): {bad}'


def test_the_pinned_differences_between_entry_points_are_in_the_table():
    """What the table is for: the entry points do NOT all check the same things, and callers rely on the codes."""
    g = _golden()
    assert g['bmnas_conv1x1_fwd']['valid b=0'] == 0 and g['bmnas_conv1x1_fwd']['L=5'] == -2
    assert g['bmnas_conv1x1_fwd']['n_src=5'] == -3 and g['bmnas_conv1x1_fwd']['W=NULL'] == -1
    assert g['bmnas_conv1x1_fwd']['ldw=66 (% 4)'] == -2 and g['bmnas_conv1x1_bwd_data']['ldw=66 (% 4)'] == 0
    assert g['bmnas_conv1x1_fwd']['stat_shards=-1'] == -1 and g['bmnas_conv1x1_fwd_sdpa']['stat_shards=-1'] == 0
    assert g['bmnas_conv1x1_bwd_all_sdpa']['dsrcs[1] is dx'] == -1


def test_bwd_all_mix_ok_over_the_shape_grid():
    got, want = _query_codes()['mix_ok'], _golden()['mix_ok']
    assert len(want) == len(MIX_OK_GRID) == 1056 and want.count('1') == 697 and want.count('0') == 359
    bad = [(MIX_OK_GRID[i], got[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not bad, f'(b, L, C, n_src) -> answered: {bad[:20]} ({len(bad)} in all)'


@pytest.mark.parametrize('key,args', [('mix_ok_extra', MIX_OK_EXTRA), ('group_ok', GROUP_OK),
                                      ('num_partials', NUM_PARTIALS)])
def test_shape_queries(key, args):
    got, want = _query_codes()[key], _golden()[key]
    assert len(got) == len(want)
    bad = [(a, g, w) for a, g, w in zip(args, got, want) if g != w]
    assert not bad, f'{key}: (arguments, answered, recorded): {bad}'


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))
    json.dump(record(), sys.stdout, indent=1, sort_keys=True)
    print()
