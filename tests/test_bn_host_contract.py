"""CPU: the host contract of the BatchNorm entry points of csrc/bnmix.hip — which return code bmnas_bn_finalize, the
three forward tails (bmnas_bn_relu_fwd, _mish_fwd, _glu_fwd), the three backward tails, the two grouped entries and
bmnas_bn_bwd_apply give for a refused argument, and what the descriptor conversion (to_fin, csrc/launch.hpp)
refuses through each forward entry.

Every call here returns before any HIP call: b = 0 with valid arguments, or exactly one refused argument.  Only
bmnas_bn_finalize is called with b > 0 (it refuses b = 0 itself), and then only with an argument its first three lines
refuse.  The pointers are host buffers that are never dereferenced as tensors.  The expected values in
tests/golden/bn_host_contract.json were recorded from the build that refuses M % 4 != 0 in the single-problem forward
entries (before it they accepted it and bn_fin_fill wrote scale over shift in LDS).  What the table pins besides:
the forward entries, the forward group and bmnas_bn_bwd_apply take every L % 4 == 0 up to 16 (0 and 12 included),
the backward entries only 4, 8 and 16; the backward entries do not look at M % 4; a training-mode descriptor is refused
at b = 0 (b L < 2), so an accepted training call cannot be made here.  Regenerate with
    python tests/test_bn_host_contract.py > tests/golden/bn_host_contract.json
only when the contract is changed on purpose."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'bn_host_contract.json')

_BUF = (C.c_float * 64)()          # one host buffer stands for every tensor argument
PTR = C.addressof(_BUF)


def _lib():
    from bmnas import build, lib
    build.build()
    return lib, lib.load()


def _fin(**over):
    """an eval-mode descriptor every forward entry accepts"""
    f = dict(stat=PTR, conv_bias=PTR, bn_w=PTR, bn_b=PTR, running_mean=PTR, running_var=PTR, num_batches_tracked=PTR,
             shards=4, n_nbt=1, training=0, on=1)
    f.update(over)
    return f


def _fin_struct(lib, f):
    return lib.BnFin(f['stat'], f['conv_bias'], f['bn_w'], f['bn_b'], f['running_mean'], f['running_var'],
                     f['num_batches_tracked'], f['shards'], f['n_nbt'], f['training'], f['on'])


# (case id, descriptor): to_fin's refusals, then the entry's own b L < 2
FIN = [('fin off, every field 0', dict(stat=None, conv_bias=None, bn_w=None, bn_b=None, running_mean=None, running_var=None,
                                        num_batches_tracked=None, shards=0, n_nbt=0, training=0, on=0)),
       ('fin eval, stat / conv_bias / nbt NULL, shards 0', _fin(stat=None, conv_bias=None, num_batches_tracked=None, shards=0)),
       ('fin bn_w=NULL', _fin(bn_w=None)), ('fin bn_b=NULL', _fin(bn_b=None)),
       ('fin shards=-1', _fin(shards=-1)), ('fin shards=5', _fin(shards=5)), ('fin training shards=5', _fin(shards=5, training=1)),
       ('fin training shards=0', _fin(shards=0, training=1)), ('fin training stat=NULL', _fin(stat=None, training=1)),
       ('fin n_nbt=-1', _fin(n_nbt=-1)), ('fin training n_nbt=-1', _fin(n_nbt=-1, training=1)),
       ('fin training running_mean without running_var', _fin(running_var=None, training=1)),
       ('fin training running_var without running_mean', _fin(running_mean=None, training=1)),
       ('fin eval running_mean=NULL', _fin(running_mean=None)), ('fin eval running_var=NULL', _fin(running_var=None)),
       ('fin eval without running statistics', _fin(running_mean=None, running_var=None)),
       ('fin training valid, b L = 0 < 2', _fin(training=1)),
       ('fin training without running statistics, b L = 0 < 2', _fin(training=1, running_mean=None, running_var=None))]

L_ROWS = [(f'L={v}', {'L': v}) for v in (0, 2, 6, 12, 20)]


def _base():
    return dict(U=PTR, chan=PTR, out=PTR, g=PTR, dV=PTR, bn_grad=PTR, fin=_fin(), b=0, M=64, C=32, L=8, training=0)


def call_act_fwd(name):
    def call(lib, so, a):
        return getattr(so, name)(a['U'], a['chan'], _fin_struct(lib, a['fin']), a['out'], a['b'], a['M'], a['L'],
                                 lib.NO_DROP, None)
    return call


def call_glu_fwd(lib, so, a):
    return so.bmnas_bn_glu_fwd(a['U'], a['chan'], _fin_struct(lib, a['fin']), a['out'], a['b'], a['C'], a['L'],
                               lib.NO_DROP, None)


def call_act_bwd(name, dim='M'):
    def call(lib, so, a):
        return getattr(so, name)(a['g'], a['U'], a['chan'], a['dV'], a['bn_grad'], a['b'], a[dim], a['L'], lib.NO_DROP,
                                 None)
    return call


def call_bwd_apply(lib, so, a):
    return so.bmnas_bn_bwd_apply(a['dV'], a['U'], a['chan'], a['bn_grad'], a['b'], a['M'], a['L'], a['training'], None)


def _rows(ptrs, dim_rows):
    return ([('valid b=0', {})] + [(f'{n}=NULL', {n: None}) for n in ptrs] + [('b=-1', {'b': -1})] + L_ROWS + dim_rows)


_M_ROWS = [('M=0', {'M': 0}), ('M=4', {'M': 4}), ('M=6 (% 4)', {'M': 6}), ('M=4094 (% 4)', {'M': 4094}),
           ('M=4096', {'M': 4096}), ('M=4097', {'M': 4097}), ('M=4100', {'M': 4100})]
_C_ROWS = [('C=0', {'C': 0}), ('C=2', {'C': 2}), ('C=3 (odd)', {'C': 3}), ('C=2047 (odd)', {'C': 2047}),
           ('C=2048', {'C': 2048}), ('C=2049 (2C = 4098)', {'C': 2049}), ('C=2050', {'C': 2050})]
_FIN_ROWS = [(cid, {'fin': f}) for cid, f in FIN]

SINGLE = {
    'bmnas_bn_relu_fwd': (call_act_fwd('bmnas_bn_relu_fwd'), _rows(['U', 'chan', 'out'], _M_ROWS) + _FIN_ROWS),
    'bmnas_bn_mish_fwd': (call_act_fwd('bmnas_bn_mish_fwd'), _rows(['U', 'chan', 'out'], _M_ROWS) + _FIN_ROWS),
    'bmnas_bn_glu_fwd': (call_glu_fwd, _rows(['U', 'chan', 'out'], _C_ROWS) + _FIN_ROWS),
    'bmnas_bn_relu_bwd': (call_act_bwd('bmnas_bn_relu_bwd'), _rows(['g', 'U', 'chan', 'dV', 'bn_grad'], _M_ROWS)),
    'bmnas_bn_mish_bwd': (call_act_bwd('bmnas_bn_mish_bwd'), _rows(['g', 'U', 'chan', 'dV', 'bn_grad'], _M_ROWS)),
    'bmnas_bn_glu_bwd': (call_act_bwd('bmnas_bn_glu_bwd', 'C'), _rows(['g', 'U', 'chan', 'dV', 'bn_grad'], _C_ROWS)),
    'bmnas_bn_bwd_apply': (call_bwd_apply, _rows(['dV', 'U', 'chan', 'bn_grad'], _M_ROWS) +
                           [('training valid b=0', {'training': 1}), ('training bn_grad=NULL', {'training': 1, 'bn_grad': None}),
                            ('training U=NULL', {'training': 1, 'U': None})]),
}


def _single_codes(fn):
    lib, so = _lib()
    call, rows = SINGLE[fn]
    got = {}
    for cid, over in rows:
        a = _base()
        a.update(over)
        assert a['b'] <= 0, cid                                   # nothing here may reach a launch
        got[cid] = call(lib, so, a)
    return got


# ---- bmnas_bn_finalize: b = 0 is itself refused, so every row carries one argument that the entry refuses ---------
def _finalize_base():
    return dict(part=PTR, n_part=1, b=1, L=8, M=8, bn_w=PTR, bn_b=PTR, rm=PTR, rv=PTR, nbt=PTR, n_nbt=1, training=1,
                chan=PTR)


FINALIZE = [('bn_w=NULL', {'bn_w': None}), ('bn_b=NULL', {'bn_b': None}), ('chan=NULL', {'chan': None}),
            ('M=0', {'M': 0}), ('b=0', {'b': 0}), ('b=-1', {'b': -1}), ('L=0', {'L': 0}),
            ('eval bn_w=NULL', {'bn_w': None, 'training': 0}), ('eval b=0', {'b': 0, 'training': 0}),
            ('training part=NULL', {'part': None}), ('training n_part=0', {'n_part': 0}),
            ('training b L = 1 < 2', {'L': 1}),
            ('eval running_mean=NULL', {'training': 0, 'rm': None}), ('eval running_var=NULL', {'training': 0, 'rv': None}),
            ('eval without running statistics', {'training': 0, 'rm': None, 'rv': None})]


def _finalize_refused(a):
    """the refusals of bmnas_bn_finalize as its first three lines state them: a row that they let through would launch"""
    if not a['bn_w'] or not a['bn_b'] or not a['chan'] or a['M'] < 1 or a['b'] < 1 or a['L'] < 1:
        return True
    if a['training']:
        return not a['part'] or a['n_part'] < 1 or a['b'] * a['L'] < 2
    return not a['rm'] or not a['rv']


def _finalize_codes():
    lib, so = _lib()
    got = {}
    for cid, over in FINALIZE:
        a = _finalize_base()
        a.update(over)
        assert _finalize_refused(a), cid
        got[cid] = so.bmnas_bn_finalize(a['part'], a['n_part'], a['b'], a['L'], a['M'], a['bn_w'], a['bn_b'], a['rm'],
                                        a['rv'], a['nbt'], a['n_nbt'], a['training'], a['chan'], None)
    return got


# ---- the grouped entry points -------------------------------------------------------------------------------------
def _fwd_prob(**over):
    p = dict(U=PTR, chan=PTR, out=PTR, fin=_fin())
    p.update(over)
    return p


def _bwd_prob(**over):
    p = dict(g=PTR, U=PTR, chan=PTR, dV=PTR, bn_grad=PTR)
    p.update(over)
    return p


_GROUP_ARGS = ([('valid b=0', {}), ('valid b=0, n=8', {'n': 8}), ('probs=NULL', {'null': True}), ('n=0', {'n': 0}),
                ('n=9', {'n': 9}), ('n=-1', {'n': -1}), ('b=-1', {'b': -1})] + L_ROWS + _M_ROWS)
GROUP = {
    'bmnas_bn_relu_fwd_group': (
        'BnReluFwdProb', _fwd_prob,
        _GROUP_ARGS + [(f'probs[{i}]: {f}=NULL', {'prob': {f: None}, 'at': i}) for i in (0, 2) for f in ('U', 'chan', 'out')] +
        [(f'probs[{i}]: {cid}', {'prob': {'fin': f}, 'at': i}) for i in (0, 2) for cid, f in FIN]),
    'bmnas_bn_relu_bwd_group': (
        'BnReluBwdProb', _bwd_prob,
        _GROUP_ARGS + [(f'probs[{i}]: {f}=NULL', {'prob': {f: None}, 'at': i}) for i in (0, 2)
                       for f in ('g', 'U', 'chan', 'dV', 'bn_grad')]),
}


def _group_codes(fn):
    lib, so = _lib()
    struct, make, rows = GROUP[fn]
    cls = getattr(lib, struct)
    got = {}
    for cid, over in rows:
        probs = [make(**(over.get('prob', {}) if i == over.get('at', -1) else {})) for i in range(9)]
        arr = (cls * 9)()
        for i, p in enumerate(probs):
            if struct == 'BnReluFwdProb':
                arr[i] = cls(p['U'], p['chan'], p['out'], _fin_struct(lib, p['fin']), lib.NO_DROP)
            else:
                arr[i] = cls(p['g'], p['U'], p['chan'], p['dV'], p['bn_grad'], lib.NO_DROP)
        b = over.get('b', 0)
        assert b <= 0, cid
        got[cid] = getattr(so, fn)(None if over.get('null') else arr, over.get('n', 3), b, over.get('M', 64),
                                   over.get('L', 8), None)
    return got


def record():
    out = {fn: _single_codes(fn) for fn in SINGLE}
    out['bmnas_bn_finalize'] = _finalize_codes()
    out.update({fn: _group_codes(fn) for fn in GROUP})
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


def test_bn_finalize_return_codes():
    got = _finalize_codes()
    bad = _diff(got, _golden()['bmnas_bn_finalize'])
    assert not bad, f'case -> (returned, recorded): {bad}'
    assert set(got.values()) == {-1}                               # every row is a refusal: nothing was launched


@pytest.mark.parametrize('fn', sorted(GROUP))
def test_group_entry_point_return_codes(fn):
    bad = _diff(_group_codes(fn), _golden()[fn])
    assert not bad, f'{fn}: case -> (returned, recorded): {bad}'


def test_no_row_reached_a_launch():
    """a code > 0 is a hipError_t: a call that got as far as a launch"""
    g = _golden()
    assert len(g) == 10
    assert all(code <= 0 for table in g.values() for code in table.values())


def test_the_forward_entries_refuse_what_bn_fin_fill_cannot_write():
    """four adjacent channels per thread, float4 LDS stores at sc + 4 t and sh = sc + M: M % 4 == 0, with the code the
    grouped entry already returned; the backward entries (one channel per thread) take any M"""
    g = _golden()
    for fn in ('bmnas_bn_relu_fwd', 'bmnas_bn_mish_fwd', 'bmnas_bn_relu_fwd_group'):
        assert g[fn]['M=6 (% 4)'] == g[fn]['M=4094 (% 4)'] == g[fn]['M=4097'] == g[fn]['M=4100'] == -3, fn
        assert g[fn]['M=4'] == g[fn]['M=4096'] == 0, fn
    t = g['bmnas_bn_glu_fwd']
    assert t['C=3 (odd)'] == t['C=2047 (odd)'] == t['C=2049 (2C = 4098)'] == t['C=2050'] == -3
    assert t['C=2'] == t['C=2048'] == 0
    assert g['bmnas_bn_relu_bwd']['M=6 (% 4)'] == 0 and g['bmnas_bn_glu_bwd']['C=3 (odd)'] == 0


def test_the_pinned_differences_between_entry_points_are_in_the_table():
    g = _golden()
    for fn in ('bmnas_bn_relu_fwd', 'bmnas_bn_mish_fwd', 'bmnas_bn_glu_fwd', 'bmnas_bn_relu_fwd_group', 'bmnas_bn_bwd_apply'):
        assert [g[fn][f'L={v}'] for v in (0, 2, 6, 12, 20)] == [0, -2, -2, 0, -2], fn
    for fn in ('bmnas_bn_relu_bwd', 'bmnas_bn_mish_bwd', 'bmnas_bn_glu_bwd', 'bmnas_bn_relu_bwd_group'):
        assert [g[fn][f'L={v}'] for v in (0, 2, 6, 12, 20)] == [-2] * 5, fn
    t = g['bmnas_bn_relu_fwd']
    assert t['fin shards=5'] == -3 and t['fin training shards=0'] == -1 and t['fin n_nbt=-1'] == -1
    assert t['fin training running_mean without running_var'] == -1 and t['fin eval without running statistics'] == -1
    assert t['fin training valid, b L = 0 < 2'] == -1 and t['fin off, every field 0'] == 0
    for fn in ('bmnas_bn_relu_fwd_group', 'bmnas_bn_relu_bwd_group'):
        assert g[fn]['n=0'] == -1 and g[fn]['n=9'] == -3 and g[fn]['valid b=0, n=8'] == 0, fn
    assert g['bmnas_bn_relu_fwd_group']['probs[2]: fin shards=5'] == -3
    assert g['bmnas_bn_bwd_apply']['bn_grad=NULL'] == -1               # refused in eval too, where it is never read


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))
    json.dump(record(), sys.stdout, indent=1, sort_keys=True)
    print()
