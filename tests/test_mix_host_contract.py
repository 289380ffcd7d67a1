"""CPU: the host contract of the NodeMixedOp mix entry points — bmnas_node_mix_fwd_next (hence bmnas_node_mix_fwd),
bmnas_node_mix_ln_fwd, bmnas_node_mix_pre_fwd, bmnas_node_mix_bwd_next, bmnas_node_mix_ln_bwd,
bmnas_node_mix_sel_act_fwd / _bwd and bmnas_node_mix_conv_fwd: which return code each gives for a refused argument, in
which order (BMNAS_E_ARG -1, then BMNAS_E_SHAPE -2, then BMNAS_E_LIMIT -3), and what the descriptor conversion (to_fin,
csrc/launch.hpp) refuses through each forward entry.

Every call here returns before any HIP call: b = 0 with valid arguments, or an argument that the entry refuses (the
order rows carry two, and show which one wins).  The only rows with b > 0 are refusals that the entry makes AFTER its
b == 0 return (bmnas_node_mix_ln_bwd: b 129, C 514 at L 16; bmnas_node_mix_conv_fwd: its _ok limits and ldw) — _b_rows_ok
states those refusals again in Python, and a row they would let through is not called.  The pointers are host buffers
that are never dereferenced as tensors.

The expected values in tests/golden/mix_host_contract.json were recorded from the build in which the three forward
entries that finalise BatchNorm in the kernel (bn_fin_fill: four adjacent channels per thread, scale | shift of 3 C
rows in LDS) refuse (3 C) % 4 != 0 and 3 C > 4096 with BMNAS_E_LIMIT — before it they accepted any C >= 1 (at b = 0 they
returned 0 for C 1, 2, 3, 5, 6 and 1368: exactly the rows on which this table differs from that build).  Regenerate with
    python tests/test_mix_host_contract.py > tests/golden/mix_host_contract.json
only when the contract is changed on purpose."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'mix_host_contract.json')

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


FIN = [('fin off, every field 0', dict(stat=None, conv_bias=None, bn_w=None, bn_b=None, running_mean=None, running_var=None,
                                        num_batches_tracked=None, shards=0, n_nbt=0, training=0, on=0)),
       ('fin eval, stat / conv_bias / nbt NULL, shards 0', _fin(stat=None, conv_bias=None, num_batches_tracked=None, shards=0)),
       ('fin bn_w=NULL', _fin(bn_w=None)), ('fin bn_b=NULL', _fin(bn_b=None)),
       ('fin shards=-1', _fin(shards=-1)), ('fin shards=5', _fin(shards=5)), ('fin training shards=5', _fin(shards=5, training=1)),
       ('fin training shards=0', _fin(shards=0, training=1)), ('fin training stat=NULL', _fin(stat=None, training=1)),
       ('fin n_nbt=-1', _fin(n_nbt=-1)),
       ('fin training running_mean without running_var', _fin(running_var=None, training=1)),
       ('fin eval running_mean=NULL', _fin(running_mean=None)), ('fin eval running_var=NULL', _fin(running_var=None)),
       ('fin eval without running statistics', _fin(running_mean=None, running_var=None)),
       ('fin training valid, b L = 0 < 2', _fin(training=1)),
       ('fin training without running statistics, b L = 0 < 2', _fin(training=1, running_mean=None, running_var=None))]
_FIN_ROWS = [(cid, {'fin': f}) for cid, f in FIN]
L_ROWS = [(f'L={v}', {'L': v}) for v in (0, 2, 4, 6, 8, 12, 16, 20)]
# the rows of the finding: 3 C must be a multiple of 4 and at most 4096 in the entries that run bn_fin_fill over 3 C rows
C_ROWS = [(f'C={v}', {'C': v}) for v in (0, 1, 2, 3, 4, 5, 6, 8, 1364, 1368)]
NEW_C = ('C=1', 'C=2', 'C=3', 'C=5', 'C=6', 'C=1368')
OLD_C = ('C=4', 'C=8', 'C=1364')


def _arr(n, null_at=None):
    a = (C.c_void_p * max(n, 1))()
    for i in range(n):
        a[i] = None if i == null_at else PTR
    return a


def _base():
    d = {k: PTR for k in ('x', 'y', 'p1', 'U', 'chan', 'gamma', 'out', 'resid', 'ln_w', 'ln_b', 'pre', 'stats', 'rec', 'prm',
                          'out_sums', 'g', 'dgamma', 'dx', 'dy', 'dV', 'bn_grad', 'g_in', 'dresid', 'w', 'z_next', 'dw', 's',
                          'gz', 'gz2', 'g_out', 'mix_out', 'W', 'bias', 'V', 'stat')}
    d.update(fin=_fin(), b=0, C=16, L=8, n_prev=0, prev='arr', dprev='arr', prev_null=None, w_stride=1, dg_shards=1,
             dw_shards=1, acc_resid=0, cols=(0, 1, 2, 3), n_cols=4, fc_act=0, n_src=1, srcs='arr', src_null=None, ldw=32,
             stat_shards=1)
    return d


def _prev(a, key, null_key):
    return None if a[key] is None else _arr(max(a['n_prev'], 0), a.get(null_key))


def call_fwd_next(lib, so, a):
    return so.bmnas_node_mix_fwd_next(a['x'], a['y'], a['p1'], a['U'], a['chan'], _fin_struct(lib, a['fin']), a['gamma'],
                                      a['out'], a['b'], a['C'], a['L'], lib.NO_DROP, lib.NO_DROP,
                                      _prev(a, 'prev', 'prev_null'), a['n_prev'], a['w'], a['w_stride'], a['z_next'], None)


def call_ln_fwd(lib, so, a):
    return so.bmnas_node_mix_ln_fwd(a['x'], a['y'], a['p1'], a['U'], a['chan'], _fin_struct(lib, a['fin']), a['gamma'],
                                    a['resid'], a['ln_w'], a['ln_b'], a['pre'], a['out'], a['stats'], a['b'], a['C'],
                                    a['L'], lib.NO_DROP, lib.NO_DROP, a['out_sums'], None)


def call_pre_fwd(lib, so, a):
    return so.bmnas_node_mix_pre_fwd(a['x'], a['y'], a['p1'], a['U'], a['chan'], _fin_struct(lib, a['fin']), a['gamma'],
                                     a['resid'], a['ln_w'], a['ln_b'], a['pre'], a['rec'], a['prm'], a['b'], a['C'],
                                     a['L'], lib.NO_DROP, lib.NO_DROP, None)


def call_bwd_next(lib, so, a):
    return so.bmnas_node_mix_bwd_next(a['g'], a['x'], a['y'], a['p1'], a['U'], a['chan'], a['gamma'], a['dgamma'],
                                      a['dg_shards'], 4, a['dx'], a['dy'], 0, a['dV'], a['bn_grad'], a['b'], a['C'],
                                      a['L'], lib.NO_DROP, lib.NO_DROP, _prev(a, 'prev', 'prev_null'),
                                      _prev(a, 'dprev', None), a['n_prev'], 0, a['w'], a['w_stride'], a['dw'],
                                      a['dw_shards'], 8, a['s'], a['gz'], a['gz2'], a['g_out'], None)


def call_ln_bwd(lib, so, a):
    return so.bmnas_node_mix_ln_bwd(a['g'], a['pre'], a['ln_w'], a['stats'], a['g_in'], a['dresid'], a['acc_resid'],
                                    a['x'], a['y'], a['p1'], a['U'], a['chan'], a['gamma'], a['dgamma'], a['dg_shards'],
                                    4, a['dx'], a['dy'], 0, a['dV'], a['bn_grad'], a['b'], a['C'], a['L'], lib.NO_DROP,
                                    lib.NO_DROP, None)


def _sel(lib, a):
    return lib.NodeSel((C.c_int * 4)(*a['cols']), a['n_cols'])


def call_sel_fwd(lib, so, a):
    return so.bmnas_node_mix_sel_act_fwd(a['x'], a['y'], a['p1'], a['U'], a['chan'], _fin_struct(lib, a['fin']),
                                         a['gamma'], _sel(lib, a), a['out'], a['b'], a['C'], a['L'], lib.NO_DROP,
                                         lib.NO_DROP, a['fc_act'], None)


def call_sel_bwd(lib, so, a):
    return so.bmnas_node_mix_sel_act_bwd(a['g'], a['x'], a['y'], a['p1'], a['U'], a['chan'], a['gamma'], _sel(lib, a),
                                         a['dgamma'], a['dg_shards'], 4, a['dx'], a['dy'], 0, a['dV'], a['bn_grad'],
                                         a['b'], a['C'], a['L'], lib.NO_DROP, lib.NO_DROP, a['fc_act'], None)


def call_conv_fwd(lib, so, a):
    srcs = None if a['srcs'] is None else _arr(max(a['n_src'], 0), a['src_null'])
    return so.bmnas_node_mix_conv_fwd(a['x'], a['y'], a['p1'], a['U'], a['chan'], _fin_struct(lib, a['fin']), a['gamma'],
                                      a['mix_out'], lib.NO_DROP, lib.NO_DROP, srcs, a['n_src'], a['W'], a['ldw'],
                                      a['bias'], a['V'], a['stat'], a['stat_shards'], a['b'], a['C'], a['L'], None)


def _nulls(names):
    return [(f'{n}=NULL', {n: None}) for n in names]


_HEAD = [('valid b=0', {}), ('b=-1', {'b': -1})]
_NEXT_F = [('n_prev=-1', {'n_prev': -1}), ('n_prev=5 valid', {'n_prev': 5}), ('n_prev=6 (LIMIT)', {'n_prev': 6}),
           ('n_prev=2 prev=NULL', {'n_prev': 2, 'prev': None}), ('n_prev=2 prev[1]=NULL', {'n_prev': 2, 'prev_null': 1}),
           ('n_prev=2 w=NULL', {'n_prev': 2, 'w': None}), ('n_prev=2 z_next=NULL', {'n_prev': 2, 'z_next': None}),
           ('n_prev=2 w_stride=0', {'n_prev': 2, 'w_stride': 0}),
           ('n_prev=0 prev / w / z_next NULL', {'prev': None, 'w': None, 'z_next': None})]
_NEXT_B = [('n_prev=-1', {'n_prev': -1}), ('n_prev=5 valid', {'n_prev': 5}), ('n_prev=6 (LIMIT)', {'n_prev': 6}),
           ('n_prev=0 g=NULL', {'g': None}), ('n_prev=2 g=NULL (nullable)', {'n_prev': 2, 'g': None}),
           ('n_prev=2 gz2=NULL (nullable)', {'n_prev': 2, 'gz2': None}),
           ('n_prev=2 prev[0]=NULL', {'n_prev': 2, 'prev_null': 0}), ('n_prev=2 dprev=NULL', {'n_prev': 2, 'dprev': None}),
           ('n_prev=2 dw=NULL', {'n_prev': 2, 'dw': None}), ('n_prev=2 s=NULL', {'n_prev': 2, 's': None}),
           ('n_prev=2 gz=NULL', {'n_prev': 2, 'gz': None}), ('n_prev=2 g_out=NULL', {'n_prev': 2, 'g_out': None}),
           ('n_prev=2 dw_shards=0', {'n_prev': 2, 'dw_shards': 0}), ('dgamma_shards=0', {'dg_shards': 0}),
           ('dgamma / dx / dy NULL (nullable)', {'dgamma': None, 'dx': None, 'dy': None})]
# two refused arguments: the first named wins
_ORDER_F = [('order: x=NULL and L=6 -> ARG', {'x': None, 'L': 6}), ('order: L=6 and C=5 -> SHAPE', {'L': 6, 'C': 5}),
            ('order: fin bn_w=NULL and C=5 -> ARG', {'fin': _fin(bn_w=None), 'C': 5}),
            ('order: x=NULL and C=5 -> ARG', {'x': None, 'C': 5})]

ENTRIES = {
    'bmnas_node_mix_fwd_next': (call_fwd_next, _HEAD + _nulls(['x', 'y', 'p1', 'U', 'chan', 'gamma', 'out']) + L_ROWS +
                                C_ROWS + _NEXT_F + _FIN_ROWS + _ORDER_F +
                                [('order: L=6 and n_prev=6 -> SHAPE', {'L': 6, 'n_prev': 6}),
                                 ('order: n_prev=6 and C=5 -> LIMIT', {'n_prev': 6, 'C': 5})]),
    'bmnas_node_mix_ln_fwd': (call_ln_fwd, _HEAD + _nulls(['x', 'y', 'p1', 'U', 'chan', 'gamma', 'resid', 'ln_w', 'ln_b',
                                                          'pre', 'out', 'stats']) +
                              [('out_sums=NULL (nullable)', {'out_sums': None})] + L_ROWS + C_ROWS + _FIN_ROWS + _ORDER_F),
    'bmnas_node_mix_pre_fwd': (call_pre_fwd, _HEAD + _nulls(['x', 'y', 'p1', 'U', 'chan', 'gamma', 'resid', 'ln_w', 'ln_b',
                                                            'pre', 'rec', 'prm']) + L_ROWS + C_ROWS + _FIN_ROWS + _ORDER_F),
    'bmnas_node_mix_bwd_next': (call_bwd_next, _HEAD + _nulls(['x', 'y', 'p1', 'U', 'chan', 'gamma', 'dV', 'bn_grad']) +
                                L_ROWS + C_ROWS + _NEXT_B + [('order: x=NULL and L=12 -> ARG', {'x': None, 'L': 12}),
                                                            ('order: L=12 and n_prev=6 -> SHAPE', {'L': 12, 'n_prev': 6})]),
    'bmnas_node_mix_ln_bwd': (call_ln_bwd, _HEAD + _nulls(['g', 'pre', 'ln_w', 'stats', 'x', 'y', 'p1', 'U', 'chan', 'gamma',
                                                          'dV', 'bn_grad']) +
                              [('g_in / dresid / dgamma / dx / dy NULL (nullable)',
                                {'g_in': None, 'dresid': None, 'dgamma': None, 'dx': None, 'dy': None}),
                               ('accumulate_resid without dresid', {'acc_resid': 1, 'dresid': None}),
                               ('dgamma_shards=0', {'dg_shards': 0})] + L_ROWS + C_ROWS +
                              [('b=129 (LIMIT)', {'b': 129, 'L': 16}), ('b=1 C=514 L=16 (LIMIT)', {'b': 1, 'C': 514, 'L': 16}),
                               ('b=1 C=3 (odd, LIMIT)', {'b': 1, 'C': 3}),
                               ('order: g=NULL and L=12 -> ARG', {'g': None, 'L': 12}),
                               ('order: L=12 and b=129 -> SHAPE', {'L': 12, 'b': 129})]),
    'bmnas_node_mix_sel_act_fwd': (call_sel_fwd, _HEAD + _nulls(['x', 'y', 'p1', 'U', 'chan', 'gamma', 'out']) + L_ROWS +
                                   C_ROWS + [('C=16', {'C': 16}), ('C=1376 (3 C = 4128)', {'C': 1376}),
                                             ('fc_act=1', {'fc_act': 1}), ('fc_act=2', {'fc_act': 2}),
                                             ('sel n=0', {'n_cols': 0}), ('sel n=5', {'n_cols': 5}),
                                             ('sel a column twice', {'cols': (0, 1, 1, 3)}),
                                             ('sel column >= n', {'cols': (0, 1, 2, 4)}),
                                             ('sel Sum alone, x / y only', {'cols': (0, -1, -1, -1), 'n_cols': 1, 'p1': None,
                                                                            'U': None, 'chan': None, 'C': 3, 'L': 12}),
                                             ('sel Sum alone, fin bn_w=NULL (ignored)',
                                              {'cols': (0, -1, -1, -1), 'n_cols': 1, 'fin': _fin(bn_w=None)}),
                                             ('sel no Sum: x / y NULL', {'cols': (-1, 0, 1, 2), 'n_cols': 3, 'x': None,
                                                                         'y': None})] + _FIN_ROWS +
                                   [('order: sel n=0 and gamma=NULL -> ARG', {'n_cols': 0, 'gamma': None}),
                                    ('order: gamma=NULL and C=5 -> ARG', {'gamma': None, 'C': 5}),
                                    ('order: C=5 (LIMIT) and x=NULL -> LIMIT', {'C': 5, 'x': None})]),
    'bmnas_node_mix_sel_act_bwd': (call_sel_bwd, _HEAD + _nulls(['g', 'x', 'y', 'p1', 'U', 'chan', 'gamma', 'dV', 'bn_grad']) +
                                   L_ROWS + C_ROWS + [('C=16', {'C': 16}), ('C=1376 (3 C = 4128)', {'C': 1376}),
                                                      ('fc_act=1', {'fc_act': 1}), ('fc_act=2', {'fc_act': 2}),
                                                      ('dgamma_shards=0', {'dg_shards': 0}),
                                                      ('dgamma / dx / dy NULL (nullable)',
                                                       {'dgamma': None, 'dx': None, 'dy': None}),
                                                      ('sel Sum alone, C 3', {'cols': (0, -1, -1, -1), 'n_cols': 1, 'p1': None,
                                                                              'U': None, 'chan': None, 'dV': None,
                                                                              'bn_grad': None, 'C': 3, 'L': 4}),
                                                      ('sel Sum alone, L=12', {'cols': (0, -1, -1, -1), 'n_cols': 1, 'L': 12})]),
    'bmnas_node_mix_conv_fwd': (call_conv_fwd, _HEAD + _nulls(['x', 'y', 'p1', 'U', 'chan', 'gamma', 'mix_out', 'srcs', 'W',
                                                              'bias', 'V']) +
                                [('stat=NULL with 1 shard', {'stat': None}), ('stat given with 0 shards', {'stat_shards': 0}),
                                 ('stat=NULL with 0 shards', {'stat': None, 'stat_shards': 0}),
                                 ('stat_shards=-1', {'stat_shards': -1, 'stat': None}),
                                 ('b=0: nothing else is looked at (C=5, L=6, n_src=9)', {'C': 5, 'L': 6, 'n_src': 9}),
                                 ('b=1 n_src=3 C=256 (LIMIT)', {'b': 1, 'n_src': 3, 'C': 256, 'L': 16, 'ldw': 1024}),
                                 ('b=1 C=16 (% 64, LIMIT)', {'b': 1, 'C': 16}), ('b=1 C=320 (LIMIT)', {'b': 1, 'C': 320}),
                                 ('b=1 L=12 (LIMIT)', {'b': 1, 'C': 64, 'L': 12, 'ldw': 128}),
                                 ('b=1 n_src=0 (LIMIT)', {'b': 1, 'C': 64, 'n_src': 0, 'ldw': 128}),
                                 ('b=1 n_src=4 (LIMIT)', {'b': 1, 'C': 64, 'n_src': 4, 'ldw': 512}),
                                 ('b=1024 C=64 L=16: 4096 workgroups (LIMIT)', {'b': 1024, 'C': 64, 'L': 16, 'ldw': 128}),
                                 ('b=1 C=64 ldw=124 (< K, SHAPE)', {'b': 1, 'C': 64, 'ldw': 124}),
                                 ('b=1 C=64 ldw=130 (% 4, SHAPE)', {'b': 1, 'C': 64, 'ldw': 130}),
                                 ('order: b=1 C=16 and ldw=2 -> LIMIT', {'b': 1, 'C': 16, 'ldw': 2}),
                                 ('order: b=1 x=NULL and C=16 -> ARG', {'b': 1, 'x': None, 'C': 16})]),
}


def _b_rows_ok(fn, a):
    """a row with b > 0 may be called only where the entry refuses it before its launch; the refusals restated"""
    if a['b'] <= 0:
        return True
    if fn == 'bmnas_node_mix_ln_bwd':
        if not all(a[k] for k in ('g', 'pre', 'ln_w', 'stats', 'x', 'y', 'p1', 'U', 'chan', 'gamma', 'dV', 'bn_grad')):
            return True
        C_, L = a['C'], a['L']
        return L not in (4, 8, 16) or a['b'] > 128 or C_ < 2 or C_ % 2 == 1 or C_ * L // 4 > 2048
    if fn == 'bmnas_node_mix_conv_fwd':
        if not all(a[k] for k in ('x', 'y', 'p1', 'U', 'chan', 'gamma', 'mix_out', 'srcs', 'W', 'bias', 'V')):
            return True
        C_, L, n = a['C'], a['L'], a['n_src']
        ok = (1 <= n <= 3 and L in (4, 8, 16) and C_ % 64 == 0 and C_ <= 256 and
              ((a['b'] * L + 15) // 16) * (C_ // 16) <= 256 and ((n + 1) * C_ // 16 + 3) // 4 <= 12)
        return not ok or a['ldw'] < (n + 1) * C_ or a['ldw'] % 4 != 0
    return False


def _codes(fn):
    lib, so = _lib()
    call, rows = ENTRIES[fn]
    got = {}
    for cid, over in rows:
        a = _base()
        a.update(over)
        assert _b_rows_ok(fn, a), (fn, cid)                        # nothing here may reach a launch
        assert cid not in got, (fn, cid)
        got[cid] = call(lib, so, a)
    return got


def record():
    return {fn: _codes(fn) for fn in ENTRIES}


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('fn', sorted(ENTRIES))
def test_entry_point_return_codes(fn):
    got, want = _codes(fn), _golden()[fn]
    assert sorted(got) == sorted(want), 'the case list and the recorded table differ: regenerate on purpose only'
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, f'{fn}: case -> (returned, recorded): {bad}'


def test_no_row_reached_a_launch():
    """a code > 0 is a hipError_t: a call that got as far as a launch"""
    g = _golden()
    assert sorted(g) == sorted(ENTRIES)
    assert all(code in (0, -1, -2, -3) for table in g.values() for code in table.values())
    for fn, table in g.items():
        for cid, over in ENTRIES[fn][1]:
            if over.get('b', 0) > 0:
                assert table[cid] < 0, (fn, cid)


FWD_FIN = ('bmnas_node_mix_fwd_next', 'bmnas_node_mix_ln_fwd', 'bmnas_node_mix_pre_fwd')


def test_the_forward_entries_refuse_what_bn_fin_fill_cannot_take():
    """four adjacent channels per thread and float4 LDS stores at sc + 4 t, sh = sc + 3 C: (3 C) % 4 == 0; scale | shift
    of 3 C rows in LDS: 3 C <= 4096, the limit bmnas_node_mix_sel_ok states for the same arrays.  The backward entries
    read chan per channel and take any C (bmnas_node_mix_ln_bwd: any even C)."""
    g = _golden()
    for fn in FWD_FIN:
        assert [g[fn][k] for k in NEW_C] == [-3] * len(NEW_C), fn
        # (bmnas_node_mix_pre_fwd: bmnas_lazy_ln_ok keeps C L <= 4096, so C 1364 was and is beyond its limit)
        assert [g[fn][k] for k in OLD_C] == ([0, 0, -3] if fn == 'bmnas_node_mix_pre_fwd' else [0, 0, 0]), fn
        assert g[fn]['C=0'] == -1, fn
    t = g['bmnas_node_mix_bwd_next']
    assert [t[k] for k in NEW_C + OLD_C] == [0] * 9 and t['C=0'] == -1
    for fn in ('bmnas_node_mix_sel_act_fwd', 'bmnas_node_mix_sel_act_bwd'):      # C % 16 with a conv term, 3 C <= 4096
        assert [g[fn][k] for k in NEW_C + OLD_C] == [-3] * 9 and g[fn]['C=16'] == 0 and g[fn]['C=1376 (3 C = 4128)'] == -3, fn


def test_the_pinned_order_and_differences_between_entry_points():
    g = _golden()
    Ls = [f'L={v}' for v in (0, 2, 4, 6, 8, 12, 16, 20)]
    for fn in ('bmnas_node_mix_fwd_next', 'bmnas_node_mix_ln_fwd'):
        assert [g[fn][k] for k in Ls] == [0, -2, 0, -2, 0, 0, 0, -2], fn
    for fn in ('bmnas_node_mix_pre_fwd', 'bmnas_node_mix_bwd_next', 'bmnas_node_mix_ln_bwd'):
        assert [g[fn][k] for k in Ls] == [-2, -2, 0, -2, 0, -2, 0, -2], fn
    for fn in ('bmnas_node_mix_sel_act_fwd', 'bmnas_node_mix_sel_act_bwd'):      # one limit function: LIMIT, not SHAPE
        assert [g[fn][k] for k in Ls] == [-3, -3, 0, -3, 0, -3, 0, -3], fn
    assert g['bmnas_node_mix_sel_act_fwd']['sel Sum alone, x / y only'] == 0     # L 12, C 3: no conv, no attention
    assert g['bmnas_node_mix_sel_act_bwd']['sel Sum alone, L=12'] == 0
    for fn in FWD_FIN:
        t = g[fn]
        assert t['order: x=NULL and L=6 -> ARG'] == -1 and t['order: L=6 and C=5 -> SHAPE'] == -2, fn
        assert t['order: fin bn_w=NULL and C=5 -> ARG'] == -1 and t['order: x=NULL and C=5 -> ARG'] == -1, fn
        assert t['fin shards=5'] == -3 and t['fin training shards=0'] == -1 and t['fin off, every field 0'] == 0, fn
        assert t['fin training valid, b L = 0 < 2'] == -1 and t['fin eval without running statistics'] == -1, fn
    t = g['bmnas_node_mix_fwd_next']
    assert t['n_prev=6 (LIMIT)'] == -3 and t['n_prev=5 valid'] == 0 and t['n_prev=-1'] == -1
    assert t['order: L=6 and n_prev=6 -> SHAPE'] == -2 and t['order: n_prev=6 and C=5 -> LIMIT'] == -3
    assert t['n_prev=2 prev[1]=NULL'] == -1 and t['n_prev=0 prev / w / z_next NULL'] == 0
    t = g['bmnas_node_mix_bwd_next']
    assert t['n_prev=6 (LIMIT)'] == -3 and t['order: L=12 and n_prev=6 -> SHAPE'] == -2
    assert t['n_prev=0 g=NULL'] == -1 and t['n_prev=2 g=NULL (nullable)'] == 0 and t['n_prev=2 gz=NULL'] == -1
    t = g['bmnas_node_mix_ln_bwd']
    assert t['b=129 (LIMIT)'] == -3 and t['b=1 C=514 L=16 (LIMIT)'] == -3 and t['order: L=12 and b=129 -> SHAPE'] == -2
    assert t['accumulate_resid without dresid'] == -1
    t = g['bmnas_node_mix_conv_fwd']
    assert t['b=1 n_src=3 C=256 (LIMIT)'] == -3 and t['b=1 C=64 ldw=124 (< K, SHAPE)'] == -2
    assert t['order: b=1 C=16 and ldw=2 -> LIMIT'] == -3 and t['stat=NULL with 1 shard'] == -1


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))
    json.dump(record(), sys.stdout, indent=1, sort_keys=True)
    print()
