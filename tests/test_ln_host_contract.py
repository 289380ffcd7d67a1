"""CPU: the host contract of the mixed-sum and per-sample LayerNorm entry points that had no table — bmnas_mixsum_fwd,
_bwd, _pair_fwd, _pair_bwd, _pair_bwd_x (csrc/mixsum.hip), bmnas_cat_ln_fwd, _bwd, bmnas_ln_affine_bwd, _multi
(csrc/layernorm.hip), bmnas_bn_relu_ln_fwd_pair, _bwd_pair and through them the two plain forms (csrc/bnmix.hip),
bmnas_node_mix_lnp_bwd, bmnas_mixsum_pair_fwd_lazy, _bwd_lazy and bmnas_lazy_ln_ok / _parts (csrc/lazyln.hip): which
return code each gives for a refused argument and in which order (BMNAS_E_ARG -1, BMNAS_E_SHAPE -2, BMNAS_E_LIMIT -3).

Every call here returns before any HIP call: b = 0 (n_elem = 0) with valid arguments, or exactly one refused argument
(the order rows carry two, and show which one wins).  A row with b > 0 (n_elem > 0) is one whose refusal the entry makes
AFTER its b == 0 return — a null element of a pointer list, a sample too wide for the kernel family, an aliased
destination: _late_refusal states those refusals again in Python, and a row they would let through is not called.  The
pointers are host buffers that are never dereferenced as tensors.

The expected values in tests/golden/ln_host_contract.json were recorded from the library of commit 0c58601 ("One
definition of the LayerNorm formulas and epsilon"), the parent of the commit that moved these entries' launches onto
csrc/launch.hpp (dispatch_range / dispatch_of / ln_launch_shape, fill_ptrs, fin_for): that commit had to reproduce the
table without a regenerated row.  Regenerate with
    python tests/test_ln_host_contract.py > tests/golden/ln_host_contract.json
only when the contract is changed on purpose."""
import ctypes as C
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'ln_host_contract.json')

_BUF = (C.c_float * 4096)()        # one host buffer stands for every tensor argument
PTR = C.addressof(_BUF)
_PP = C.POINTER(C.c_void_p)


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


# the to_fin rows of the existing tables, through bmnas_bn_relu_ln_fwd_pair
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
N_IN_ROWS = [(f'n_in={v}', {'n_in': v}) for v in (0, 1, 15, 16, 17)]


def _arr(n, null_at=None, same=None):
    """n distinct pointers into _BUF; element null_at is NULL; same = (j, k): element j repeats element k"""
    a = (C.c_void_p * max(n, 1))()
    for i in range(n):
        a[i] = None if i == null_at else PTR + 64 * (i + 1)
    if same is not None:
        a[same[0]] = a[same[1]]
    return a


def _list(a, key, n, null_key=None, same_key=None):
    return None if a[key] is None else _arr(max(n, 0), a.get(null_key), a.get(same_key))


def _base():
    d = {k: PTR for k in ('w', 'w2', 'out', 'out2', 'g', 'g2', 'dw', 'dw2', 'h', 'gh', 'gz', 'gz2', 'resid', 'ln_w', 'ln_b',
                          'stats', 'out_sums', 'dresid', 'dln_w', 'dln_b', 'gscale', 'scrub', 'U', 'chan', 'o', 'z', 'dV',
                          'bn_grad', 'g_full', 'pre', 'lnp0', 'lnp1', 'g_in', 'x', 'y', 'p1', 'gamma', 'dgamma', 'dx', 'dy',
                          'bn_part', 'last_out', 'last_sums', 'rec', 'prm')}
    d.update(xs='arr', dxs='arr', xs_null=None, dxs_same=None, n_in=2, w_stride=1, w2_stride=1, dw_shards=1, n_elem=0,
             g_more='arr', w_more='arr', g_more_null=None, w_more_null=None, n_more=1,
             srcs='arr', dsrcs='arr', src_null=None, n_src=1, b=0, C=16, L=8, relu=0, prenorm=0, scrub_n=0,
             fin=_fin(), n_prev=0, acc_resid=0, n0=1, n1=0, dg_shards=1,
             last='struct', last_null=None, lazy='arr', lazy_null=None, lnpart='arr', lnpart_null=None,
             lnpart_stride='arr', stride=4, n_lazy=1,
             # bmnas_ln_affine_bwd_multi: every list, and what element 1 of a list holds
             n_prob=2, lists={}, elem1={})
    return d


def call_mixsum_fwd(lib, so, a):
    return so.bmnas_mixsum_fwd(_list(a, 'xs', a['n_in'], 'xs_null'), a['n_in'], a['w'], a['w_stride'], a['out'],
                               a['n_elem'], None)


def call_mixsum_bwd(lib, so, a):
    return so.bmnas_mixsum_bwd(_list(a, 'xs', a['n_in'], 'xs_null'), _list(a, 'dxs', a['n_in']), a['n_in'], a['w'],
                               a['w_stride'], a['g'], a['g2'], a['dw'], a['dw_shards'], 8, 0, a['n_elem'], None)


def call_pair_fwd(lib, so, a):
    return so.bmnas_mixsum_pair_fwd(_list(a, 'xs', a['n_in'], 'xs_null'), a['n_in'], a['w'], a['w_stride'], a['w2'],
                                    a['w2_stride'], a['out'], a['out2'], a['n_elem'], None)


def call_pair_bwd(lib, so, a):
    return so.bmnas_mixsum_pair_bwd(_list(a, 'xs', a['n_in'], 'xs_null'), _list(a, 'dxs', a['n_in']), a['n_in'], a['w'],
                                    a['w_stride'], a['w2'], a['w2_stride'], a['h'], a['gh'], a['gz'], a['gz2'], a['dw'],
                                    a['dw2'], a['dw_shards'], 8, 0, a['n_elem'], None)


def call_pair_bwd_x(lib, so, a):
    return so.bmnas_mixsum_pair_bwd_x(_list(a, 'xs', a['n_in'], 'xs_null'), _list(a, 'dxs', a['n_in']), a['n_in'], a['w'],
                                      a['w_stride'], a['w2'], a['w2_stride'], a['h'], a['gh'], a['gz'], a['gz2'],
                                      a['dw'], a['dw2'], a['dw_shards'], 8, 0,
                                      _list(a, 'g_more', a['n_more'], 'g_more_null'),
                                      _list(a, 'w_more', a['n_more'], 'w_more_null'), a['n_more'], a['n_elem'], None)


def call_cat_ln_fwd(lib, so, a):
    return so.bmnas_cat_ln_fwd(_list(a, 'srcs', a['n_src'], 'src_null'), a['n_src'], a['resid'], a['ln_w'], a['ln_b'],
                               a['out'], a['stats'], a['b'], a['C'], a['L'], a['relu'], a['out_sums'], None)


def call_cat_ln_bwd(lib, so, a):
    return so.bmnas_cat_ln_bwd(a['g'], _list(a, 'srcs', a['n_src'], 'src_null'), a['n_src'], a['resid'], a['ln_w'],
                               a['ln_b'], a['stats'], _list(a, 'dsrcs', a['n_src']), a['dresid'], 0, a['dln_w'],
                               a['dln_b'], a['b'], a['C'], a['L'], a['relu'], a['scrub'], a['scrub_n'], None)


def call_ln_affine(lib, so, a):
    return so.bmnas_ln_affine_bwd(a['g'], a['gscale'], _list(a, 'srcs', a['n_src'], 'src_null'), a['n_src'], a['resid'],
                                  a['ln_w'], a['ln_b'], a['stats'], a['dln_w'], a['dln_b'], a['b'], a['C'], a['L'],
                                  a['relu'], a['prenorm'], None)


_MULTI_PTR = ('g', 'gscale', 'resid', 'ln_w', 'ln_b', 'stats', 'dln_w', 'dln_b')
_MULTI_INT = ('n_src', 'C', 'relu', 'prenorm')


def call_ln_affine_multi(lib, so, a):
    """a['lists'][name] = None: the whole list is NULL; a['elem1'][name]: element 1 of that list"""
    n = max(a['n_prob'], 0)
    keep = []

    def plist(name):
        if a['lists'].get(name, 'arr') is None:
            return None
        arr = (C.c_void_p * max(n, 1))(*[PTR] * n)
        if n > 1 and name in a['elem1']:
            arr[1] = a['elem1'][name]
        return arr

    def ilist(name, v):
        if a['lists'].get(name, 'arr') is None:
            return None
        arr = (C.c_int * max(n, 1))(*[v] * n)
        if n > 1 and name in a['elem1']:
            arr[1] = a['elem1'][name]
        return arr

    if a['lists'].get('srcs', 'arr') is None:
        srcs = None
    else:
        keep = [_arr(1) for _ in range(n)]
        if n > 1 and 'srcs[0]' in a['elem1']:
            keep[1][0] = a['elem1']['srcs[0]']
        srcs = (_PP * max(n, 1))(*[C.cast(k, _PP) for k in keep])
        if n > 1 and 'srcs' in a['elem1']:
            srcs[1] = C.cast(a['elem1']['srcs'], _PP)
    return so.bmnas_ln_affine_bwd_multi(a['n_prob'], plist('g'), plist('gscale'), srcs, ilist('n_src', 1), plist('resid'),
                                        plist('ln_w'), plist('ln_b'), plist('stats'), plist('dln_w'), plist('dln_b'),
                                        a['b'], ilist('C', a['C']), a['L'], ilist('relu', a['relu']),
                                        ilist('prenorm', a['prenorm']), None)


def call_brl_fwd_pair(lib, so, a):
    return so.bmnas_bn_relu_ln_fwd_pair(a['U'], a['chan'], _fin_struct(lib, a['fin']), a['resid'], a['ln_w'], a['ln_b'],
                                        a['o'], a['out'], a['stats'], a['b'], a['C'], a['L'], lib.NO_DROP, a['out_sums'],
                                        _list(a, 'xs', a['n_prev'], 'xs_null'), a['n_prev'], a['w'], a['w_stride'],
                                        a['w2'], a['w2_stride'], a['h'], a['z'], None)


def call_brl_fwd(lib, so, a):
    return so.bmnas_bn_relu_ln_fwd(a['U'], a['chan'], _fin_struct(lib, a['fin']), a['resid'], a['ln_w'], a['ln_b'],
                                   a['o'], a['out'], a['stats'], a['b'], a['C'], a['L'], lib.NO_DROP, a['out_sums'], None)


def call_brl_bwd_pair(lib, so, a):
    return so.bmnas_bn_relu_ln_bwd_pair(a['g'], a['o'], a['resid'], a['ln_w'], a['stats'], a['U'], a['chan'], a['dV'],
                                        a['bn_grad'], a['dresid'], a['acc_resid'], a['b'], a['C'], a['L'], lib.NO_DROP,
                                        _list(a, 'xs', a['n_prev'], 'xs_null'),
                                        _list(a, 'dxs', a['n_prev'], None, 'dxs_same'), a['n_prev'], 0, a['out'], a['w'],
                                        a['w_stride'], a['w2'], a['w2_stride'], a['h'], a['gh'], a['gz'], a['gz2'],
                                        a['dw'], a['dw2'], a['dw_shards'], 8, a['g_full'], None)


def call_brl_bwd(lib, so, a):
    return so.bmnas_bn_relu_ln_bwd(a['g'], a['o'], a['resid'], a['ln_w'], a['stats'], a['U'], a['chan'], a['dV'],
                                   a['bn_grad'], a['dresid'], a['acc_resid'], a['b'], a['C'], a['L'], lib.NO_DROP, None)


def call_lnp_bwd(lib, so, a):
    return so.bmnas_node_mix_lnp_bwd(a['g'], a['pre'], a['ln_w'], a['stats'], a['lnp0'], a['n0'], a['lnp1'], a['n1'],
                                     a['g_in'], a['dresid'], a['acc_resid'], a['x'], a['y'], a['p1'], a['U'], a['chan'],
                                     a['gamma'], a['dgamma'], a['dg_shards'], 4, a['dx'], a['dy'], 0, a['dV'],
                                     a['bn_grad'], a['b'], a['C'], a['L'], lib.NO_DROP, lib.NO_DROP, a['bn_part'], None)


_LAZY_FIELDS = ('pre', 'rec', 'prm', 'ln_w', 'ln_b', 'stats')


def _lazy(lib, null=None):
    return lib.LazyLn(*[None if f == null else PTR for f in _LAZY_FIELDS])


def call_fwd_lazy(lib, so, a):
    last = None if a['last'] is None else C.byref(_lazy(lib, a['last_null']))
    return so.bmnas_mixsum_pair_fwd_lazy(_list(a, 'xs', a['n_in'], 'xs_null'), a['n_in'], a['w'], a['w_stride'], a['w2'],
                                         a['w2_stride'], last, a['last_out'], a['last_sums'], a['out'], a['out2'],
                                         a['b'], a['C'], a['L'], None)


def call_bwd_lazy(lib, so, a):
    n = max(a['n_lazy'], 1)
    lazy = None if a['lazy'] is None else (lib.LazyLn * n)(*[_lazy(lib, a['lazy_null'] if t == 0 else None)
                                                            for t in range(n)])
    stride = None if a['lnpart_stride'] is None else (C.c_int * n)(*[a['stride']] * n)
    return so.bmnas_mixsum_pair_bwd_lazy(_list(a, 'xs', a['n_in'], 'xs_null'),
                                         _list(a, 'dxs', a['n_in'], None, 'dxs_same'), a['n_in'], a['w'], a['w_stride'],
                                         a['w2'], a['w2_stride'], a['h'], a['gh'], a['gz'], a['gz2'], a['dw'], a['dw2'],
                                         a['dw_shards'], 8, 0, lazy, _list(a, 'lnpart', n, 'lnpart_null'), stride,
                                         a['n_lazy'], a['g_full'], a['b'], a['C'], a['L'], None)


def _nulls(names):
    return [(f'{n}=NULL', {n: None}) for n in names]


def _nullable(names):
    return [(f'{n}=NULL (nullable)', {n: None}) for n in names]


_ELEM = [('n_elem=-4', {'n_elem': -4}), ('n_elem=2 (% 4)', {'n_elem': 2}), ('n_elem=6 (% 4)', {'n_elem': 6}),
         ('n_elem=4 xs[1]=NULL', {'n_elem': 4, 'xs_null': 1}), ('w_stride=0', {'w_stride': 0})]
_DW = [('dw without dw2', {'dw2': None}), ('dw2 without dw', {'dw': None}), ('dw and dw2 NULL (no dots)', {'dw': None, 'dw2': None}),
       ('dw_shards=0', {'dw_shards': 0})]
_PAIR_B = (_nulls(['xs', 'dxs', 'w', 'w2', 'h', 'gz']) + _nullable(['gh', 'gz2']) + _DW +
           [('w2_stride=0', {'w2_stride': 0})] + N_IN_ROWS + _ELEM +
           [('order: dw without dw2 and n_in=16 -> ARG', {'dw2': None, 'n_in': 16}),
            ('order: n_in=16 and n_elem=2 -> LIMIT', {'n_in': 16, 'n_elem': 2}),
            ('order: n_elem=2 and xs[0]=NULL -> SHAPE', {'n_elem': 2, 'xs_null': 0})])
_CAT = ([('n_src=0', {'n_src': 0}), ('n_src=4', {'n_src': 4, 'resid': None}), ('n_src=5 (LIMIT)', {'n_src': 5, 'resid': None}),
         ('resid with n_src=2', {'n_src': 2}), ('n_src=2 resid=NULL', {'n_src': 2, 'resid': None}),
         ('b=-1', {'b': -1}), ('C=0', {'C': 0}), ('C=3 L=2 (C L % 4)', {'C': 3, 'L': 2}), ('C=3 L=4', {'C': 3, 'L': 4})] +
        L_ROWS +
        [('b=1 srcs[0]=NULL', {'b': 1, 'src_null': 0}),
         ('b=1 C=8196 L=4: 8196 float4 > 16 x 512 (LIMIT)', {'b': 1, 'C': 8196, 'L': 4}),
         ('b=257 C=4100 L=4: 4100 float4 > 16 x 256 (LIMIT)', {'b': 257, 'C': 4100, 'L': 4}),
         ('order: n_src=5 and resid -> LIMIT', {'n_src': 5}),
         ('order: resid with n_src=2 and C=3 L=2 -> ARG', {'n_src': 2, 'C': 3, 'L': 2}),
         ('order: out/g=NULL and n_src=5 -> ARG', {'out': None, 'g': None, 'n_src': 5})])
_PREV = [('n_prev=-1', {'n_prev': -1}), ('n_prev=1', {'n_prev': 1}), ('n_prev=15', {'n_prev': 15}),
         ('n_prev=16 (LIMIT)', {'n_prev': 16}), ('n_prev=17 (LIMIT)', {'n_prev': 17}),
         ('n_prev=2 xs=NULL', {'n_prev': 2, 'xs': None}), ('n_prev=2 xs[1]=NULL', {'n_prev': 2, 'xs_null': 1}),
         ('n_prev=2 w=NULL', {'n_prev': 2, 'w': None}), ('n_prev=2 w2=NULL', {'n_prev': 2, 'w2': None}),
         ('n_prev=2 h=NULL', {'n_prev': 2, 'h': None}), ('n_prev=2 w_stride=0', {'n_prev': 2, 'w_stride': 0}),
         ('n_prev=2 w2_stride=0', {'n_prev': 2, 'w2_stride': 0}),
         ('n_prev=2 C=256 L=16: 1024 float4 > 256 (LIMIT)', {'n_prev': 2, 'C': 256, 'L': 16}),
         ('n_prev=2 b=129 (LIMIT)', {'n_prev': 2, 'b': 129}),
         ('order: n_prev=16 and xs[0]=NULL -> LIMIT', {'n_prev': 16, 'xs_null': 0}),
         ('order: n_prev=2 xs[0]=NULL and L=6 -> ARG', {'n_prev': 2, 'xs_null': 0, 'L': 6}),
         ('order: n_prev=16 and L=6 -> LIMIT', {'n_prev': 16, 'L': 6})]
_BRL_F = (_nulls(['U', 'chan', 'resid', 'ln_w', 'ln_b', 'o', 'out', 'stats']) + _nullable(['out_sums']) +
          [('b=-1', {'b': -1}), ('C=0', {'C': 0}), ('C=6 (% 4)', {'C': 6}),
           ('b=1 C=2052 L=4: C > 4 x 512 (LIMIT)', {'b': 1, 'C': 2052, 'L': 4}),
           ('b=257 C=1028 L=4: C > 4 x 256 (LIMIT)', {'b': 257, 'C': 1028, 'L': 4}),
           ('b=1 C=2048 L=16: 8192 float4 > 8 x 512 (LIMIT)', {'b': 1, 'C': 2048, 'L': 16}),
           ('order: U=NULL and L=6 -> ARG', {'U': None, 'L': 6}),
           ('order: L=6 and fin bn_w=NULL -> SHAPE', {'L': 6, 'fin': _fin(bn_w=None)})] + L_ROWS + _FIN_ROWS)
_BRL_B = (_nulls(['g', 'o', 'resid', 'ln_w', 'stats', 'U', 'chan', 'dV', 'bn_grad']) +
          [('b=-1', {'b': -1}), ('C=0', {'C': 0}), ('C=6', {'C': 6}), ('dresid=NULL (nullable)', {'dresid': None}),
           ('accumulate_resid without dresid', {'acc_resid': 1, 'dresid': None}),
           ('b=1 C=2304 L=16: 9216 float4 > 8 x 512 (LIMIT)', {'b': 1, 'C': 2304, 'L': 16}),
           ('order: o=NULL and L=12 -> ARG', {'o': None, 'L': 12}),
           ('order: L=12 and accumulate_resid without dresid -> SHAPE', {'L': 12, 'acc_resid': 1, 'dresid': None})] + L_ROWS)

ENTRIES = {
    'bmnas_mixsum_fwd': (call_mixsum_fwd, [('valid n_elem=0', {})] + _nulls(['xs', 'w', 'out']) + N_IN_ROWS + _ELEM +
                         [('order: out=NULL and n_in=17 -> ARG', {'out': None, 'n_in': 17}),
                          ('order: n_in=17 and n_elem=2 -> LIMIT', {'n_in': 17, 'n_elem': 2}),
                          ('order: n_elem=2 and xs[0]=NULL -> SHAPE', {'n_elem': 2, 'xs_null': 0})]),
    'bmnas_mixsum_bwd': (call_mixsum_bwd, [('valid n_elem=0', {})] + _nulls(['xs', 'dxs', 'w', 'g']) +
                         _nullable(['g2', 'dw']) + [('dw_shards=0', {'dw_shards': 0})] + N_IN_ROWS + _ELEM +
                         [('order: g=NULL and n_in=17 -> ARG', {'g': None, 'n_in': 17})]),
    'bmnas_mixsum_pair_fwd': (call_pair_fwd, [('valid n_elem=0', {})] + _nulls(['xs', 'w', 'w2', 'out', 'out2']) +
                              [('w2_stride=0', {'w2_stride': 0})] + N_IN_ROWS + _ELEM),
    'bmnas_mixsum_pair_bwd': (call_pair_bwd, [('valid n_elem=0', {})] + _PAIR_B),
    'bmnas_mixsum_pair_bwd_x': (call_pair_bwd_x, [('valid n_elem=0', {})] + _PAIR_B +
                                [('n_more=0 (the plain entry)', {'n_more': 0}),
                                 ('n_more=0 g_more / w_more NULL', {'n_more': 0, 'g_more': None, 'w_more': None}),
                                 ('n_more=0 n_in=16 (LIMIT)', {'n_more': 0, 'n_in': 16}),
                                 ('n_more=2', {'n_more': 2}), ('n_more=3 (LIMIT)', {'n_more': 3}),
                                 ('n_more=-1 (LIMIT)', {'n_more': -1}), ('g_more=NULL', {'g_more': None}),
                                 ('w_more=NULL', {'w_more': None}),
                                 ('n_elem=4 g_more[0]=NULL', {'n_elem': 4, 'g_more_null': 0}),
                                 ('n_elem=4 n_more=2 w_more[1]=NULL', {'n_elem': 4, 'n_more': 2, 'w_more_null': 1}),
                                 ('order: g_more=NULL and n_more=3 -> ARG', {'g_more': None, 'n_more': 3}),
                                 ('order: n_more=3 and n_elem=2 -> LIMIT', {'n_more': 3, 'n_elem': 2})]),
    'bmnas_cat_ln_fwd': (call_cat_ln_fwd, [('valid b=0', {})] + _nulls(['srcs', 'ln_w', 'ln_b', 'out', 'stats']) +
                         _nullable(['resid', 'out_sums']) + _CAT),
    'bmnas_cat_ln_bwd': (call_cat_ln_bwd, [('valid b=0', {})] + _nulls(['g', 'srcs', 'ln_w', 'ln_b', 'stats', 'dsrcs']) +
                         _nullable(['resid', 'dresid']) + _CAT +
                         [('dln_w without dln_b', {'dln_b': None}), ('dln_b without dln_w', {'dln_w': None}),
                          ('dln_w and dln_b NULL', {'dln_w': None, 'dln_b': None}),
                          ('scrub_n=-4', {'scrub_n': -4}), ('scrub_n=8', {'scrub_n': 8}), ('scrub_n=6 (% 4)', {'scrub_n': 6}),
                          ('scrub_n=8 scrub=NULL', {'scrub_n': 8, 'scrub': None}),
                          ('scrub_n=0 scrub=NULL', {'scrub': None}),
                          ('order: scrub_n=6 and n_src=5 -> ARG', {'scrub_n': 6, 'n_src': 5, 'resid': None})]),
    'bmnas_ln_affine_bwd': (call_ln_affine, [('valid b=0', {})] + _nulls(['g', 'srcs', 'dln_w', 'dln_b']) +
                            _nullable(['gscale', 'resid', 'ln_w', 'ln_b']) +
                            [('stats=NULL', {'stats': None}), ('stats=NULL prenorm', {'stats': None, 'prenorm': 1}),
                             ('relu ln_w=NULL', {'relu': 1, 'ln_w': None}), ('relu ln_b=NULL', {'relu': 1, 'ln_b': None}),
                             ('relu', {'relu': 1}), ('n_src=0', {'n_src': 0}), ('n_src=4', {'n_src': 4, 'resid': None}),
                             ('n_src=5 (LIMIT)', {'n_src': 5, 'resid': None}), ('resid with n_src=2', {'n_src': 2}),
                             ('srcs[0]=NULL', {'src_null': 0}), ('b=-1', {'b': -1}), ('C=0', {'C': 0}),
                             ('C=3 L=2 (C L % 4)', {'C': 3, 'L': 2}),
                             ('order: b=-1 and g=NULL -> ARG', {'b': -1, 'g': None}),
                             ('order: n_src=5 and C=3 L=2 -> LIMIT', {'n_src': 5, 'resid': None, 'C': 3, 'L': 2}),
                             ('order: C=3 L=2 and srcs[0]=NULL -> SHAPE', {'C': 3, 'L': 2, 'src_null': 0})] + L_ROWS),
    'bmnas_ln_affine_bwd_multi': (call_ln_affine_multi, [('valid b=0', {})] +
                                  [(f'n_prob={v}', {'n_prob': v}) for v in (0, 1, 8, 9)] +
                                  [(f'{n} list NULL', {'lists': {n: None}})
                                   for n in ('g', 'srcs', 'n_src', 'dln_w', 'dln_b', 'C', 'relu', 'prenorm')] +
                                  [(f'{n} list NULL (nullable)', {'lists': {n: None}})
                                   for n in ('gscale', 'resid', 'ln_w', 'ln_b')] +
                                  [('stats list NULL', {'lists': {'stats': None}}),
                                   ('stats list NULL, prenorm', {'lists': {'stats': None}, 'prenorm': 1}),
                                   ('relu, ln_w list NULL', {'lists': {'ln_w': None}, 'relu': 1}),
                                   ('g[1]=NULL', {'elem1': {'g': None}}), ('srcs[1]=NULL', {'elem1': {'srcs': None}}),
                                   ('srcs[1][0]=NULL', {'elem1': {'srcs[0]': None}}),
                                   ('dln_b[1]=NULL', {'elem1': {'dln_b': None}}),
                                   ('stats[1]=NULL', {'elem1': {'stats': None}}),
                                   ('stats[1]=NULL prenorm[1]', {'elem1': {'stats': None, 'prenorm': 1}}),
                                   ('n_src[1]=0', {'elem1': {'n_src': 0}}), ('C[1]=3 L=2', {'elem1': {'C': 3}, 'L': 2}),
                                   ('relu[1] ln_w[1]=NULL', {'elem1': {'relu': 1, 'ln_w': None}}),
                                   ('b=-1', {'b': -1}),
                                   ('order: n_prob=9 and g list NULL -> ARG', {'n_prob': 9, 'lists': {'g': None}})]),
    'bmnas_bn_relu_ln_fwd_pair': (call_brl_fwd_pair, [('valid b=0', {})] + _BRL_F + _PREV +
                                  [('n_prev=2 z=NULL', {'n_prev': 2, 'z': None}),
                                   ('n_prev=0 xs / w / w2 / h / z NULL', {'xs': None, 'w': None, 'w2': None, 'h': None,
                                                                          'z': None})]),
    'bmnas_bn_relu_ln_fwd': (call_brl_fwd, [('valid b=0', {})] + _BRL_F),
    'bmnas_bn_relu_ln_bwd_pair': (call_brl_bwd_pair, [('valid b=0', {})] + _BRL_B + _PREV +
                                  [('n_prev=2 g=NULL (nullable)', {'n_prev': 2, 'g': None}),
                                   ('n_prev=2 gh / gz2 NULL (nullable)', {'n_prev': 2, 'gh': None, 'gz2': None})] +
                                  [(f'n_prev=2 {n}=NULL', {'n_prev': 2, n: None})
                                   for n in ('dxs', 'out', 'gz', 'dw', 'dw2', 'g_full')] +
                                  [('n_prev=2 dw_shards=0', {'n_prev': 2, 'dw_shards': 0}),
                                   ('n_prev=3 dxs[2]=dxs[0]', {'n_prev': 3, 'dxs_same': (2, 0)}),
                                   ('n_prev=3 dxs[2]=dxs[1]', {'n_prev': 3, 'dxs_same': (2, 1)}),
                                   ('order: n_prev=3 dxs[2]=dxs[0] and L=12 -> ARG', {'n_prev': 3, 'dxs_same': (2, 0),
                                                                                      'L': 12})]),
    'bmnas_bn_relu_ln_bwd': (call_brl_bwd, [('valid b=0', {})] + _BRL_B),
    'bmnas_node_mix_lnp_bwd': (call_lnp_bwd, [('valid b=0', {})] +
                               _nulls(['g', 'pre', 'ln_w', 'stats', 'x', 'y', 'p1', 'U', 'chan', 'gamma', 'dV', 'bn_grad']) +
                               _nullable(['g_in', 'dresid', 'dgamma', 'dx', 'dy', 'bn_part']) +
                               [('b=-1', {'b': -1}), ('C=0', {'C': 0}), ('dgamma_shards=0', {'dg_shards': 0}),
                                ('n0=-1', {'n0': -1}), ('n1=-1', {'n1': -1}), ('n0=0 n1=0', {'n0': 0}),
                                ('n0=1 lnp0=NULL', {'lnp0': None}), ('n0=0 n1=1 lnp0=NULL', {'n0': 0, 'n1': 1, 'lnp0': None}),
                                ('n1=1 lnp1=NULL', {'n1': 1, 'lnp1': None}), ('n0=1 n1=0 lnp1=NULL', {'lnp1': None}),
                                ('n0=300', {'n0': 300}),
                                ('accumulate_resid without dresid', {'acc_resid': 1, 'dresid': None}),
                                ('C=256 L=16: 4 parts', {'C': 256, 'L': 16}),
                                ('C=260 L=16: 5 parts (LIMIT)', {'C': 260, 'L': 16}),
                                ('order: g=NULL and L=12 -> ARG', {'g': None, 'L': 12}),
                                ('order: accumulate_resid without dresid and L=12 -> ARG',
                                 {'acc_resid': 1, 'dresid': None, 'L': 12}),
                                ('order: L=12 and C=260 -> SHAPE', {'L': 12, 'C': 260})] + L_ROWS),
    'bmnas_mixsum_pair_fwd_lazy': (call_fwd_lazy, [('valid b=0', {})] +
                                   _nulls(['xs', 'w', 'w2', 'last', 'last_out', 'out', 'out2']) +
                                   _nullable(['last_sums']) +
                                   [(f'last.{f}=NULL', {'last_null': f}) for f in _LAZY_FIELDS] +
                                   [('b=-1', {'b': -1}), ('w_stride=0', {'w_stride': 0}), ('w2_stride=0', {'w2_stride': 0}),
                                    ('C=0 (LIMIT)', {'C': 0}), ('C=260 L=16: 5 parts (LIMIT)', {'C': 260, 'L': 16}),
                                    ('b=1 xs[1]=NULL', {'b': 1, 'xs_null': 1}),
                                    ('order: out=NULL and n_in=16 -> ARG', {'out': None, 'n_in': 16}),
                                    ('order: last.rec=NULL and n_in=16 -> ARG', {'last_null': 'rec', 'n_in': 16}),
                                    ('order: n_in=16 and L=12 -> LIMIT', {'n_in': 16, 'L': 12})] + N_IN_ROWS + L_ROWS),
    'bmnas_mixsum_pair_bwd_lazy': (call_bwd_lazy, [('valid b=0', {})] +
                                   _nulls(['xs', 'dxs', 'w', 'w2', 'h', 'gz', 'lazy', 'lnpart', 'lnpart_stride']) +
                                   _nullable(['gh', 'gz2', 'g_full']) + _DW +
                                   [('b=-1', {'b': -1}), ('w_stride=0', {'w_stride': 0}), ('w2_stride=0', {'w2_stride': 0}),
                                    ('n_lazy=0 (LIMIT)', {'n_lazy': 0}), ('n_lazy=-1 (LIMIT)', {'n_lazy': -1}),
                                    ('n_lazy=2 n_in=3', {'n_lazy': 2, 'n_in': 3}), ('n_lazy=3 n_in=4 (LIMIT)', {'n_lazy': 3, 'n_in': 4}),
                                    ('n_lazy=2 n_in=2 (LIMIT)', {'n_lazy': 2}), ('n_lazy=1 n_in=1 (LIMIT)', {'n_in': 1}),
                                    ('n_lazy=2 n_in=15', {'n_lazy': 2, 'n_in': 15}),
                                    ('C=0 (LIMIT)', {'C': 0}), ('C=260 L=16: 5 parts (LIMIT)', {'C': 260, 'L': 16}),
                                    ('b=1 xs[0]=NULL', {'b': 1, 'xs_null': 0}),
                                    ('b=1 lazy[0].pre=NULL', {'b': 1, 'lazy_null': 'pre'}),
                                    ('b=1 lazy[0].ln_w=NULL', {'b': 1, 'lazy_null': 'ln_w'}),
                                    ('b=1 lazy[0].stats=NULL', {'b': 1, 'lazy_null': 'stats'}),
                                    ('b=1 lnpart[0]=NULL', {'b': 1, 'lnpart_null': 0}),
                                    ('b=1 C=256 L=16 lnpart_stride=3 < 4 parts', {'b': 1, 'C': 256, 'L': 16, 'stride': 3}),
                                    ('b=1 lnpart_stride=0', {'b': 1, 'stride': 0}),
                                    ('b=1 n_in=3 dxs[0]=dxs[2], the lazy one', {'b': 1, 'n_in': 3, 'dxs_same': (0, 2)}),
                                    ('b=1 n_in=3 n_lazy=2 dxs[1]=dxs[2], both lazy', {'b': 1, 'n_in': 3, 'n_lazy': 2,
                                                                                     'dxs_same': (1, 2)}),
                                    ('order: dw without dw2 and n_lazy=0 -> ARG', {'dw2': None, 'n_lazy': 0}),
                                    ('order: n_lazy=0 and n_in=16 -> LIMIT', {'n_lazy': 0, 'n_in': 16}),
                                    ('order: b=1 xs[0]=NULL and lnpart_stride=0 -> ARG', {'b': 1, 'xs_null': 0, 'stride': 0})] +
                                   [(f'n_in={v}', {'n_in': v}) for v in (0, 15, 16, 17)] + L_ROWS),
}

# bmnas_lazy_ln_ok / bmnas_lazy_ln_parts at their edges: (C, L)
LAZY_SHAPES = [(0, 4), (1, 4), (1, 8), (1, 16), (1, 12), (1, 0), (16, 2), (256, 4), (257, 4), (1024, 4), (1025, 4),
               (1028, 4), (512, 8), (513, 8), (514, 8), (256, 16), (257, 16), (64, 16), (65, 16), (4096, 4), (-4, 4)]


def _late_refusal(fn, a):
    """a row that passes the entry's b == 0 (n_elem == 0) return may be called only where the entry refuses it before its
    launch; those refusals restated"""
    if fn.startswith('bmnas_mixsum_') and 'lazy' not in fn:
        if a['n_elem'] <= 0 or a['n_elem'] % 4:
            return True
        bad = a['xs_null'] is not None and a['xs_null'] < a['n_in']
        if fn == 'bmnas_mixsum_pair_bwd_x' and a['n_more'] > 0:
            bad = bad or any(a[k] is not None and a[k] < a['n_more'] for k in ('g_more_null', 'w_more_null'))
        return bad
    if a['b'] <= 0:
        return True
    cl4 = a['C'] * a['L'] // 4
    bs = 512 if a['b'] <= 256 and cl4 * (a['n_src'] if 'cat_ln' in fn else 1) >= 512 else 256
    if fn in ('bmnas_cat_ln_fwd', 'bmnas_cat_ln_bwd'):
        return a['src_null'] is not None or cl4 * a['n_src'] > 16 * bs
    if fn.startswith('bmnas_bn_relu_ln_'):
        if a['n_prev'] > 0 and (a['b'] > 128 or cl4 > 256):
            return True
        return ('fwd' in fn and a['C'] > 4 * bs) or cl4 > 8 * bs
    if fn == 'bmnas_mixsum_pair_fwd_lazy':
        return a['xs_null'] is not None and a['xs_null'] < a['n_in']
    if fn == 'bmnas_mixsum_pair_bwd_lazy':
        parts = (cl4 + 255) // 256
        alias = a['dxs_same'] is not None and any(j >= a['n_in'] - a['n_lazy'] for j in a['dxs_same'])
        return (a['xs_null'] is not None or a['lazy_null'] in ('pre', 'ln_w', 'stats') or a['lnpart_null'] is not None or
                a['stride'] < parts or alias)
    return False


def _codes(fn):
    lib, so = _lib()
    call, rows = ENTRIES[fn]
    got = {}
    for cid, over in rows:
        a = _base()
        a.update(over)
        assert _late_refusal(fn, a), (fn, cid)                     # nothing here may reach a launch
        assert cid not in got, (fn, cid)
        got[cid] = call(lib, so, a)
    return got


def _lazy_codes():
    _, so = _lib()
    return {f'C={c} L={l}': [so.bmnas_lazy_ln_ok(c, l), so.bmnas_lazy_ln_parts(c, l)] for c, l in LAZY_SHAPES}


def record():
    out = {fn: _codes(fn) for fn in ENTRIES}
    out['bmnas_lazy_ln_ok / _parts'] = _lazy_codes()
    return out


def _golden():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.mark.parametrize('fn', sorted(ENTRIES))
def test_entry_point_return_codes(fn):
    got, want = _codes(fn), _golden()[fn]
    assert sorted(got) == sorted(want), 'the case list and the recorded table differ: regenerate on purpose only'
    bad = {k: (got[k], want[k]) for k in got if got[k] != want[k]}
    assert not bad, f'{fn}: case -> (returned, recorded): {bad}'


def test_lazy_ln_ok_and_parts():
    got, want = _lazy_codes(), _golden()['bmnas_lazy_ln_ok / _parts']
    assert got == want
    # restated: L in {4, 8, 16}, C >= 1, ceil(C L / 4 / 256) parts, at most 4
    for c, l in LAZY_SHAPES:
        parts = (c * l // 4 + 255) // 256
        ok = c >= 1 and l in (4, 8, 16) and parts <= 4
        assert want[f'C={c} L={l}'] == [int(ok), parts if ok else -3], (c, l)


def test_no_row_reached_a_launch():
    """a code > 0 is a hipError_t: a call that got as far as a launch"""
    g = _golden()
    assert sorted(g) == sorted(list(ENTRIES) + ['bmnas_lazy_ln_ok / _parts'])
    for fn in ENTRIES:
        assert all(code in (0, -1, -2, -3) for code in g[fn].values()), fn
        for cid, over in ENTRIES[fn][1]:
            if over.get('b', 0) > 0 or (over.get('n_elem', 0) > 0 and over['n_elem'] % 4 == 0):
                assert g[fn][cid] < 0, (fn, cid)


def test_the_pinned_order_and_list_lengths():
    g = _golden()
    n_in = [f'n_in={v}' for v in (0, 1, 15, 16, 17)]
    for fn in ('bmnas_mixsum_fwd', 'bmnas_mixsum_bwd', 'bmnas_mixsum_pair_fwd'):          # up to 16 inputs
        assert [g[fn][k] for k in n_in] == [-1, 0, 0, 0, -3], fn
    for fn in ('bmnas_mixsum_pair_bwd', 'bmnas_mixsum_pair_bwd_x', 'bmnas_mixsum_pair_fwd_lazy'):   # up to 15
        assert [g[fn][k] for k in n_in] == [-1, 0, 0, -3, -3], fn
    t = g['bmnas_mixsum_pair_bwd_lazy']                          # n_lazy = 1 < n_in
    assert [t[k] for k in ('n_in=0', 'n_lazy=1 n_in=1 (LIMIT)', 'n_in=15', 'n_in=16', 'n_in=17')] == [-1, -3, 0, -3, -3]
    assert t['n_lazy=2 n_in=2 (LIMIT)'] == -3 and t['n_lazy=2 n_in=3'] == 0 and t['n_lazy=3 n_in=4 (LIMIT)'] == -3
    assert t['b=1 n_in=3 dxs[0]=dxs[2], the lazy one'] == -1 and t['b=1 lnpart_stride=0'] == -1
    for fn in ('bmnas_bn_relu_ln_fwd_pair', 'bmnas_bn_relu_ln_bwd_pair'):
        t = g[fn]
        assert [t[k] for k in ('n_prev=-1', 'n_prev=1', 'n_prev=15', 'n_prev=16 (LIMIT)', 'n_prev=17 (LIMIT)')] == \
            [-1, 0, 0, -3, -3], fn
        assert t['n_prev=2 xs[1]=NULL'] == -1 and t['order: n_prev=16 and xs[0]=NULL -> LIMIT'] == -3, fn
    t = g['bmnas_bn_relu_ln_bwd_pair']
    assert t['n_prev=3 dxs[2]=dxs[0]'] == -1 and t['n_prev=3 dxs[2]=dxs[1]'] == -1
    for fn in ('bmnas_mixsum_pair_bwd', 'bmnas_mixsum_pair_bwd_x', 'bmnas_mixsum_pair_bwd_lazy'):
        t = g[fn]
        assert t['dw without dw2'] == -1 and t['dw2 without dw'] == -1 and t['dw and dw2 NULL (no dots)'] == 0, fn
    Ls = [f'L={v}' for v in (0, 2, 4, 6, 8, 12, 16, 20)]
    for fn in ('bmnas_bn_relu_ln_fwd_pair', 'bmnas_bn_relu_ln_fwd'):                    # the forward tails' rule
        assert [g[fn][k] for k in Ls] == [0, -2, 0, -2, 0, 0, 0, -2], fn
        assert g[fn]['fin shards=5'] == -3 and g[fn]['fin training valid, b L = 0 < 2'] == -1, fn
        assert g[fn]['order: L=6 and fin bn_w=NULL -> SHAPE'] == -2, fn
    for fn in ('bmnas_bn_relu_ln_bwd_pair', 'bmnas_bn_relu_ln_bwd', 'bmnas_node_mix_lnp_bwd'):   # the backward rule
        assert [g[fn][k] for k in Ls] == [-2, -2, 0, -2, 0, -2, 0, -2], fn
    for fn in ('bmnas_mixsum_pair_fwd_lazy', 'bmnas_mixsum_pair_bwd_lazy'):            # bmnas_lazy_ln_ok: LIMIT
        assert [g[fn][k] for k in Ls] == [-3, -3, 0, -3, 0, -3, 0, -3], fn
    for fn in ('bmnas_cat_ln_fwd', 'bmnas_cat_ln_bwd', 'bmnas_ln_affine_bwd'):         # any L >= 1 with C L % 4 == 0
        assert [g[fn][k] for k in Ls] == [-1, 0, 0, 0, 0, 0, 0, 0], fn
    for fn in ('bmnas_cat_ln_fwd', 'bmnas_cat_ln_bwd'):                                 # ln_launch_shape: 16 per thread
        assert g[fn]['b=1 C=8196 L=4: 8196 float4 > 16 x 512 (LIMIT)'] == -3, fn
        assert g[fn]['b=257 C=4100 L=4: 4100 float4 > 16 x 256 (LIMIT)'] == -3, fn
    t = g['bmnas_bn_relu_ln_fwd_pair']                                                  # ... 8 per thread, C <= 4 bs
    assert t['b=1 C=2052 L=4: C > 4 x 512 (LIMIT)'] == -3 and t['b=257 C=1028 L=4: C > 4 x 256 (LIMIT)'] == -3
    assert t['b=1 C=2048 L=16: 8192 float4 > 8 x 512 (LIMIT)'] == -3
    assert g['bmnas_bn_relu_ln_bwd_pair']['b=1 C=2304 L=16: 9216 float4 > 8 x 512 (LIMIT)'] == -3
    t = g['bmnas_mixsum_pair_bwd_x']
    assert t['n_more=3 (LIMIT)'] == -3 and t['n_more=-1 (LIMIT)'] == -3 and t['n_more=0 g_more / w_more NULL'] == 0
    t = g['bmnas_ln_affine_bwd_multi']
    assert [t[f'n_prob={v}'] for v in (0, 1, 8, 9)] == [-1, 0, 0, -3] and t['g[1]=NULL'] == -1


if __name__ == '__main__':
    sys.path.insert(0, os.path.join(ROOT, 'bm-nas_amd'))
    json.dump(record(), sys.stdout, indent=1, sort_keys=True)
    print()
