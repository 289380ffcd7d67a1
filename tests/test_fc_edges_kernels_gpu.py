"""-m gpu: the five entry points behind a mixed-edge sum with fc_relu / fc_mish primitives (include/bmnas_hip.h:
bmnas_fc_edges_gemm_fwd with F = 1 and 2, bmnas_fc_edges_mix_fwd, bmnas_fc_edges_bwd_reduce, bmnas_fc_edges_bwd_du,
bmnas_fc_edges_bwd_gemm) called directly, in the order bmnas.functions.FcEdgeSumFn issues them, against the float64
restatement of tests/fc_sum_ref.py (itself checked on the CPU by tests/test_fc_sum_ref.py).

Cases (fc_sum_ref.CASES: C, L, b, the columns, the state every edge reads):
  1  the smallest accepted sum: P = 1, no skip column, no data gradient requested (n_dx = 0)
  2  C = 16, F = 2: both primitives' 16 rows in one 64-row tile of fc_gemm_fwd_k, waves 2-3 exit; L = 4 (16 sample
     slots per block of the elementwise kernels)
  3  F * C = 96: a row tile holds rows 0-47 of f = 0 and 0-15 of f = 1; col = (0, 3); 72 columns (a tail of 8); wave 3
     of the data-gradient blocks exits
  4  N = 528: two split-K chunks of the weight-gradient blocks, the second 16 columns wide; the second FC_SPC block
     holds one sample; k-tail tiles of dW (k < 80)
  5  a NodeCell's inner sum: one destination with qmask 0b11, the skip weight summed over both edges
  6  shared and own sources, one source that needs no gradient: masks 0b0101, 0b0010
  7  BMNAS_FC_MAX_EDGES = 15 edges, P = 8, two skip columns: the largest by-value argument blocks
  8  the production channel count, three row tiles

x, W and bias lie on dyadic grids (fc_sum_ref.make_case), so U is compared with torch.equal and no ReLU decision is
within round-off of zero.  out, every dU[j], every requested dx and dw sit in NaN-guarded buffers; the rows of the
sources whose gradient was not requested must stay NaN."""
import ctypes as C

import pytest
import torch

import fc_sum_ref as R
from fc_edges_util import guarded, guards_intact
from gpu_util import assert_close_of_scale, assert_close_scaled, dev

pytestmark = pytest.mark.gpu


def run_gpu(case, xs, edges, w, g, drops, training):
    """Zero-filled stat, gemm_fwd, mix_fwd, zero-filled pool, bwd_reduce, bwd_du, bwd_gemm."""
    from bmnas import lib
    Cc, L, b, prims, src, need_dx = case
    fcols, kinds, skip_cols = R.columns(prims)
    n, P, F = len(src), len(prims), len(fcols)
    d = dev()
    nan = lambda *s: torch.full(s, float('nan'), device=d, dtype=torch.float32)
    xg = [x.to(d) for x in xs]
    wg, gg = w.to(d).contiguous(), g.to(d).contiguous()
    prm = [[{k: q[k].to(d).contiguous() for k in ('W', 'bias', 'bn_w', 'bn_b', 'rm', 'rv')} for q in fc] for fc in edges]
    nbt = [[torch.tensor(7, device=d, dtype=torch.int64) for _ in range(F)] for _ in range(n)]
    U = nan(n, b, F * Cc, L)
    chan = nan(n, F, 4 * Cc)
    stat = torch.zeros(n, F, 2 * Cc, device=d) if training else None
    out_buf, (out,), out_keep = guarded(1, (b, Cc, L))
    recs = [dict(x=xg[src[j]], U=U[j],
                 fc=[dict(W=prm[j][f]['W'], bias=prm[j][f]['bias'], bn_w=prm[j][f]['bn_w'], bn_b=prm[j][f]['bn_b'],
                          running_mean=prm[j][f]['rm'], running_var=prm[j][f]['rv'], num_batches_tracked=nbt[j][f],
                          stat=None if stat is None else stat[j, f], chan=chan[j, f], drop=drops[j][f], col=fcols[f],
                          mish=kinds[f]) for f in range(F)]) for j in range(n)]
    arr = lib.make_fc_edges(recs)
    lib.fc_edges_gemm_fwd(arr, F, training, b, Cc, L)
    lib.fc_edges_mix_fwd(arr, F, wg, P, skip_cols, training, out, b, Cc, L)
    # backward: bn_grad | dW | dbias per (edge, primitive) zero-filled, dw zero-filled between NaN guards
    per = 2 * Cc + Cc * Cc + Cc
    pool = torch.zeros(n, F, per, device=d)
    dw_buf, (dw,), dw_keep = guarded(1, (n, P))
    dw.zero_()
    du_buf, dUs, du_keep = guarded(n, (b, F * Cc, L))
    for j in range(n):
        recs[j]['dU'] = dUs[j]
        for f in range(F):
            q = recs[j]['fc'][f]
            q['bn_grad'], q['dW'], q['dbias'] = pool[j, f, :2 * Cc], pool[j, f, 2 * Cc:2 * Cc + Cc * Cc], \
                pool[j, f, 2 * Cc + Cc * Cc:]
    arr = lib.make_fc_edges(recs)
    lib.fc_edges_bwd_reduce(arr, F, wg, P, skip_cols, gg, dw, b, Cc, L)
    lib.fc_edges_bwd_du(arr, F, wg, P, gg, training, b, Cc, L)
    dx_buf, dx_rows, dx_keep = guarded(len(xs), (b, Cc, L))
    targets, masks, which = [], [], []
    for s in range(len(xs)):
        if need_dx[s]:
            targets.append(dx_rows[s])
            masks.append(sum(1 << j for j in range(n) if src[j] == s))
            which.append(s)
    lib.fc_edges_bwd_gemm(arr, F, wg, P, skip_cols, gg, targets, masks, b, Cc, L)
    torch.cuda.synchronize()
    assert guards_intact(out_buf, out_keep) and guards_intact(du_buf, du_keep) and guards_intact(dw_buf, dw_keep)
    # (the rows of the sources that need no gradient are guards too)
    for s in range(len(xs)):
        if not need_dx[s]:
            dx_keep[2 + 3 * s] = True
    assert guards_intact(dx_buf, dx_keep)
    return dict(U=U, chan=chan, out=out, dw=dw, dUs=dUs, pool=pool, prm=prm, nbt=nbt, masks=masks,
                dx={s: dx_rows[s] for s in which})


def sites(case, training):
    """Live dropout in the training cases with more than one edge: one site per (edge, primitive), edge by edge,
    offsets as _DropState hands them out.  -> (descriptors[j][f], exported masks[j][f] on the CPU)."""
    from bmnas import lib
    Cc, L, b, prims, src, _ = case
    n, F = len(src), len(R.columns(prims)[0])
    numel = b * Cc * L
    live = training and n > 1
    drops = [[lib.make_dropout(R.P_DROP, 1234, (j * F + f) * ((numel + 3) // 4)) if live else lib.NO_DROP
              for f in range(F)] for j in range(n)]
    masks = [[lib.dropout_mask(dr, numel, dev()).cpu() for dr in row] for row in drops]
    if live:
        flat = [m for row in masks for m in row]
        assert 0.1 < float((torch.stack(flat) == 0).float().mean()) < 0.4
        assert not torch.equal(flat[0], flat[1])
    return drops, masks


@pytest.mark.parametrize('training', [True, False], ids=['train', 'eval'])
@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_entry_points_against_float64(case, training):
    Cc, L, b, prims, src, need_dx = case
    fcols, kinds, skip_cols = R.columns(prims)
    n, P, F = len(src), len(prims), len(fcols)
    xs, edges, w, g = R.make_case(case, 2100 + 7 * Cc + L + b + n)
    drops, masks = sites(case, training)
    want = R.reference(case, xs, edges, w, g, masks, training)
    got = run_gpu(case, xs, edges, w, g, drops, training)
    for j in range(n):
        for f in range(F):
            r, tag = want['fc'][j][f], f'[{j}][{f}]'
            assert float(r['U'].abs().min()) >= 1.0 / 512 - 1e-12
            assert torch.equal(got['U'][j][:, f * Cc:(f + 1) * Cc, :].cpu().double(), r['U']), 'U' + tag   # exact
            for i, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
                assert_close_of_scale(f'chan{tag}.{name}', got['chan'][j, f, i * Cc:(i + 1) * Cc], r['chan'][i], rel=1e-4)
            assert_close_of_scale('running_mean' + tag, got['prm'][j][f]['rm'], r['rm'], rel=1e-4)
            assert_close_of_scale('running_var' + tag, got['prm'][j][f]['rv'], r['rv'], rel=1e-4)
            assert int(got['nbt'][j][f]) == 7 + int(training)
            pool = got['pool'][j, f]
            assert_close_scaled('bn_grad' + tag, pool[:2 * Cc], r['bn_grad'], rel=2e-4)
            assert_close_scaled('dU' + tag, got['dUs'][j][:, f * Cc:(f + 1) * Cc, :], r['dU'], rel=2e-4)
            assert_close_scaled('dW' + tag, pool[2 * Cc:2 * Cc + Cc * Cc].view(Cc, Cc), r['dW'], rel=2e-4)
            assert_close_scaled('dbias' + tag, pool[2 * Cc + Cc * Cc:], r['dbias'], rel=2e-4)
    assert_close_of_scale('out', got['out'], want['out'], rel=1e-4)
    assert_close_scaled('dw', got['dw'], want['dw'], rel=2e-4)
    for c, name in enumerate(prims):
        if name == 'none':
            assert float(got['dw'][:, c].abs().max()) == 0.0
    assert sorted(got['dx']) == [s for s in range(len(xs)) if need_dx[s]]
    for s, dx in got['dx'].items():
        assert_close_scaled(f'dx[{s}]', dx, want['dx'][s], rel=2e-4)
    if case is R.CASES[4]:
        assert got['masks'] == [0b11]
    if case is R.CASES[5]:
        assert got['masks'] == [0b0101, 0b0010]


def test_shifted_batch_variance():
    """Case 2's shape, training, no dropout, 128 (fc_sum_ref.SHIFT_BIAS) added to every fc_relu bias: the channel mean
    of act(u) is ~128, its standard deviation below 1.  fc_gemm_fwd_k sums act(u) - act(bias) and its square, so that
    E[d^2] - E[d]^2 does not cancel.  Emulated in fp32 (tests/test_fc_sum_ref.py, test_shifted_variance_constant),
    measured against the float64 reference in units of the rel = 1e-4 tolerance on chan.mean, chan.rstd and
    running_var: the shifted sums err by 0.0016 x the tolerance, the unshifted E[a^2] - E[a]^2 by 227 x (sequential and
    pairwise summation, the better of the two).  128 + the 1/512 grid needs 17 bits: U stays exact."""
    case = R.CASES[1]
    Cc, L, b, prims, src, _ = case
    xs, edges, w, g = R.make_case(case, R.SHIFT_SEED, R.SHIFT_BIAS)
    drops, masks = sites(case, False)                       # no dropout
    want = R.reference(case, xs, edges, w, g, masks, True)
    got = run_gpu(case, xs, edges, w, g, drops, True)
    for j in range(len(src)):
        for f in range(2):
            r, tag = want['fc'][j][f], f'[{j}][{f}]'
            assert torch.equal(got['U'][j][:, f * Cc:(f + 1) * Cc, :].cpu().double(), r['U']), 'U' + tag
            assert_close_of_scale(f'chan{tag}.mean', got['chan'][j, f, :Cc], r['chan'][0], rel=1e-4)
            assert_close_of_scale(f'chan{tag}.rstd', got['chan'][j, f, Cc:2 * Cc], r['chan'][1], rel=1e-4)
            assert_close_of_scale('running_var' + tag, got['prm'][j][f]['rv'], r['rv'], rel=1e-4)
    r = want['fc'][0][0]
    assert float((r['chan'][0] * r['chan'][1]).min()) > 100.0          # mean / std of the fc_relu channels


def test_argument_errors():
    """BMNAS_E_ARG (-1) first, then BMNAS_E_SHAPE (-2), then BMNAS_E_LIMIT (-3); nothing is launched on a bad call."""
    from bmnas import lib
    L_ = lib.load()
    Cc, L, b, n, F, P = 16, 4, 3, 2, 2, 4
    d = dev()
    t = lambda *s: torch.zeros(*s, device=d)
    x, U, dU, out, g, dx = t(b, Cc, L), t(16, b, F * Cc, L), t(16, b, F * Cc, L), t(b, Cc, L), t(b, Cc, L), t(b, Cc, L)
    chan, stat, pool = t(16, F, 4 * Cc), t(16, F, 2 * Cc), t(16, F, 2 * Cc + Cc * Cc + Cc)
    W, vec = t(Cc, Cc), t(Cc)
    rm, rv = t(Cc), t(Cc) + 1
    w, dw = t(16, 9) + 0.25, t(16, 9)
    nbt = torch.zeros((), device=d, dtype=torch.int64)
    cols, skip = (1, 2), 0b1000

    def recs(n_=n):
        return [dict(x=x, U=U[j], dU=dU[j],
                     fc=[dict(W=W, bias=vec, bn_w=vec, bn_b=vec, running_mean=rm, running_var=rv,
                              num_batches_tracked=nbt, stat=stat[j, f], chan=chan[j, f], bn_grad=pool[j, f, :2 * Cc],
                              dW=pool[j, f, 2 * Cc:2 * Cc + Cc * Cc], dbias=pool[j, f, 2 * Cc + Cc * Cc:], col=cols[f],
                              mish=f) for f in range(F)]) for j in range(n_)]
    s = lib._stream()
    one = lambda m: (C.c_uint32 * 1)(m)
    dxs, pw, pg, pdw, pout = lib._ptrs([dx]), w.data_ptr(), g.data_ptr(), dw.data_ptr(), out.data_ptr()

    def all_five(arr, n_=n, F_=F, P_=P, sk=skip, b_=b, C_=Cc, L_len=L, w_=pw, g_=pg, out_=pout, dw_=pdw, dxs_=dxs,
                 mk=None, n_dx=1):
        mk = one(0b11) if mk is None else mk
        return (L_.bmnas_fc_edges_gemm_fwd(arr, n_, F_, 1, b_, C_, L_len, s),
                L_.bmnas_fc_edges_mix_fwd(arr, n_, F_, w_, P_, sk, 1, out_, b_, C_, L_len, s),
                L_.bmnas_fc_edges_bwd_reduce(arr, n_, F_, w_, P_, sk, g_, dw_, b_, C_, L_len, s),
                L_.bmnas_fc_edges_bwd_du(arr, n_, F_, w_, P_, g_, 1, b_, C_, L_len, s),
                L_.bmnas_fc_edges_bwd_gemm(arr, n_, F_, w_, P_, sk, g_, dxs_, mk, n_dx, b_, C_, L_len, s))
    good = lib.make_fc_edges(recs())
    assert all_five(good) == (0,) * 5
    assert all_five(None) == (-1,) * 5                                   # no edges
    assert all_five(good, n_=0) == (-1,) * 5
    assert all_five(good, b_=0) == (-1,) * 5
    assert all_five(lib.make_fc_edges(recs(16)), n_=16, mk=one(1)) == (-3,) * 5            # n = 16: a limit
    assert all_five(good, P_=9)[1:] == (-3,) * 4                         # P = 9 (the forward GEMM takes no P)
    assert all_five(good, C_=24) == (-2,) * 5                            # C = 24
    assert all_five(good, L_len=12) == (-2,) * 5                         # L = 12
    assert all_five(good, F_=3) == (-2,) * 5
    assert lib.fc_edges_ok(n, F, P, 65535, Cc, L) and not lib.fc_edges_ok(n, F, P, 65536, Cc, L)
    assert all_five(good, b_=65536) == (-2,) * 5                         # (refused before anything is touched)
    # null pointers, entry point by entry point
    assert all_five(good, w_=None) == (0, -1, -1, -1, -1)
    assert all_five(good, out_=None) == (0, -1, 0, 0, 0)
    assert all_five(good, g_=None) == (0, 0, -1, -1, -1)
    assert all_five(good, dw_=None) == (0, 0, -1, 0, 0)
    # skip_cols with a bit at or above P
    assert all_five(good, sk=1 << P) == (0, -1, -1, 0, -1)
    assert all_five(good, P_=3) == (0, -1, -1, 0, -1)                    # (the skip column itself is column 3)
    # the data-gradient destinations
    null_mask = C.POINTER(C.c_uint32)()
    assert all_five(good, dxs_=None)[4] == -1 and all_five(good, mk=null_mask)[4] == -1
    assert all_five(good, dxs_=None, mk=null_mask, n_dx=0)[4] == 0       # n_dx = 0: no destination
    assert all_five(good, dxs_=(C.c_void_p * 1)(None))[4] == -1
    assert all_five(good, mk=one(0))[4] == -1                            # a zero mask
    assert all_five(good, mk=one(0b100))[4] == -1                        # a mask bit at or above n
    assert all_five(good, dxs_=lib._ptrs([dx] * 16), mk=(C.c_uint32 * 16)(*[1] * 16), n_dx=16)[4] == -1
    assert all_five(good, n_dx=-1)[4] == -1
    # missing fields, (gemm_fwd, mix_fwd, bwd_reduce, bwd_du, bwd_gemm)
    for field, hits in (('W', (-1,) * 5), ('bias', (-1,) * 5), ('bn_w', (-1,) * 5), ('bn_b', (-1,) * 5),
                        ('chan', (-1,) * 5), ('stat', (-1, -1, 0, 0, 0)), ('running_mean', (0, -1, 0, 0, 0)),
                        ('running_var', (0, -1, 0, 0, 0)), ('bn_grad', (0, 0, -1, -1, 0)), ('dbias', (0, 0, 0, -1, 0)),
                        ('dW', (0, 0, 0, 0, -1)), ('edge_dU', (0, 0, 0, -1, -1)), ('edge_x', (-1,) * 5),
                        ('edge_U', (-1,) * 5)):
        r = recs()
        if field.startswith('edge_'):
            r[1][field[5:]] = None
        else:
            r[1]['fc'][1][field] = None
        assert all_five(lib.make_fc_edges(r)) == hits, field
    # col >= P (the forward GEMM knows no P: its bound is 8) and col < 0, on both edges alike
    for value, hits in ((P, (0, -1, -1, -1, -1)), (8, (-1,) * 5), (-1, (-1,) * 5)):
        r = recs()
        for j in range(n):
            r[j]['fc'][1]['col'] = value
        assert all_five(lib.make_fc_edges(r)) == hits, value
    # col or mish differing between the edges
    for field in ('col', 'mish'):
        r = recs()
        r[1]['fc'][1][field] = 0
        assert all_five(lib.make_fc_edges(r)) == (-1,) * 5, field
    # dropout configurations that differ in more than the offset
    for other, ok in ((lib.make_dropout(0.5, 1, 0), False), (lib.make_dropout(0.25, 2, 0), False),
                      (lib.make_dropout(0.25, 1, 64), True)):
        r = recs()
        for j in range(n):
            for f in range(F):
                r[j]['fc'][f]['drop'] = lib.make_dropout(0.25, 1, 0)
        r[1]['fc'][0]['drop'] = other
        assert all_five(lib.make_fc_edges(r)) == ((0,) * 5 if ok else (-1,) * 5), other
    torch.cuda.synchronize()
