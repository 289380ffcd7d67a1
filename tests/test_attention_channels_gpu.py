"""-m gpu: the scaled-dot-attention kernels (csrc/sdpa.hip, csrc/sdpa_body.hpp) and the two merged conv + attention
launches (csrc/conv1x1.hip) over the whole channel range the ABI accepts, through the C ABI, against the plain
float64 statement of the operation in tests/attention_ref.py (itself checked by tests/test_attention_ref.py).

Which code a channel count C runs (C % 16 == 0, 16 <= C <= 512; a wave owns the 16-channel chunks wave, wave + 4, ...
so C/16 not a multiple of 4 gives the waves unequal numbers of chunks = "ragged"):

    C          chunks  KCH = ceil(C/64)  sdpa_ln_{fwd,bwd}_k<..>  merged launches (conv M = 3C beside the attention)
    16 ..  64   1.. 4  1                 <1>                      C <= 256, forward (conv K == C):
    80 .. 128   5.. 8  2                 <2>                        fold_cols == 0 and ceil(ng/2) * ceil(3C/96) >= 96
   144 .. 192   9..12  3                 <3>                          -> conv_pipe_fwd_sdpa_k<32|48, KCH, 2|4>   fwd_sdpa_pipe
   208 .. 256  13..16  4                 <4>                        else -> conv_fwd_sdpa_k<1|2, 1|2, KCH>        fwd_sdpa_ksplit
   272 .. 320  17..20  5                 <6>  (rounded up)        C <= 256, backward (dU (b, 3C, L), J = n_src * C):
   336 .. 384  21..24  6                 <6>                        fold_cols == 0 and ceil(ng/2) * ceil(J/64) >= 48
   400 .. 448  25..28  7                 <8>  (rounded up)            -> conv_bwd_all_pipe_k<48, KCH, 2>          bwd_all_pipe
   464 .. 512  29..32  8                 <8>                        else C % 64 == 0 -> conv_bwd_all_k<1|2, 1|2, KCH>  bwd_all_ksplit
                                                                    else three launches (data, attention, weight)
                                                                  C > 256, conv K != C (forward) or M != 3C (backward):
                                                                    separate launches, no fwd_sdpa_* / bwd_all_* count

(ng = ceil(b * L / 16) 16-column groups.)  A rounded-up instantiation runs more chunk slots than the wave owns: the
`ch < nch` guards, the clamped prefetch addresses and the [C][17] LDS transpose buffer of the backward are what the
C = 272 / 400 cases exercise; C = 80 / 208 are the ragged ones.

Every output buffer starts as NaN with one more sample's worth of a sentinel behind it: nothing may be left
unwritten and nothing may be written for the padded samples of the last tile group.  Each case prints its worst
err / (|want| + max|want|) per tensor (pytest -s) and, when BMNAS_TEST_ERR_DIR names a directory, appends it to
attention_channels_err.jsonl there."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import attention_ref as ar
from gpu_util import assert_close_scaled, dev

pytestmark = pytest.mark.gpu

# the family expectations describe the DEFAULT dispatch (as tests/test_dispatch_gpu.py): with a kernel family
# forced through the environment only the numbers are checked
_FORCED = [k for k in ('BMNAS_CONV_PIPE', 'BMNAS_FUSE_ATTN_GEMM', 'BMNAS_FUSE_BWD_PAIR') if os.environ.get(k) is not None]

SENTINEL = 12345.0
FWD_REL, BWD_REL = 1e-4, 2e-4            # test_sdpa_ln_fwd_bwd
U_REL, SUM_REL, SQ_REL = 2e-5, 5e-5, 2e-4  # test_conv1x1_fwd_large_single_source
CONV_BWD_REL = 5e-5                      # test_conv1x1_bwd_all_pair


def _guarded(shape, init=None):
    """A device buffer of `shape`, NaN (or `init`), with one more shape[0]-slab of SENTINEL behind it -> (buffer,
    tail)."""
    n = int(np.prod(shape))
    full = torch.full((n + n // shape[0],), SENTINEL, device=dev(), dtype=torch.float32)
    real = full[:n].view(*shape)
    if init is None:
        real.fill_(float('nan'))
    else:
        real.copy_(init)
    return real, full[n:]


def _tails_untouched(**tails):
    torch.cuda.synchronize()
    for name, t in tails.items():
        if t is not None:
            assert torch.equal(t, torch.full_like(t, SENTINEL)), f'{name}: written behind the last sample'


class _Checks:
    """Collects (tensor, expected, bound); finish() records the measured errors, then asserts every bound."""

    def __init__(self, case):
        self.case, self.items = case, []

    def close(self, name, got, want, rel, key=None):
        g = got.detach().cpu().double().numpy()
        w = want.detach().cpu().double().numpy()
        self.items.append((name, key or name, g, w, rel))

    def finish(self):
        errs = {}
        for _, key, g, w, _ in self.items:
            scale = np.abs(w) + np.abs(w).max()
            r = np.abs(g - w) / np.where(scale > 0, scale, 1.0) if g.shape == w.shape else np.array([np.inf])
            r = float(np.max(np.where(np.isfinite(r), r, np.inf)))
            errs[key] = max(errs.get(key, 0.0), r)
        print(f'[{self.case}] worst err / (|want| + max|want|): ' + ', '.join(f'{k} {v:.2e}' for k, v in errs.items()))
        out_dir = os.environ.get('BMNAS_TEST_ERR_DIR')
        if out_dir:
            try:
                os.makedirs(out_dir, exist_ok=True)
                with open(os.path.join(out_dir, 'attention_channels_err.jsonl'), 'a') as f:
                    f.write(json.dumps({'case': self.case, 'err': errs}) + '\n')
            except OSError:
                pass
        for name, _, g, w, rel in self.items:
            assert_close_scaled(f'{self.case} {name}', g, w, rel=rel)


def _drop(on):
    from bmnas import lib
    return lib.make_dropout(ar.DROP_P, ar.DROP_SEED, ar.DROP_OFFSET) if on else lib.NO_DROP


@functools.lru_cache(maxsize=None)
def _attn_case(C, b, L, same, drop_on, have_gs):
    """(fp32 inputs, exported dropout multipliers, float64 reference) of one attention case; shared, never written."""
    from bmnas import lib
    t = ar.make_inputs(C, b, L, same)
    mask = None
    if drop_on:
        mask = lib.dropout_mask(_drop(True), b * C * L, dev()).cpu()
        kept = float((mask > 0).float().mean())
        assert 0.6 < kept < 0.9 and set(np.unique(mask.numpy())) <= {np.float32(0.0), np.float32(1.0 / (1.0 - ar.DROP_P))}
    ref = ar.attention_ref(t['x'], t['y'], t['ln_w'], t['ln_b'], t['g'], mask, ar.GSCALE if have_gs else None, same)
    return t, ref


def _gscale(have):
    return torch.tensor([ar.GSCALE], device=dev(), dtype=torch.float32) if have else None


def _attn_bwd_buffers(t, ref, same, acc, b, C, L):
    """dx / dy buffers (NaN or the previous value to accumulate onto) and what they must hold afterwards."""
    dx, dx_tail = _guarded((b, C, L), t['prev_dx'] if acc & 1 else None)
    want_dx = ref['dx'] + (t['prev_dx'].double() if acc & 1 else 0.0)
    if same:
        return dx, dx_tail, want_dx, None, None, None
    dy, dy_tail = _guarded((b, C, L), t['prev_dy'] if acc & 2 else None)
    want_dy = ref['dy'] + (t['prev_dy'].double() if acc & 2 else 0.0)
    return dx, dx_tail, want_dx, dy, dy_tail, want_dy


# ------------------------------------------------------------------ A. stand-alone attention
@pytest.mark.parametrize('C,b,L,mode,have_gs,drop_on', ar.TABLE_A)
def test_sdpa_ln_channel_range(C, b, L, mode, have_gs, drop_on):
    """bmnas_sdpa_ln_fwd / bmnas_sdpa_ln_bwd at every KCH instantiation, full, ragged and rounded up, with a full and
    a partly empty tile group.  The backward is fed the reference's xhat / stats, so it is judged on its own."""
    from bmnas import lib
    same = mode.startswith('same')
    acc = {'same': 0, 'same+': 1}[mode] if same else int(mode[3:])
    t, ref = _attn_case(C, b, L, same, drop_on, have_gs)
    ck = _Checks(f'A C={C} b={b} L={L} {mode} gs={int(have_gs)} drop={int(drop_on)}')
    d = {k: v.to(dev()) for k, v in t.items()}
    x = d['x']
    y = x if same else d['y']
    out, out_tail = _guarded((b, C, L))
    xhat, xhat_tail = _guarded((b, C, L))
    stats, stats_tail = _guarded((b, 2))
    lib.sdpa_ln_fwd(x, y, d['ln_w'], d['ln_b'], out, xhat, stats, b, C, L, _drop(drop_on))
    for name, buf in (('out', out), ('xhat', xhat), ('stats', stats)):
        ck.close(name, buf, ref[name], FWD_REL)
    dx, dx_tail, want_dx, dy, dy_tail, want_dy = _attn_bwd_buffers(t, ref, same, acc, b, C, L)
    lib.sdpa_ln_bwd(d['g'], _gscale(have_gs), x, y, d['ln_w'], ref['xhat'].float().to(dev()),
                    ref['stats'].float().to(dev()), dx, dy, acc, b, C, L, _drop(drop_on))
    ck.close('dx', dx, want_dx, BWD_REL)
    if not same:
        ck.close('dy', dy, want_dy, BWD_REL)
    _tails_untouched(out=out_tail, xhat=xhat_tail, stats=stats_tail, dx=dx_tail, dy=dy_tail)
    ck.finish()


# ------------------------------------------------------------------ B / C. the merged launches
# (id, C, b, L, n_src, raw, dup, forward family, backward family).  raw: W is the unfolded (3C, 2C) weight of
# NodeMixedOp(z, z) and fold_cols = C; else n_src = 1 reads a pre-folded (3C, C) weight, n_src = 2 (x != y) the plain
# (3C, 2C) one.  dup: dup_cols = C (the weight gradient lands in both halves of a (3C, 2C) dW).  Families: by hand
# from the rules in the module docstring — b = 23 at C = 256 / L = 16 is the smallest batch with
# ceil(23/2) * ceil(768/96) = 96 forward and 12 * 4 = 48 backward tiles (and its last 32-column tile is half empty),
# b = 95 at C = 64 the same for 48 * 2 and 48 * 1; None = separate launches.
MERGED = [
    ('ksplit_raw_C64', 64, 6, 8, 1, True, True, 'fwd_sdpa_ksplit', 'bwd_all_ksplit'),
    ('ksplit_raw_C80', 80, 6, 8, 1, True, True, 'fwd_sdpa_ksplit', None),
    ('ksplit_raw_C208', 208, 6, 8, 1, True, True, 'fwd_sdpa_ksplit', None),
    ('ksplit_raw_C256', 256, 6, 8, 1, True, True, 'fwd_sdpa_ksplit', 'bwd_all_ksplit'),
    ('ksplit_prefolded_C256', 256, 5, 4, 1, False, False, 'fwd_sdpa_ksplit', 'bwd_all_ksplit'),
    ('pipe_C256', 256, 23, 16, 1, False, False, 'fwd_sdpa_pipe', 'bwd_all_pipe'),
    ('pipe_C64', 64, 95, 16, 1, False, True, 'fwd_sdpa_pipe', 'bwd_all_pipe'),
    ('fallback_C320', 320, 6, 8, 1, True, True, None, None),
    ('two_sources_C128', 128, 6, 8, 2, False, False, None, 'bwd_all_ksplit'),
]
# backward only: a three-launch fallback with a pre-folded weight
MERGED_BWD = MERGED + [('fallback_prefolded_C80', 80, 6, 8, 1, False, False, None, None)]
_IDS = [c[0] for c in MERGED_BWD]


@functools.lru_cache(maxsize=None)
def _conv_case(cid):
    """fp32 conv-side tensors of a merged case (shared, never written)."""
    _, C, b, L, n_src, raw, dup, _, _ = MERGED_BWD[_IDS.index(cid)]
    g = ar.gen(9000 + _IDS.index(cid))
    M, K = 3 * C, n_src * C
    ldw = 2 * C if raw else K
    ldg = K + (C if dup else 0)
    return {'W': ar.rand(g, M, ldw) * 0.1, 'bias': ar.rand(g, M), 'dV': ar.rand(g, b, M, L),
            'U': ar.rand(g, b, M, L) * 1.5 + 0.3, 'bn_w': ar.rand(g, M) * 0.3 + 1.0,
            'dW0': ar.rand(g, M, ldg), 'db0': ar.rand(g, M), 'prev': [ar.rand(g, b, C, L) for _ in range(n_src)]}


def _family_delta(fam, names, want):
    if _FORCED:
        return
    for n in names:
        assert fam[n] == (1 if n == want else 0), (want, fam)


@pytest.mark.parametrize('stat_shards', [2, 0])
@pytest.mark.parametrize('cid', [c[0] for c in MERGED])
def test_conv1x1_fwd_sdpa_routes(cid, stat_shards):
    """bmnas_conv1x1_fwd_sdpa called directly: U, both forms of the BatchNorm statistics and the attention outputs
    (dropout on), on the pipelined, the split-K and the separate-launch route."""
    from bmnas import lib
    _, C, b, L, n_src, raw, _, family, _ = MERGED[_IDS.index(cid)]
    same = n_src == 1
    M = 3 * C
    t, ref = _attn_case(C, b, L, same, True, True)
    cv = _conv_case(cid)
    ck = _Checks(f'B {cid} shards={stat_shards}')
    d = {k: v.to(dev()) for k, v in t.items()}
    x = d['x']
    y = x if same else d['y']
    srcs = [x] if same else [x, y]
    fold = C if raw else 0
    W, bias = cv['W'].to(dev()), cv['bias'].to(dev())
    U, U_tail = _guarded((b, M, L))
    out, out_tail = _guarded((b, C, L))
    xhat, xhat_tail = _guarded((b, C, L))
    stats, stats_tail = _guarded((b, 2))
    n_part = lib.conv1x1_num_partials(b, L)
    if stat_shards:
        part = torch.zeros(stat_shards, M, 2, device=dev())
    else:
        part = torch.full((M * n_part * 2,), float('nan'), device=dev())
    lib.conv_family_calls(reset=True)
    lib.conv1x1_fwd_sdpa(srcs, C, W, W.shape[1], bias, U, part, b, L, M, fold, x, y, d['ln_w'], d['ln_b'], out, xhat,
                         stats, C, _drop(True), stat_shards)
    _family_delta(lib.conv_family_calls(), ('fwd_sdpa_pipe', 'fwd_sdpa_ksplit'), family)
    cref = ar.conv_fwd_ref([t['x']] if same else [t['x'], t['y']], cv['W'], cv['bias'], fold)
    ck.close('U', U, cref['U'], U_REL)
    if stat_shards:
        got = part.sum(0)
        ck.close('bn_sum', got[:, 0], cref['d_sum'], SUM_REL)
        ck.close('bn_sq', got[:, 1], cref['d_sq'], SQ_REL)
    else:
        cols = cref['U'].permute(1, 0, 2).reshape(M, b * L)                 # (M, n) in (sample, l) order
        got = part.view(M, n_part, 2)
        for gi in sorted({0, n_part // 2, n_part - 1}):
            seg = cols[:, 16 * gi:16 * gi + 16]
            ck.close(f'sum[{gi}]', got[:, gi, 0], seg.sum(1), SUM_REL, key='bn_sum')
            ck.close(f'm2[{gi}]', got[:, gi, 1], ((seg - seg.mean(1, keepdim=True)) ** 2).sum(1), SQ_REL, key='bn_m2')
    for name, buf in (('out', out), ('xhat', xhat), ('stats', stats)):
        ck.close(name, buf, ref[name], FWD_REL)
    _tails_untouched(U=U_tail, out=out_tail, xhat=xhat_tail, stats=stats_tail)
    ck.finish()


@pytest.mark.parametrize('variant', ['bn', 'acc', 'no_dW'])
@pytest.mark.parametrize('cid', _IDS)
def test_conv1x1_bwd_all_sdpa_routes(cid, variant):
    """bmnas_conv1x1_bwd_all_sdpa called directly (gscale given, dropout on, dy = NULL where x is y) on its three
    routes.  'bn': the BatchNorm input gradient rides in the launch (dV must stay as it is) or, on the fallback, is
    applied in place first (dV must then hold dU).  'acc': no BatchNorm, accumulate bits set on dsrcs[0] and on dx.
    'no_dW': the architecture step, no weight-gradient tiles — dbias is still passed and must stay untouched."""
    from bmnas import lib
    _, C, b, L, n_src, raw, dup, _, family = MERGED_BWD[_IDS.index(cid)]
    same = n_src == 1
    M, K = 3 * C, n_src * C
    t, ref = _attn_case(C, b, L, same, True, True)
    cv = _conv_case(cid)
    ck = _Checks(f'C {cid} {variant}')
    d = {k: v.to(dev()) for k, v in t.items()}
    x = d['x']
    y = x if same else d['y']
    cpu_srcs = [t['x']] if same else [t['x'], t['y']]
    fold = C if raw else 0
    with_bn = variant in ('bn', 'no_dW')
    acc_src = 1 if variant == 'acc' else 0
    acc_attn = {'bn': 0, 'acc': 1 if same else 3, 'no_dW': 1}[variant]
    if with_bn:
        dU_ref, chan, bn_grad = ar.bn_input_grad(cv['dV'], cv['U'], cv['bn_w'])
        bn = (cv['U'].to(dev()), chan.float().to(dev()), bn_grad.float().to(dev()), True)
    else:
        dU_ref, bn = cv['dV'].double(), None
    cref = ar.conv_bwd_ref(dU_ref, cv['W'], fold, cpu_srcs)
    dV_dev = cv['dV'].clone().to(dev())                                    # (the fallback rewrites it in place)
    dsrcs, tails = [], {}
    for q in range(n_src):
        buf, tails[f'dsrc{q}'] = _guarded((b, C, L), cv['prev'][q] if acc_src & (1 << q) else None)
        dsrcs.append(buf)
    dW, db = cv['dW0'].clone().to(dev()), cv['db0'].clone().to(dev())
    dx, tails['dx'], want_dx, dy, tails['dy'], want_dy = _attn_bwd_buffers(t, ref, same, acc_attn, b, C, L)
    lib.conv_family_calls(reset=True)
    lib.conv1x1_bwd_all_sdpa(dV_dev, cv['W'].to(dev()), cv['W'].shape[1], dsrcs, C, acc_src, b, L, M, fold,
                             [x] if same else [x, y], None if variant == 'no_dW' else dW, dW.shape[1], db,
                             C if dup else 0, d['g'], _gscale(True), x, y, d['ln_w'], ref['xhat'].float().to(dev()),
                             ref['stats'].float().to(dev()), dx, dy, acc_attn, C, _drop(True), bn)
    _family_delta(lib.conv_family_calls(), ('bwd_all_pipe', 'bwd_all_ksplit'), family)
    for q in range(n_src):
        want = cref['dsrc'][:, q * C:(q + 1) * C]
        if acc_src & (1 << q):
            want = want + cv['prev'][q].double()
        ck.close(f'dsrc{q}', dsrcs[q], want, CONV_BWD_REL, key='dsrc')
    if variant == 'no_dW':
        assert torch.equal(dW.cpu(), cv['dW0']) and torch.equal(db.cpu(), cv['db0'])
    else:
        grad = torch.cat([cref['dW'], cref['dW']], 1) if dup else cref['dW']
        ck.close('dW', dW, cv['dW0'].double() + grad, CONV_BWD_REL)
        ck.close('dbias', db, cv['db0'].double() + cref['dbias'], CONV_BWD_REL)
    ck.close('dx', dx, want_dx, BWD_REL)
    if not same:
        ck.close('dy', dy, want_dy, BWD_REL)
    _tails_untouched(**tails)
    unchanged = torch.equal(dV_dev.cpu(), cv['dV'])
    if not with_bn or (family is not None and not _FORCED):
        assert unchanged, 'the launch wrote to its dU / dV operand'
    elif not (unchanged and _FORCED):
        ck.close('dU in place', dV_dev, dU_ref, CONV_BWD_REL, key='dU_in_place')
    ck.finish()
