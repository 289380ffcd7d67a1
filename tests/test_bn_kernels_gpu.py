"""The BatchNorm finalisers and BatchNorm tails of csrc/bn_fin.hpp and csrc/bnmix.hip, kernel by kernel, through the C ABI
(bmnas.lib) against the float64 statement in tests/bn_ref.py (pinned by tests/test_bn_ref.py on the CPU): bn_fin_fill
inside bmnas_bn_relu_fwd / _mish_fwd / _glu_fwd / _relu_fwd_group, bmnas_bn_finalize, the three forward and three
backward tails, the two grouped kernels and bmnas_bn_bwd_apply.  The module-level tests run production shapes with
randn inputs; here are the smallest shapes at which each path of these kernels exists.

How every case is checked
  * every output is a view into a larger NaN buffer, GUARD elements on each side, that must be bit-unchanged afterwards
    (gpu_util.Pool.check); the int64 counters sit in a guarded buffer of their own;
  * every accumulated output (bn_grad, running_mean, running_var, num_batches_tracked) starts from a random previous
    value that the expectation includes;
  * every input that must not be written (U, g, the sums / partials, the affine parameters, `chan` where it is given,
    the running statistics and counters in eval mode) is compared bit for bit afterwards;
  * dropout masks are the kernels' own (lib.dropout_mask at the same site, p = 0.3, a non-zero offset);
  * nothing is excluded from a comparison.  gpu_util.assert_close_scaled at the bounds of tests/test_conv_kernels_gpu.py:
    forward outputs, chan, running statistics 2e-5, dV and phase B 3e-5, bn_grad 5e-5, counters exact.  The four
    quarters of chan are compared one by one, and channels that are constant over the batch (rstd = 316) apart from
    the others, so that no tensor is judged by another one's scale.

Inputs.  U is drawn in float64 and rounded once to float32; the sums of d = U - bias and d^2 (the partials of
bmnas_bn_finalize) are computed from that float32 U in float64, split across the shards into parts of both signs
(0.1 .. 0.6 of the total each, the last shard takes the rest: a dropped shard moves the result by >= 10 %), rounded to
float32, and the expectation is computed from the ROUNDED values: these tests check the finalisation, not the GEMM
epilogue that produces the sums.  The backward cases take chan as a given float32 input (on = 0) and build U from a
target v = sign (0.05 + |n|) as U = (v - shift) / scale, so no ReLU decision is within round-off of zero (_Given checks
|v| >= 0.04 on the float64 evaluation of the rounded U for every case); one channel with shift = 0 also holds exact
U = 0 elements, whose ReLU gradient must be exactly 0.

  A  bn_fin_fill through bmnas_bn_relu_fwd, on = 1, training: M 4, 8, 12 (one thread, two, three), 1024 (4 x 256: exactly
     one trip), 1028 (the second trip is thread 0 alone), 4096 (the limit: four trips); (b, L) = (1, 4) (N 4: the
     unbiased factor 4 / 3), (1, 12) (forward only: the backward entries refuse L 12), (3, 8), and (8, 8) at M 64
     (four workgroups: the running statistics and counters move exactly once); shards 1 .. 4; conv_bias given / NULL;
     running statistics given / NULL; counters NULL or 1, 2, 4 (and 6 at M 8: the counters of the second thread) starting
     at 7 and 2^33 + 5.  Channels with |E d| / std about 0, 1, 3 in turn; where N is a power of two, two channels that
     are exactly constant (d = 0.5 and d = 0: var exactly 0 in float32, rstd = 1 / sqrt(1e-5), the output is bn_b);
     sums that round-off left inconsistent (E d^2 < (E d)^2: the clamp); one case at r ~ 20 under the law already
     pinned by tests/test_numerics_gpu.py, 2.5e-7 r^2 + 2e-6 of scale with r measured on the float64 evaluation.
  B  the same finaliser in bmnas_bn_mish_fwd, bmnas_bn_glu_fwd (C 2, 4, 512, 2048: M = 2 C up to the limit) and
     bmnas_bn_relu_fwd_group (n 1, 3, 8: each problem its own descriptor, training and eval mixed in one launch,
     distinct counter widths; b 64, M 128, L 16, n 8: the 768 / n grid cap makes every workgroup walk several
     rounds), training and eval (eval at M 4 too), and on = 0 (chan given, the output comes from it).
  C  bmnas_bn_finalize: M 1, 3, 5, 64 (a grid of one, waves without a channel, counters up to M); n_part 1 (N 2 and N 4),
     2 (16 + 8 columns), 16, 64, 65, 256, 257 (the first partial that is re-read instead of kept in registers), 300;
     ragged last partials, running statistics NULL, counters NULL, eval; U with |mean| / std up to 30 — Chan's rule does
     not follow the r^2 law, so the bound at r 30 is the bound at r 0: the case that tells the two finalisers apart.
  D  tails forward, on = 0: relu, mish (v over -30 .. 30, both sides of 20), glu (gates over -30 .. 30, one channel at
     +100 and one at -100: finite, equal to va m and to 0), L 4, 8, 16, dropout on / off; per kernel one case of
     b 129, M 1024 (C 1024), L 16: more than 2048 x 256 float4, the grid-stride loop.
  E  tails backward: M L / 4 = 4 (one partly filled 64-column block), 20, 72 (the second block has 8 active columns),
     2048; L 4, 8, 16 (row reductions over 1, 2, 4 lanes); b 1, 2, 3 (fewer samples than the four sample lanes), 5, 9,
     and b 33, M 512, L 16 (pick_chunk gives 8, the last chunk holds one sample); dropout on / off; bn_grad accumulated
     onto a random value.  bmnas_bn_relu_bwd_group: n 1, 3, 8, a chunk of 4 and a chunk of 8, a dropout site per problem.
  F  bmnas_bn_bwd_apply in place: training and eval, L 4, 8, 16, M 4 / b 1 and a grid-stride case; in eval U and bn_grad
     hold NaN (the launcher refuses NULL there, tests/test_bn_host_contract.py): they are not read.

Findings of these cases and of reading the kernels for them (fixed in the same change):
  1. bmnas_bn_relu_fwd, bmnas_bn_mish_fwd and bmnas_bn_glu_fwd accepted M (2 C) % 4 != 0, which bmnas_bn_relu_fwd_group
     refuses: bn_fin_fill then writes sc[M ..] over sh[0 ..] in LDS through misaligned float4 stores.  They now return
     BMNAS_E_LIMIT like the grouped entry (tests/test_bn_host_contract.py; no such launch is made here).
  2. bn_fin_fill in eval mode at M = 4 read its two dummy float4 from bn_w[0 .. 7], 16 bytes past the tensor (the values
     are discarded).  The second load now repeats the first there; no predicated load was added (eval at M 4 below).
  3. bn_fin_fill's comment claimed n_nbt <= 4; the code gives thread t the counters 4 t .. 4 t + 3 below n_nbt, i.e.
     n_nbt <= M, like bn_finalize_k — the comment was corrected, and n_nbt 6 at M 8 is a case here.

A property of the inputs, not of the kernels: the backward cases draw |bn_w| from 0.4 .. 1.6.  With a weight that falls
next to 0, U = (v - shift) / scale puts u_hat at ~1e4 and a channel's sum of dV u_hat becomes 1600 of cancelling terms
for a result of 1 (measured at b 2, C 5, L 16 with bn_w = -0.001: the kernel off by 5.7e-5 of scale, a float32 CPU
evaluation of the same case by 3.1e-5).

Evidence that the tests bite — value-only mutations (none moves an address or changes a launch shape), each built into
a scratch copy of the library and this file run once against it on an MI355X (201 cases, 4 s; with the committed
kernels all pass):
   1. bn_fin_fill, N / (N - 1) -> 1: 42 fail — every training case that tracks running statistics (A: 16 + 12 + 2 + the
      r 20 case, B: 6 mish / glu + all 5 groups).
   2. bn_fin_fill, the shard sum stops at 3: 17 fail — exactly the cases with 4 shards (8 of A, 3 at N 32, the r 20 case,
      the 5 groups).
   3. bn_fin_fill, mean without + conv_bias: 41 fail — every training case with a bias.
   4. bn_fin_fill, the fmaxf(var, 0) clamp removed: 2 fail — test_fin_fill_clamps_a_variance_that_round_off_left_negative
      (rstd NaN); sums of a real U never get there at these sizes, so only the constructed sums separate it.
   5. bn_finalize_k, cnt always 16: 7 fail — the training cases with a ragged last partial (N 2, 4, 24, 24, 1032, 4104,
      4792); the full ones pass.
   6. bn_finalize_k, the re-read loop starts one stride late (the m2 pass; the same for the sum pass): 4 fail each — the
      cases with more than 256 partials (257 ragged, 257 full, 300 ragged, 300 full).
   7. bn_finalize_k, the cnt d^2 term dropped: 11 fail — every training case with more than one partial.
   8. bn_relu_bwd_body, v >= 0 for v > 0: 30 fail — every ReLU backward case (26 single, 4 groups): the exact zeros.
   9. bn_relu_bwd_body, csum[2] not added: 23 fail — the ReLU and Mish cases with b >= 4 in a chunk (b 5, 9, 33: 20
      single, 3 groups).
  10. bn_relu_bwd_body, row_sum skipped: 38 fail — the ReLU and Mish cases with L 8 and 16 (36 single, 2 groups).
  11. glu_grad without (1 - sg): 26 fail — every GLU backward case.
  12. mish_t, threshold 20 -> 10: NONE fails, and no case can: q / (q + 2) already rounds to 1.0f at u = 9 (q = 6.6e7, the
      quotient is 1 - 3e-8), so the forward is bit-identical, and dact_f moves by 4 u / q <= 9e-8, one ulp of 1.  The
      nearest threshold float32 can see, 5, fails 30: every Mish backward case (26) and 4 Mish forward cases of B.
  13. bn_bwd_apply_k, the eval branch takes the training formula: 6 fail — every eval case (NaN from U and bn_grad).
  14. bn_relu_fwd_group_k, the problem index always 0: 4 fail — every group with more than one problem.
   0. the library of the parent commit: none fails.  Finding 1 is a refusal (tests/test_bn_host_contract.py pins it; its
      M % 4 rows were not run against the parent library), finding 2 an out-of-bounds READ of values that are thrown
      away, finding 3 a comment: none of them changes a value these cases can see.
"""
import pytest
import torch

import bn_ref as br
from gpu_util import Pool, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

R_FWD, R_DV, R_GRAD = 2e-5, 3e-5, 5e-5
DROP_P, DROP_SEED, DROP_OFFSET = 0.3, 0x1234567890ABCDEF, 4099
F64 = torch.float64
NAN = float('nan')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _drop(site, on=True):
    from bmnas import lib
    return lib.make_dropout(DROP_P, DROP_SEED + site, DROP_OFFSET + 1000003 * site) if on else lib.NO_DROP


def _mask(drop, numel):
    from bmnas import lib
    return lib.dropout_mask(drop, numel, dev()).cpu()


def _same(name, t, ref):
    """an input (or an eval-mode buffer) was not written: bit for bit"""
    a, b = t.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    view = torch.int64 if a.dtype == torch.int64 else torch.int32
    assert torch.equal(a.view(view), b.view(view)), f'{name} was written'


def _close_rows(name, got, want, apart, rel):
    """per-channel vectors: the channels `apart` (constant over the batch: another scale) and the rest, each in full"""
    got, want = got.detach().cpu().double(), want.double()
    rest = [i for i in range(want.numel()) if i not in apart]
    assert_close_scaled(name, got[rest], want[rest], rel=rel)
    if apart:
        assert_close_scaled(name + ' (constant channels)', got[list(apart)], want[list(apart)], rel=rel)


def _split(S, shards, g, exact):
    """(M, 2) float64 totals -> (shards, M, 2) float32 parts of both signs that add up to them; rows `exact` in quarters
    (their float32 sums are exact in any order)"""
    M = S.shape[0]
    w = (0.1 + 0.5 * torch.rand(max(shards - 1, 0), M, 2, generator=g, dtype=F64))
    w = w * torch.where(torch.rand(max(shards - 1, 0), M, 2, generator=g) < 0.5, -1.0, 1.0).double()
    parts = w * S[None]
    for i in exact:
        parts[:, i] = torch.round(parts[:, i] * 4.0) / 4.0
    stat = torch.cat([parts, (S - parts.sum(0))[None]], 0)
    stat = stat[torch.randperm(shards, generator=g)]               # the remainder sits in a random shard
    return stat.float()


def _counters(n):
    return torch.tensor([(7, 2 ** 33 + 5)[i % 2] + i // 2 for i in range(n)], dtype=torch.int64)


# ------------------------------------------------------------------------------------------- forward, with finalisation
class _Fwd:
    """One forward problem of bmnas_bn_relu_fwd | _mish_fwd | _glu_fwd (M = 2 C there): the inputs on the device, the
    outputs in `pool`, the float64 expectation.  mode 'train' | 'eval' (on = 1) | 'given' (on = 0: chan is an input)."""

    def __init__(self, pool, kind, M, b, L, seed, *, mode='train', shards=4, bias=True, running=True, n_nbt=1,
                 const=False, neg_var=False, ratios=(0.0, 1.0, 3.0), drop=None, eval_stat=False):
        from bmnas import lib
        g = _gen(1000 * seed + 7 * b + 3 * M + L + shards)
        self.kind, self.M, self.b, self.L, self.mode, self.pool = kind, M, b, L, mode, pool
        N = b * L
        std = 0.5 + _randn(g, M).abs()
        r = torch.tensor([ratios[i % len(ratios)] * (1.0 if (i // len(ratios)) % 2 == 0 else -1.0) for i in range(M)],
                         dtype=F64)
        z = _randn(g, b, M, L)                                       # standardised per channel: at N = 4 the SAMPLE ratio
        z = (z - z.mean(dim=(0, 2), keepdim=True)) / z.var(dim=(0, 2), unbiased=False, keepdim=True).sqrt()
        d = (z + r[None, :, None]) * std[None, :, None]             # |E d| / std is r, not what four draws make of it
        cb = (_randn(g, M) * 2.0 + 1.0).float()
        bn_w, bn_b = (1.0 + 0.3 * _randn(g, M)).float(), (0.5 * _randn(g, M)).float()
        self.apart = ()
        if const:
            assert N & (N - 1) == 0 and M >= 4, 'a constant channel is exact only where 1 / N is'
            d[:, 1], d[:, 2] = 0.5, 0.0
            cb[1], cb[2], bn_b[1] = 0.0, 0.25, 0.5
            self.apart = (1, 2)
        U = (d + cb.double()[None, :, None]).float() if bias else d.float()
        rm, rv = _randn(g, M).float(), (0.5 + _randn(g, M).abs()).float()
        nbt = _counters(n_nbt) if n_nbt else None
        training = mode == 'train'
        have_run = running or mode == 'eval'
        self.cpu = dict(U=U, cb=cb, bn_w=bn_w, bn_b=bn_b, rm=rm, rv=rv, nbt=nbt)
        stat = None
        if training:
            S = br.sums_of(U, cb if bias else None, 1)[0]
            if neg_var:                                           # dm = 2, E d^2 = 3.875 = dm^2 - 0.125, exact in float32
                assert N & (N - 1) == 0
                S[3, 0], S[3, 1] = 2.0 * N, 3.875 * N
                self.apart = self.apart + (3,)
            stat = _split(S, shards, g, self.apart)
        if mode == 'eval' and eval_stat:                          # a pointer and a shard count that eval must not use
            stat = torch.full((shards, M, 2), NAN)
        self.cpu['stat'] = stat
        if mode == 'given':
            chan32 = br.bn_eval_chan(bn_w, bn_b, rm, rv).float()
            self.want = {'chan': chan32.double()}
            self.chan = pool.new(4 * M, base=chan32)
            self.cpu['chan'] = chan32
            self.fin = lib.NO_FIN
        else:
            self.want = br.fin_from_sums(stat.double() if training else None, cb if bias else None, bn_w, bn_b,
                                         rm if have_run else None, rv if have_run else None, nbt, N, training)
            self.chan = pool.new(4 * M)
            self.d = {k: (None if v is None else v.to(dev())) for k, v in self.cpu.items() if k not in ('U', 'nbt')}
            self.rm = pool.new(M, base=rm) if have_run else None
            self.rv = pool.new(M, base=rv) if have_run else None
            self.nbt = pool.new_i64(nbt) if n_nbt else None
            p = lambda t: None if t is None else t.data_ptr()
            self.fin = lib.BnFin(p(self.d['stat']), p(self.d['cb']) if bias else None, p(self.d['bn_w']), p(self.d['bn_b']),
                                 p(self.rm), p(self.rv), p(self.nbt), shards if stat is not None else 0, n_nbt, int(training), 1)
        self.bias = bias
        self.Ud = U.to(dev())
        Mo = M // 2 if kind == 'glu' else M
        self.out = pool.new(b, Mo, L)
        self.drop = drop if drop is not None else lib.NO_DROP
        mask = _mask(self.drop, b * Mo * L) if self.drop.thr else None
        c = self.want['chan']
        self.want_out = br.tail_fwd(kind, U, c[2 * M:3 * M], c[3 * M:], mask)
        self.ratio = float(((d.mean(dim=(0, 2))).abs() / d.var(dim=(0, 2), unbiased=False).sqrt().clamp(min=1e-30)).median())

    def run(self):
        from bmnas import lib
        if self.kind == 'glu':
            lib.bn_glu_fwd(self.Ud, self.chan, self.out, self.b, self.M // 2, self.L, self.drop, self.fin)
        else:
            (lib.bn_relu_fwd if self.kind == 'relu' else lib.bn_mish_fwd)(self.Ud, self.chan, self.out, self.b, self.M,
                                                                          self.L, self.drop, self.fin)
        return self

    def check(self, rel=R_FWD):
        """after pool.check()"""
        M, w = self.M, self.want
        _same('U', self.Ud, self.cpu['U'])
        if self.mode == 'given':
            _same('chan (on = 0)', self.chan, self.cpu['chan'])
        else:
            for q, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
                _close_rows('chan: ' + name, self.chan[q * M:(q + 1) * M], w['chan'][q * M:(q + 1) * M], self.apart,
                            R_FWD if name == 'mean' else rel)
            for k in ('stat', 'cb', 'bn_w', 'bn_b'):
                if self.cpu[k] is not None:
                    _same(k, self.d[k], self.cpu[k])
            if self.mode == 'eval':
                _same('running_mean (eval)', self.rm, self.cpu['rm'])
                _same('running_var (eval)', self.rv, self.cpu['rv'])
            elif self.rm is not None:
                assert_close_scaled('running_mean', self.rm, w['rm'], rel=R_FWD)
                _close_rows('running_var', self.rv, w['rv'], (), rel)
            if self.nbt is not None:
                assert torch.equal(self.nbt.cpu(), w['nbt']), ('num_batches_tracked', self.nbt.cpu(), w['nbt'])
        rest = [i for i in range(self.want_out.shape[1]) if i not in self.apart or self.kind == 'glu']
        assert_close_scaled('out', self.out[:, rest], self.want_out[:, rest], rel=rel)
        if len(rest) < self.want_out.shape[1]:
            assert_close_scaled('out (constant channels)', self.out[:, list(self.apart)], self.want_out[:, list(self.apart)],
                                rel=rel)
        if 1 in self.apart and self.kind == 'relu' and not self.drop.thr:      # the constant channel: out = bn_b = 0.5
            assert_close_scaled('out of the constant channel', self.out[:, 1], torch.full((self.b, self.L), 0.5, dtype=F64),
                                rel=2 * R_FWD)


def _one_fwd(kind, M, b, L, seed, **kw):
    pool = Pool()
    p = _Fwd(pool, kind, M, b, L, seed, **kw).run()
    pool.check()
    p.check()
    return p


#            M, b, L, shards, bias, running, n_nbt
FIN_CASES = [(4, 1, 4, 1, True, True, 1), (4, 1, 4, 4, False, False, 0), (4, 3, 8, 3, True, True, 4),
             (4, 1, 12, 2, True, True, 2),
             (8, 1, 4, 2, True, True, 2), (8, 1, 12, 4, False, True, 0), (8, 3, 8, 1, True, False, 4),
             (8, 3, 8, 4, True, True, 6), (8, 3, 8, 3, False, False, 1),
             (12, 1, 12, 3, True, True, 1), (12, 3, 8, 2, False, True, 2), (12, 1, 4, 4, True, False, 0),
             (1024, 1, 4, 4, True, True, 4), (1024, 3, 8, 3, False, True, 1), (1024, 1, 12, 1, True, False, 2),
             (1028, 1, 4, 2, True, True, 2), (1028, 3, 8, 4, True, False, 0), (1028, 1, 12, 1, False, True, 4),
             (4096, 1, 4, 4, True, True, 4), (4096, 3, 8, 3, True, True, 1), (4096, 1, 12, 2, False, False, 2),
             (64, 8, 8, 4, True, True, 4), (64, 8, 8, 2, False, True, 1)]


@pytest.mark.parametrize('M,b,L,shards,bias,running,n_nbt', FIN_CASES)
def test_fin_fill_training_through_bn_relu_fwd(M, b, L, shards, bias, running, n_nbt):
    """A: chan, the running statistics, the counters and the output; constant channels where N is a power of two"""
    N = b * L
    _one_fwd('relu', M, b, L, 1, shards=shards, bias=bias, running=running, n_nbt=n_nbt, const=N & (N - 1) == 0)


@pytest.mark.parametrize('M,b,L', [(8, 2, 16), (8, 4, 8), (1028, 2, 16)])
@pytest.mark.parametrize('shards', [1, 2, 3, 4])
def test_fin_fill_constant_channels_at_n_32(M, b, L, shards):
    """A: d = 0.5 everywhere and d = 0 with N = 32: var exactly 0, rstd = 1 / sqrt(1e-5), out = bn_b"""
    p = _one_fwd('relu', M, b, L, 2, shards=shards, const=True, n_nbt=2)
    rstd = p.chan[M:2 * M].cpu()
    assert float(rstd[1]) == float(rstd[2]) and abs(float(rstd[1]) - 1e-5 ** -0.5) <= 1e-3, rstd[:4]


@pytest.mark.parametrize('bias', [True, False])
def test_fin_fill_clamps_a_variance_that_round_off_left_negative(bias):
    """A: sums with E d^2 = (E d)^2 - 0.125, every step exact in float32: var = 0, not NaN"""
    _one_fwd('relu', 8, 1, 4, 3, shards=3, bias=bias, const=True, neg_var=True, n_nbt=1)


def test_fin_fill_follows_the_pinned_law_at_r_20():
    """A: |E d| / std ~ 20 in every channel: 2.5e-7 r^2 + 2e-6 of scale (tests/test_numerics_gpu.py), r measured on the
    float64 evaluation (the median over the channels, as there)"""
    pool = Pool()
    p = _Fwd(pool, 'relu', 64, 8, 8, 4, shards=4, ratios=(20.0,), n_nbt=1).run()
    pool.check()
    assert 17.0 <= p.ratio <= 23.0, p.ratio
    bound = 2.5e-7 * p.ratio ** 2 + 2e-6
    assert bound <= 1.4e-4
    p.check(rel=bound)


FIN_ELSEWHERE = [('mish', 4), ('mish', 12), ('mish', 1028), ('glu', 4), ('glu', 8), ('glu', 1024), ('glu', 4096)]


@pytest.mark.parametrize('mode', ['train', 'eval', 'eval, stat NULL'])
@pytest.mark.parametrize('kind,M', FIN_ELSEWHERE)
def test_fin_fill_in_the_mish_and_glu_tails(kind, M, mode):
    """B: bmnas_bn_mish_fwd, bmnas_bn_glu_fwd with C 2, 4, 512, 2048; eval at M 4: the dummy loads stay inside bn_w"""
    b, L = (3, 8) if M % 8 else (2, 16)
    _one_fwd(kind, M, b, L, 5, mode=mode.split(',')[0], shards=3, n_nbt=2, drop=_drop(3, M == 8), running=M != 12,
             eval_stat=mode == 'eval')


@pytest.mark.parametrize('kind,M,b,L', [('relu', 4, 1, 4), ('relu', 1028, 3, 8), ('relu', 4096, 1, 12), ('mish', 8, 3, 8),
                                        ('glu', 4, 1, 4), ('glu', 4096, 2, 16)])
def test_forward_tails_eval_and_given_chan(kind, M, b, L):
    """B: eval through bmnas_bn_relu_fwd (M 4 included) and on = 0 at the same shapes"""
    _one_fwd(kind, M, b, L, 6, mode='eval', n_nbt=1, drop=_drop(4, M == 4))
    _one_fwd(kind, M, b, L, 6, mode='given', drop=_drop(5, M != 4))


GROUPS = {'n 1': (1, 3, 8, 8), 'n 3': (3, 1, 4, 4), 'n 3, M 1028': (3, 3, 1028, 8), 'n 8': (8, 2, 12, 16),
          'n 8, grid cap': (8, 64, 128, 16)}


@pytest.mark.parametrize('case', list(GROUPS))
def test_bn_relu_fwd_group(case):
    """B: every problem its own descriptor: training / eval / on = 0 in turn, shards 1 .. 4, counter widths 1, 2, 4, 0,
    bias given / NULL, its own dropout site"""
    from bmnas import lib
    n, b, M, L = GROUPS[case]
    pool = Pool()
    probs = []
    for i in range(n):
        mode = ('train', 'eval', 'train', 'given')[i % 4] if n > 1 else 'train'
        probs.append(_Fwd(pool, 'relu', M, b, L, 20 + i, mode=mode, shards=1 + (i + 3) % 4, bias=i % 3 != 1,
                          running=i % 5 != 2, n_nbt=(1, 2, 4, 0)[i % 4] if M >= 4 else 1,
                          drop=_drop(10 + i, i % 2 == 0), eval_stat=i % 8 == 1))
    lib.bn_relu_fwd_group([p.Ud for p in probs], [p.chan for p in probs], [p.out for p in probs],
                          [p.fin for p in probs], [p.drop for p in probs], b, M, L)
    pool.check()
    for p in probs:
        p.check()


# ------------------------------------------------------------------------------------------------- bmnas_bn_finalize
#           M, b, L, r, running, n_nbt
FINALIZE = [(1, 1, 2, 0.0, True, 1), (3, 1, 4, 3.0, True, 3), (5, 3, 8, 30.0, True, 5), (64, 3, 8, 30.0, True, 64),
            (64, 16, 16, 10.0, False, 2), (3, 64, 16, 30.0, True, 0), (5, 129, 8, 30.0, True, 2), (5, 65, 16, 30.0, False, 0),
            (1, 256, 16, 30.0, True, 1), (3, 513, 8, 30.0, True, 1), (64, 257, 16, 20.0, True, 4), (5, 599, 8, 30.0, True, 5),
            (3, 300, 16, 0.0, True, 3)]


def _finalize_problem(M, b, L, r, seed):
    g = _gen(seed + 7 * b + 3 * M + L)
    std = 0.5 + _randn(g, M).abs()
    sign = torch.where(torch.rand(M, generator=g) < 0.5, -1.0, 1.0).double()
    U = ((_randn(g, b, M, L) + (r * sign)[None, :, None]) * std[None, :, None]).float()
    return (g, U, (1.0 + 0.3 * _randn(g, M)).float(), (0.5 * _randn(g, M)).float(), _randn(g, M).float(),
            (0.5 + _randn(g, M).abs()).float())


@pytest.mark.parametrize('M,b,L,r,running,n_nbt', FINALIZE)
def test_bn_finalize_training(M, b, L, r, running, n_nbt):
    """C: Chan's rule over the float32 partials; the bound does not depend on r"""
    from bmnas import lib
    N = b * L
    n_part = (N + 15) // 16
    _, U, bn_w, bn_b, rm, rv = _finalize_problem(M, b, L, r, 31)
    part = br.group_partials(U).float()
    nbt = _counters(n_nbt) if n_nbt else None
    want = br.fin_from_partials(part.double(), bn_w, bn_b, rm if running else None, rv if running else None, nbt, N)
    pool = Pool()
    chan = pool.new(4 * M)
    rmd, rvd = (pool.new(M, base=rm), pool.new(M, base=rv)) if running else (None, None)
    nbd = pool.new_i64(nbt) if n_nbt else None
    pd, wd, bd = part.to(dev()), bn_w.to(dev()), bn_b.to(dev())
    lib.bn_finalize(pd, n_part, b, L, M, wd, bd, rmd, rvd, nbd, True, chan)
    pool.check()
    for q, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
        assert_close_scaled('chan: ' + name, chan[q * M:(q + 1) * M], want['chan'][q * M:(q + 1) * M], rel=R_FWD)
    if running:
        assert_close_scaled('running_mean', rmd, want['rm'], rel=R_FWD)
        assert_close_scaled('running_var', rvd, want['rv'], rel=R_FWD)
    if n_nbt:
        assert torch.equal(nbd.cpu(), want['nbt']), (nbd.cpu(), want['nbt'])
    _same('part', pd, part)
    _same('bn_w', wd, bn_w)
    _same('bn_b', bd, bn_b)


@pytest.mark.parametrize('M,b,L', [(1, 1, 4), (5, 3, 8), (64, 2, 16)])
def test_bn_finalize_eval(M, b, L):
    """C: chan from the running statistics; they and the counters are left alone; part may be NULL"""
    from bmnas import lib
    _, U, bn_w, bn_b, rm, rv = _finalize_problem(M, b, L, 1.0, 37)
    nbt = _counters(min(M, 2))
    want = br.fin_from_partials(None, bn_w, bn_b, rm, rv, nbt, b * L, training=False)
    pool = Pool()
    chan = pool.new(4 * M)
    rmd, rvd, nbd = pool.new(M, base=rm), pool.new(M, base=rv), pool.new_i64(nbt)
    lib.bn_finalize(None, 0, b, L, M, bn_w.to(dev()), bn_b.to(dev()), rmd, rvd, nbd, False, chan)
    pool.check()
    for q, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
        assert_close_scaled('chan: ' + name, chan[q * M:(q + 1) * M], want['chan'][q * M:(q + 1) * M], rel=R_FWD)
    _same('running_mean (eval)', rmd, rm)
    _same('running_var (eval)', rvd, rv)
    _same('num_batches_tracked (eval)', nbd, nbt)


# ------------------------------------------------------------------------------------- tails with a given chan (on = 0)
class _Given:
    """chan as a float32 input and U = (v - shift) / scale from a target v, for the forward tails of D and the backward
    tails of E.  Mo: the output's channels (the GLU reads M = 2 Mo)."""

    def __init__(self, kind, b, Mo, L, seed, *, wide=False, far_gates=False, zeros=False):
        g = _gen(seed + 7 * b + 3 * Mo + L)
        M = 2 * Mo if kind == 'glu' else Mo
        self.kind, self.b, self.Mo, self.M, self.L = kind, b, Mo, M, L
        mean, rstd = _randn(g, M), 0.5 + _randn(g, M).abs()
        # |bn_w| in 0.4 .. 1.6, a quarter of them negative: U = (v - shift) / scale divides by it, and a weight that
        # happens to fall next to 0 makes u_hat ~ 1e4 and the channel's sums an exercise in cancellation
        bn_w = (1.0 + 0.3 * _randn(g, M)).clamp(0.4, 1.6) * torch.where(torch.rand(M, generator=g) < 0.25, -1.0, 1.0).double()
        scale = rstd * bn_w
        shift = 0.5 * _randn(g, M) - mean * scale
        zc = M - 1
        if zeros:
            shift[zc] = 0.0
        mag = _randn(g, b, M, L).abs()
        if kind == 'mish' or wide:
            mag = (mag * 10.0).clamp(max=29.95)
        elif kind == 'glu':
            mag[:, Mo:] = (mag[:, Mo:] * 10.0).clamp(max=29.95)
        v = torch.where(torch.rand(b, M, L, generator=g) < 0.5, -1.0, 1.0).double() * (0.05 + mag)
        if kind != 'relu':                                          # both sides of the softplus threshold, the ends
            edge = torch.tensor([19.5, 20.5, -19.5, -20.5, 30.0, -30.0, 19.999, 20.001], dtype=F64)
            flat = v[:, M - Mo:].reshape(-1).clone()
            flat[:min(8, flat.numel())] = edge[:min(8, flat.numel())]
            v[:, M - Mo:] = flat.reshape(b, Mo, L)
        if far_gates:
            assert kind == 'glu' and Mo >= 2
            v[:, M - 2], v[:, M - 1] = 100.0 + _randn(g, b, L), -100.0 + _randn(g, b, L)
        self.chan = torch.cat([mean, rstd, scale, shift]).float()
        c = self.chan.double()
        U = ((v - c[3 * M:][None, :, None]) / c[2 * M:3 * M][None, :, None]).float()
        self.zero = torch.zeros(b, M, L, dtype=torch.bool)
        if zeros:
            self.zero[:, zc, ::2] = True
            self.zero[0, zc] = True
            U[self.zero] = 0.0
        self.U = U
        # no activation decision within round-off: on the float64 evaluation of the ROUNDED inputs
        v64 = br.affine(U, c[2 * M:3 * M], c[3 * M:])
        assert bool(((v64.abs() >= 0.04) | self.zero).all()) and bool((v64[self.zero] == 0).all())
        assert bool(((v64 > 0) == (v > 0))[~self.zero].all())
        self.v = v64
        self.g = _randn(g, b, Mo, L).float()
        self.g[self.g.abs() < 0.1] = 0.5                            # (a wrong decision must show in dV)
        self.prev = _randn(g, 2 * M).float()


def _run_tail_fwd(kind, b, Mo, L, drop_on, site, **kw):
    from bmnas import lib
    p = _Given(kind, b, Mo, L, 41, **kw)
    M = p.M
    drop = _drop(site, drop_on)
    mask = _mask(drop, b * Mo * L) if drop_on else None
    c = p.chan.double()
    want = br.tail_fwd(kind, p.U, c[2 * M:3 * M], c[3 * M:], mask)
    pool = Pool()
    out, chan, Ud = pool.new(b, Mo, L), pool.new(4 * M, base=p.chan), p.U.to(dev())
    if kind == 'glu':
        lib.bn_glu_fwd(Ud, chan, out, b, Mo, L, drop)
    else:
        (lib.bn_relu_fwd if kind == 'relu' else lib.bn_mish_fwd)(Ud, chan, out, b, M, L, drop)
    pool.check()
    _same('U', Ud, p.U)
    _same('chan', chan, p.chan)
    assert bool(torch.isfinite(out).all())
    assert_close_scaled('out', out, want, rel=R_FWD)
    return p, out.cpu(), want, mask


@pytest.mark.parametrize('drop_on', [False, True])
@pytest.mark.parametrize('b,Mo,L', [(5, 12, 4), (3, 8, 8), (2, 4, 16)])
@pytest.mark.parametrize('kind', ['relu', 'mish', 'glu'])
def test_tails_forward_from_a_given_chan(kind, b, Mo, L, drop_on):
    """D: mish over -30 .. 30 with elements at 19.5, 20.5, 19.999, 20.001; the GLU's gates over -30 .. 30 and one
    channel each at +100 (out = va m) and -100 (out = 0: the last two gates)"""
    p, out, want, mask = _run_tail_fwd(kind, b, Mo, L, drop_on, 20 + L, far_gates=kind == 'glu')
    if kind == 'glu':
        m = torch.ones(b, Mo, L, dtype=F64) if mask is None else mask.double().reshape(b, Mo, L)
        assert_close_scaled('gate at +100: va m', out[:, Mo - 2], p.v[:, Mo - 2] * m[:, Mo - 2], rel=R_FWD)
        assert float(out[:, Mo - 1].abs().max()) <= 1e-30, 'gate at -100'


@pytest.mark.parametrize('kind', ['relu', 'mish', 'glu'])
def test_tails_forward_grid_stride(kind):
    """D: b 129, M (C) 1024, L 16: 528384 float4 > 2048 x 256, the second round of the grid-stride loop"""
    _run_tail_fwd(kind, 129, 1024, 16, True, 31, wide=kind == 'relu')


#             b, Mo, L   (Mo L / 4 = 4, 20, 72, 2048)
BWD_SHAPES = [(1, 4, 4), (2, 2, 8), (3, 1, 16), (5, 20, 4), (9, 10, 8), (2, 5, 16), (3, 72, 4), (5, 36, 8), (9, 18, 16),
              (1, 2048, 4), (2, 1024, 8), (3, 512, 16), (33, 512, 16)]


def _check_bwd(p, kind, dV, bn_grad, gd, Ud, chand, mask):
    M = p.M
    want_dV, want_grad = br.tail_bwd(kind, p.g, p.U, p.chan, mask, p.prev)
    _same('g', gd, p.g)
    _same('U', Ud, p.U)
    _same('chan', chand, p.chan)
    assert_close_scaled('dV', dV, want_dV, rel=R_DV)
    assert_close_scaled('bn_grad: sum dV u_hat', bn_grad[:M], want_grad[:M], rel=R_GRAD)
    assert_close_scaled('bn_grad: sum dV', bn_grad[M:], want_grad[M:], rel=R_GRAD)
    if kind == 'relu' and p.zero.any():
        assert p.zero.sum() >= p.L // 2 + 1 and bool((dV.cpu()[p.zero] == 0).all()), 'the ReLU gradient at v == 0 is 0'


@pytest.mark.parametrize('drop_on', [False, True])
@pytest.mark.parametrize('b,Mo,L', BWD_SHAPES)
@pytest.mark.parametrize('kind', ['relu', 'mish', 'glu'])
def test_tails_backward(kind, b, Mo, L, drop_on):
    """E: dV and the per-channel sums, accumulated onto a random bn_grad; exact U = 0 on a channel with shift = 0"""
    from bmnas import lib
    p = _Given(kind, b, Mo, L, 43, zeros=kind == 'relu')
    drop = _drop(40 + L, drop_on)
    mask = _mask(drop, b * Mo * L) if drop_on else None
    pool = Pool()
    dV, bn_grad = pool.new(b, p.M, L), pool.new(2 * p.M, base=p.prev)
    gd, Ud, chand = p.g.to(dev()), p.U.to(dev()), p.chan.to(dev())
    fn = {'relu': lib.bn_relu_bwd, 'mish': lib.bn_mish_bwd, 'glu': lib.bn_glu_bwd}[kind]
    fn(gd, Ud, chand, dV, bn_grad, b, Mo, L, drop)
    pool.check()
    _check_bwd(p, kind, dV, bn_grad, gd, Ud, chand, mask)


@pytest.mark.parametrize('n,b,M,L', [(1, 2, 4, 4), (3, 5, 12, 8), (8, 9, 20, 4), (8, 33, 64, 16)])
def test_bn_relu_bwd_group(n, b, M, L):
    """E: blockIdx.z = problem; pick_chunk(b, n M L / 4) = 4, 4, 4 and 8 (b 33: the last chunk holds one sample)"""
    from bmnas import lib
    pool = Pool()
    ps = [_Given('relu', b, M, L, 50 + i, zeros=True) for i in range(n)]
    drops = [_drop(60 + i, i % 3 != 1) for i in range(n)]
    masks = [_mask(d, b * M * L) if d.thr else None for d in drops]
    dVs = [pool.new(b, M, L) for _ in ps]
    grads = [pool.new(2 * M, base=p.prev) for p in ps]
    gds, Uds, cds = [p.g.to(dev()) for p in ps], [p.U.to(dev()) for p in ps], [p.chan.to(dev()) for p in ps]
    lib.bn_relu_bwd_group(gds, Uds, cds, dVs, grads, drops, b, M, L)
    pool.check()
    for i, p in enumerate(ps):
        _check_bwd(p, 'relu', dVs[i], grads[i], gds[i], Uds[i], cds[i], masks[i])


# ----------------------------------------------------------------------------------------------- bmnas_bn_bwd_apply
@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('b,M,L', [(1, 4, 4), (1, 4, 8), (1, 4, 16), (3, 12, 4), (5, 20, 8), (129, 1024, 16)])
def test_bn_bwd_apply_in_place(b, M, L, training):
    """F: dU over dV; in eval U and bn_grad hold NaN and must not reach the result"""
    from bmnas import lib
    p = _Given('relu', b, M, L, 71)
    g = _gen(73 + b + M + L)
    dV = _randn(g, b, M, L).float()
    grad = (_randn(g, 2 * M) * float(b * L) ** 0.5).float()
    want = br.phase_b(dV, p.U, p.chan, grad, training)
    U = p.U if training else torch.full_like(p.U, NAN)
    grad_in = grad if training else torch.full_like(grad, NAN)
    pool = Pool()
    dVd = pool.new(b, M, L, base=dV)
    Ud, cd, gd = U.to(dev()), p.chan.to(dev()), grad_in.to(dev())
    lib.bn_bwd_apply(dVd, Ud, cd, gd, b, M, L, training)
    pool.check()
    _same('U', Ud, U)
    _same('chan', cd, p.chan)
    _same('bn_grad', gd, grad_in)
    assert_close_scaled('dU in place', dVd, want, rel=R_DV)
