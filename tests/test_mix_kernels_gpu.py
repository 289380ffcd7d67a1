"""The NodeMixedOp mix kernels, kernel by kernel, through the C ABI (bmnas.lib) against the float64 statement in
tests/mix_ref.py (pinned to torch autograd by tests/test_mix_ref.py on the CPU):

    s = g0 (x + y) + g1 p1 + g2 drop(va sigmoid(vg)) + g3 drop(act(vf)),      va | vg | vf = BatchNorm(U rows)

csrc/mix_terms.hpp defines it once; seven kernel families compile it, each with its own indexing, reductions and launch
rules: node_mix_fwd_k<NP>, node_mix_ln_fwd_k<VPT, BS>, node_mix_bwd_k<NP>, node_mix_ln_bwd_k<VPT1, VPT2, 512> (bnmix.hip),
node_mix_sel_fwd_k / _bwd_k<MASK, ACT> (nodemix_sel.hip), mix_conv_fwd_k<KPW> (mixconv.hip) and mix_ep_tile (conv1x1.hip,
through bmnas_conv1x1_bwd_all_mix).  The module-level tests run production shapes against the fp32 oracle and the
kernel-against-kernel tests compare two compilations of the same header; here are the smallest shapes at which each
instantiation and edge path exists.  (node_mix_pre_fwd_k / node_mix_lnp_bwd_k of lazyln.hip stay with
tests/test_lazy_ln_kernels_gpu.py: their `pre` is bit-equal to bmnas_node_mix_ln_fwd's, which group B holds to float64.)

How every case is checked
  * every output is a view into a larger NaN buffer, GUARD floats on each side, that must be bit-unchanged afterwards
    (gpu_util.Pool.check): an edge tile that stores past its tensor fails instead of faulting;
  * every accumulated output — bn_grad, the dgamma and dw shards, destinations under an accumulate bit, dresid with
    accumulate_resid, stat, the running statistics and counters — starts from a random previous value that the
    expectation includes; dgamma / dw shards are judged by their sum, the floats between their columns bit for bit;
  * every input that must not be written is compared bit for bit afterwards (with fin.on = 0 that includes chan);
  * dropout masks are the kernels' own (lib.dropout_mask at the same two sites, p 0.1 and 0.2, non-zero offsets);
  * fin.on = 1: the batch sums are float32 inputs built as in tests/test_bn_kernels_gpu.py — float64 sums of the float32
    U about the conv bias, split over the shards into parts of both signs — and the expectation is computed from the
    rounded values; fin.on = 0: chan is a given float32 input (the batch statistics of U, rounded);
  * gamma and the next-step weights come from randn (negative entries, no softmax: a swapped column is visible), one case
    per direction has a zero column; a quarter of the BatchNorm weights are negative, |bn_w| in 0.4 .. 1.6;
  * ReLU margin: mix_ref.clear_fc_relu chooses bn_b of the FC rows on the CPU so that no vf lies within 1e-3 of zero;
    every case asserts the margin reached on the float64 evaluation of the rounded inputs (_Mix.margin).  Nothing is
    left out of a comparison.  One exact element per backward family: a channel with shift = 0 holds U = 0 in its FC row
    (vf = 0 exactly, excluded from the margin and from nothing else), and its df must be exactly 0.

Bounds (gpu_util.assert_close_scaled; those tests/test_bn_kernels_gpu.py and tests/test_conv_kernels_gpu.py hold for the
same kind of quantity): forward outputs (s, z_next, pre, mix_out, V) and chan 2e-5; data gradients (dV, dx, dy, dprev,
g_out, g_in, dresid, dsrcs) 3e-5; bn_grad, dW, dbias, the sums of stat 5e-5, its second moments 2e-4; LayerNorm outputs,
stats and out_sums 1e-4 as in tests/test_lazy_ln_kernels_gpu.py; the offset case under that file's offset rule,
max(1e-4, 3 x the error of bmnas_node_mix_fwd + bmnas_cat_ln_fwd as separate launches against the same float64
reference) — measured: out 2.4e-7 both, S(o) 6.5e-5 both.  Scalar reductions over a whole tensor (dgamma, dw) can cancel
and have no scale of their own: |got - want| <= 5e-5 x (float64 sum of the absolute values of their terms).  No bound
needed a measured replacement: every case passes at the bounds above.

  A  bmnas_node_mix_fwd / _fwd_next, node_mix_fwd_k<0..5>.  (C, L, b) = (4, 4, 1): four float4, one wave of one workgroup;
     (16, 8, 3); (48, 12, 5): the forward takes L 12 (three float4 per row); (20, 16, 5): 3 C = 60, the last thread of
     bn_fin_fill's 15.  x is y and distinct; fin on in training (1 and 4 shards, conv_bias given / NULL), on in eval, off;
     dropout on / off; n_prev 0 .. 5 with w_stride 1 and 2, prev[1] aliasing prev[0].  b 129, C 1024, L 16: 528 384 float4
     against stream_grid's 2048 x 256 — the grid-stride loop — and M = 3072: three trips of bn_fin_fill<256>; fin on,
     n_prev 2.
  B  bmnas_node_mix_ln_fwd: BS = 512 iff b <= 256 and C L / 4 >= 512, VPT = the first of 1, 2, 3, 4, 8 that covers
     ceil(C L / 4 / BS).  One case per instantiation at L 16 (B_CASES names each); b 257 selects BS 256 at any width:
     <3,256> C 192, <4,256> C 256, <8,256> C 320 (need 5).  b 1 and 5 elsewhere, out_sums given / NULL, fin on / off, dropout.
  C  bmnas_node_mix_bwd / _bwd_next, node_mix_bwd_k<0..5>: 64 float4 slots x 4 sample lanes per workgroup.  C L / 4 = 4
     (C 4, L 4), 40 (C 20, L 8), 80 (C 20, L 16: the second 64-slot block holds 16 active slots); L 4, 8, 16: row
     reductions over 1, 2, 4 lanes; b 1, 2, 3 (fewer samples than sample lanes), 5, 9; b 33, C 512, L 16: 32 column blocks
     x ceil(33 / 8) = 160 >= 128, so pick_chunk gives 8 and the last chunk holds one sample.  dgamma NULL, 1 shard, 3 shards
     of stride 8; dx / dy in all nine combinations of NULL, overwrite and accumulate (dy NULL puts 2 g0 g into dx); the rider
     with gz2 and g_in NULL / given, g_out == g_in, a NULL dprev in the middle, accumulate bits, dprev[1] == dprev[0]
     (overwrite then accumulate, and accumulate then overwrite), dw in 1 and 3 shards with unused floats between strides.
  D  bmnas_node_mix_ln_bwd: C L / 4 <= 512 <1,1>, <= 1024 <2,1>, else <4,2>; two workgroups per sample, each half
     C L / 8 float4.  <1,1>: C 2, L 4 (each half one float4), C 6, L 8, C 128, L 16 (512, exact); <2,1>: C 130 (520, its lower
     boundary) and C 256 (1024, exact); <4,2>: C 258 and C 512 (2048, the limit).  b 1, 3, 128 (the limit); g_in NULL /
     given; dresid NULL / overwrite / accumulate; dx / dy masks; dgamma NULL, 1 and 3 shards; dropout.  b 129 and C 514 at
     L 16 return BMNAS_E_LIMIT with every output still NaN.
  E  bmnas_node_mix_sel_act_fwd / _bwd at (b, C, L) = (5, 16, 8): all 15 masks with ReLU and the 8 FC masks with Mish (23
     instantiations per direction), each with identity gamma columns (chan given) and with the present kinds reversed
     (finalisation in the forward kernel over M = C | 2 C | 3 C rows), dropout on at every site the mask has; three more
     without dropout, in eval.  U holds only the present rows.  Mish backward: vf spans -30 .. 30.  ['Sum'] alone at C 3,
     L 4, b 2 (C L / 4 = 3) and at L 12 forward only.  No-Sum masks: dx (bit clear) zero-filled, dy (bit set) bit-unchanged.
     Backward edges b 3 and C 80, L 4 (C L / 4 = 80) at masks 12 and 9, both activations.
  F  bmnas_node_mix_conv_fwd: kpw = ceil((n_src + 1) C / 16 / 4) picks mix_conv_fwd_k<2 | 3 | 4 | 6 | 8 | 12>: (n_src, C) =
     (1, 64) 2, (2, 64) 3, (3, 64) 4, (2, 128) 6, (3, 128) 8, (2, 192): 36 blocks, kpw 9 runs <12> with 12 block slots past
     the end of K, (2, 256): 48 blocks fill <12>; (3, 256): kpw 16, refused.  L 4 with b 7, L 8 with b 3 (ragged last
     n-group, clamped), L 16 with b 2; ldw = K and K + 4; stat NULL, 1 and 3 shards; fin on (training, eval) / off; dropout.
  G  the mix backward as the epilogue of bmnas_conv1x1_bwd_all_mix: b 5, L 8, M = C_src = C in 16, 80, 256 (kpw 1, 2, 4 of
     conv_bwd_pair_k, group H of tests/test_conv_kernels_gpu.py), mix source q = 0 and q = last, accumulate_dx 0 / 1,
     1 / 3 dgamma shards, dropout on / off, against conv_ref.conv_bwd_data then mix_ref.mix_bwd on that source's gradient.
     bmnas_conv_family_calls must name bwd_pair alone; only that assertion is dropped under a BMNAS_* family override.

Findings
  1. (reading, before any case ran) bmnas_node_mix_fwd_next (hence bmnas_node_mix_fwd), bmnas_node_mix_ln_fwd and
     bmnas_node_mix_pre_fwd accepted any C >= 1 and launched with 6 C floats of dynamic LDS, but bn_fin_fill gives thread
     t the channels 4 t .. 4 t + 3: with (3 C) % 4 != 0 its last thread writes sc[M ..] over sh[0 ..] through misaligned
     16-byte stores and, with fin.on = 1, 1 to 3 floats past chan; C > 2730 was a raw launch error.  The three entries
     now return BMNAS_E_LIMIT for (3 C) % 4 != 0 or 3 C > 4096, before their b == 0 return (include/bmnas_hip.h states
     it; tests/test_mix_host_contract.py pins it; no such shape is launched here).  No production caller passes such a
     C.  The backward entries read chan per channel and keep taking any C (groups C and D run C 2, 4, 6, 20, 130).
  The cases themselves found no wrong value: all 123 pass against the library of the parent commit as well.

Evidence that the tests bite — value-only mutations (none moves an address, changes a launch shape or a bound), each built
into a scratch copy of the library and this file run once against it on an MI355X (123 cases, 4.1 s wall for the file;
with the committed kernels all pass, also under BMNAS_FUSE_BWD_PAIR=0):
   1. mix_fwd, g2 and g3 swapped: 81 fail — all of A (11), B (12), F (7) and the 51 selected-term cases with a conv term.
   2. glu_grad without (1 - sg): 54 fail — C (11), G (12), the 31 selected-term cases with LinearGLU; D passes because
      node_mix_ln_bwd_k writes the block out (its own mutation is 7).
   3. mix_dxy_store, the factor 2 of dy == NULL dropped (both forms): 9 fail — the cases with dx given and dy NULL: 3 of
      C, 5 of D, ['Sum'] alone.
   4. node_mix_bwd_k, sample walk s += 4 -> s += 8: 1 fails — b 33, the only chunk of 8 (with a chunk of 4 a lane walks
      one sample, and the mutation computes the same).
   5. row_sum without its l4n >= 4 step: 10 fail — the L 16 cases of C (5) and D (5).
   6. node_mix_ln_fwd_k, inv_d from cl4 * 4 - 1: 12 fail — all of B.  (From C L = 5120 on, 1 / (C L - 1) against 1 / (C L)
      moves mean, rstd and out by less than 2e-4 of themselves, inside 1e-4 (|want| + max |want|): there it is S(o), a
      cancelling sum, that fails, so every case of C >= 320 asks for out_sums.)
   7. node_mix_ln_bwd_k, the m2 term dropped: 8 fail — all of D.
   8. node_mix_sel_bwd_k, dgamma to column q instead of sel.col[q]: 51 fail — every selected-term case whose columns are
      not the kind indices.
   9. mix_conv_fwd_k, the !vb zeroing removed: 1 fails — (2, 192), the only shape with block slots past the end of K.
  10. the next-step rider, wn[NP] -> wn[0]: 8 fail — the cases of C with n_prev >= 1.
   0. the library of the parent commit: none fails here; tests/test_mix_host_contract.py fails against it on exactly
      the rows C = 1, 2, 3, 5, 6 and 1368 of the three forward entries (bmnas_node_mix_pre_fwd: all but 1368, which
      bmnas_lazy_ln_ok already refused).
"""
import os

import pytest
import torch

import bn_ref as br
import conv_ref as cr
import lazy_ln_ref as lr
import mix_ref as mr
from gpu_util import Pool, assert_close_scaled, dev

pytestmark = pytest.mark.gpu

R_FWD, R_DV, R_GRAD, R_M2, R_LN, R_DOT = 2e-5, 3e-5, 5e-5, 2e-4, 1e-4, 5e-5
E_LIMIT = r'rc=-3\)'
F64 = torch.float64
NAN = float('nan')
KINDS = ('Sum', 'ScaleDotAttn', 'LinearGLU', 'ConcatFC')


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(g, *shape):
    return torch.randn(*shape, generator=g, dtype=F64)


def _f32(g, *shape):
    return _randn(g, *shape).float()


def _d(t):
    return None if t is None else t.to(dev())


def _same(name, t, ref):
    """an input was not written: bit for bit"""
    a, b = t.detach().cpu().contiguous(), ref.detach().cpu().contiguous()
    view = torch.int64 if a.dtype == torch.int64 else torch.int32
    assert torch.equal(a.view(view), b.view(view)), f'{name} was written'


def _split(S, shards, g):
    """(M, 2) float64 totals -> (shards, M, 2) float32 parts of both signs that add up to them (0.1 .. 0.6 of the total
    each, the rest in a random shard), as tests/test_bn_kernels_gpu.py builds them"""
    M = S.shape[0]
    w = (0.1 + 0.5 * torch.rand(max(shards - 1, 0), M, 2, generator=g, dtype=F64))
    w = w * torch.where(torch.rand(max(shards - 1, 0), M, 2, generator=g) < 0.5, -1.0, 1.0).double()
    parts = w * S[None]
    stat = torch.cat([parts, (S - parts.sum(0))[None]], 0)
    return stat[torch.randperm(shards, generator=g)].float()


def _drops(on, b, C, L, site=0):
    """the two dropout sites (p 0.1 and 0.2, non-zero offsets) and the kernels' own multipliers for them"""
    from bmnas import lib
    if not on:
        return lib.NO_DROP, lib.NO_DROP, None, None
    n = b * C * L
    dglu = lib.make_dropout(0.1, 1234 + site, 4099 + 1000003 * site)
    dfc = lib.make_dropout(0.2, 1234 + site, 4099 + 1000003 * site + n // 4)
    return dglu, dfc, lib.dropout_mask(dglu, n, dev()).cpu(), lib.dropout_mask(dfc, n, dev()).cpu()


def _dot_close(name, got, want, abs_sum, prev=None):
    """a scalar reduction over a whole tensor: |got - want| <= 5e-5 x (float64 sum of the absolute values of its terms)"""
    got, want, abs_sum = got.detach().cpu().double().reshape(-1), want.double().reshape(-1), abs_sum.double().reshape(-1)
    if prev is not None:
        want = want + prev.double().reshape(-1)
        abs_sum = abs_sum + prev.double().reshape(-1).abs()
    err = (got - want).abs()
    assert bool(torch.isfinite(got).all()) and bool((err <= R_DOT * abs_sum + 1e-30).all()), \
        f'{name}: got {got.tolist()} want {want.tolist()} (|terms| {abs_sum.tolist()})'


class _Mix:
    """The inputs of one mix problem on the CPU (float32, rounded once) and on the device, its BatchNorm descriptor and
    the float64 expectation of `chan`.  mode 'given' (fin.on = 0: chan is a float32 input built from the batch statistics
    of U) | 'train' | 'eval' (fin.on = 1).  mask / act / cols as in mix_ref; U holds the present rows only."""

    def __init__(self, pool, seed, b, C, L, *, mask=15, act='relu', cols=mr.IDENT, same=False, drop=False, mode='given',
                 shards=1, bias=True, zero_col=None, exact=False, mish_span=False, site=0):
        from bmnas import lib
        g = _gen(seed * 7919 + 131 * b + 17 * C + L + 1000 * mask)
        self.b, self.C, self.L, self.mask, self.act, self.cols, self.mode, self.pool = b, C, L, mask, act, cols, mode, pool
        M, fo = mr.conv_rows(mask, C)
        self.M, self.fo, self.N = M, fo, b * L
        n = bin(mask).count('1')
        x = _f32(g, b, C, L)
        y = x if same else _f32(g, b, C, L)
        p1, gamma = _f32(g, b, C, L), _f32(g, n)
        if zero_col is not None:
            gamma[zero_col] = 0.0
        self.cpu = dict(x=x, y=y, p1=p1, gamma=gamma)
        self.dv = {k: _d(v) for k, v in self.cpu.items()}
        if same:
            self.dv['y'] = self.dv['x']
        self.dglu, self.dfc, self.m2, self.m3 = _drops(drop, b, C, L, site)
        self.fin, self.chan, self.want_chan, self.margin = lib.NO_FIN, None, None, float('inf')
        self.exact = None
        if not M:
            self.cpu['U'] = self.dv['U'] = None
            return
        sgn = torch.where(torch.rand(M, generator=g) < 0.25, -1.0, 1.0).double()
        bn_w = (sgn * (0.4 + 1.2 * torch.rand(M, generator=g, dtype=F64))).float()
        bn_b = (0.2 * _randn(g, M)).float()
        cb = (_randn(g, M) * 2.0 + 1.0).float() if (mode == 'train' and bias) else None
        U = (_randn(g, b, M, L) * 1.5 + 0.3 + (0.0 if cb is None else cb.double()[None, :, None])).float()
        rm, rv = _f32(g, M), (0.5 + _randn(g, M).abs()).float()
        nbt = torch.tensor([7, 2 ** 33 + 5][:min(2, M)], dtype=torch.int64)
        stat = None
        if mode == 'given':
            Ud = U.double()
            mean = Ud.mean(dim=(0, 2))
            rstd = 1.0 / torch.sqrt(Ud.var(dim=(0, 2), unbiased=False) + 1e-5)
        elif mode == 'train':
            stat = _split(br.sums_of(U, cb, 1)[0], shards, g)
            c0 = br.fin_from_sums(stat.double(), cb, bn_w, bn_b, rm, rv, nbt, self.N, True)['chan']
            mean, rstd = c0[:M], c0[M:2 * M]
        else:
            mean, rstd = rm.double(), 1.0 / torch.sqrt(rv.double() + 1e-5)
        if exact:                                   # FC channel 1: shift = 0 (given chan) and U = 0 at two columns of every sample
            assert mode == 'given' and mask & 8 and act == 'relu'
            ce = fo + 1
            U[:, ce] = (torch.sign(_randn(g, b, L)) * (0.05 + _randn(g, b, L).abs())).float()
            U[:, ce, :2] = 0.0
            self.exact = ce
        if mish_span:                               # vf over -30 .. 30, both sides of mish's threshold 20
            assert mode == 'given' and mask & 8
            v = torch.linspace(-30.0, 30.0, b * C * L, dtype=F64)[torch.randperm(b * C * L, generator=g)].reshape(b, C, L)
            sc = (bn_w.double() * rstd)[fo:]
            U[:, fo:] = ((v - (bn_b.double()[fo:] - mean[fo:] * sc)[None, :, None]) / sc[None, :, None]).float()
        if mask & 8 and act == 'relu':
            keep = bn_b.clone()
            bn_b[fo:], _ = mr.clear_fc_relu(g, U[:, fo:], mean[fo:], rstd[fo:], bn_w[fo:], bn_b[fo:])
            if exact:
                bn_b[ce] = keep[ce]
        self.cpu.update(U=U, bn_w=bn_w, bn_b=bn_b, cb=cb, rm=rm, rv=rv, nbt=nbt, stat=stat)
        self.dv['U'] = _d(U)
        if mode == 'given':
            scale = bn_w.double() * rstd
            chan32 = torch.cat([mean, rstd, scale, bn_b.double() - mean * scale]).float()
            if exact:
                chan32[3 * M + ce] = 0.0
            self.cpu['chan'] = chan32
            self.want = {'chan': chan32.double()}
            self.chan = pool.new(4 * M, base=chan32)
        else:
            training = mode == 'train'
            self.want = br.fin_from_sums(stat.double() if training else None, cb, bn_w, bn_b, rm, rv, nbt, self.N, training)
            self.chan = pool.new(4 * M)
            self.fd = {k: _d(self.cpu[k]) for k in ('stat', 'cb', 'bn_w', 'bn_b')}
            self.rm, self.rv, self.nbt = pool.new(M, base=rm), pool.new(M, base=rv), pool.new_i64(nbt)
            p = lambda t: None if t is None else t.data_ptr()
            self.fin = lib.BnFin(p(self.fd['stat']), p(self.fd['cb']), p(self.fd['bn_w']), p(self.fd['bn_b']), p(self.rm),
                                 p(self.rv), p(self.nbt), shards if training else 0, nbt.numel(), int(training), 1)
        c = self.want['chan']
        self.scale, self.shift = c[2 * M:3 * M], c[3 * M:]
        if mask & 8 and act == 'relu':
            vf = br.affine(U[:, fo:], self.scale[fo:], self.shift[fo:]).abs()
            if exact:
                zero = torch.zeros_like(vf, dtype=torch.bool)
                zero[:, 1, :2] = True
                assert float(vf[zero].max()) == 0.0
                vf = vf[~zero]
            self.margin = float(vf.min())
        assert self.margin >= mr.RELU_MARGIN, f'a ReLU argument lies {self.margin:.2e} from zero'

    def fwd(self):
        """s in float64"""
        c = self.cpu
        return mr.mix_fwd(self.mask, self.act, self.cols, c['gamma'], c['x'], c['y'], c['p1'], c['U'],
                          self.scale if self.M else None, self.shift if self.M else None, self.m2, self.m3)

    def bwd(self, g, **kw):
        c = self.cpu
        return mr.mix_bwd(self.mask, self.act, self.cols, c['gamma'], g, c['x'], c['y'], c['p1'], c['U'],
                          self.want['chan'] if self.M else None, self.m2, self.m3, **kw)

    def check_inputs(self):
        for k in ('x', 'y', 'p1', 'gamma', 'U'):
            if self.cpu[k] is not None:
                _same(k, self.dv[k], self.cpu[k])

    def check_fin(self):
        """chan (its four quarters one by one), the running statistics and the counters; what must not be written"""
        if not self.M:
            return
        M, w = self.M, self.want
        if self.mode == 'given':
            _same('chan (fin.on = 0)', self.chan, self.cpu['chan'])
            return
        for q, name in enumerate(('mean', 'rstd', 'scale', 'shift')):
            assert_close_scaled('chan: ' + name, self.chan[q * M:(q + 1) * M], w['chan'][q * M:(q + 1) * M], rel=R_FWD)
        for k in ('stat', 'cb', 'bn_w', 'bn_b'):
            if self.cpu[k] is not None:
                _same(k, self.fd[k], self.cpu[k])
        if self.mode == 'eval':
            _same('running_mean (eval)', self.rm, self.cpu['rm'])
            _same('running_var (eval)', self.rv, self.cpu['rv'])
            _same('num_batches_tracked (eval)', self.nbt, self.cpu['nbt'])
        else:
            assert_close_scaled('running_mean', self.rm, w['rm'], rel=R_FWD)
            assert_close_scaled('running_var', self.rv, w['rv'], rel=R_FWD)
            assert torch.equal(self.nbt.cpu(), w['nbt']), ('num_batches_tracked', self.nbt.cpu(), w['nbt'])


# ------------------------------------------------------------------- A. bmnas_node_mix_fwd / _fwd_next (node_mix_fwd_k)
#          C, L, b, same, mode, shards, bias, drop, n_prev, w_stride, alias
A_CASES = [(4, 4, 1, False, 'given', 1, True, False, 0, 1, False),
           (4, 4, 1, True, 'train', 1, True, True, 1, 2, False),
           (16, 8, 3, True, 'train', 4, False, False, 2, 1, True),
           (16, 8, 3, False, 'eval', 1, True, True, 3, 2, False),
           (48, 12, 5, False, 'train', 4, True, True, 4, 1, False),
           (48, 12, 5, True, 'given', 1, True, False, 5, 2, True),
           (20, 16, 5, False, 'train', 1, False, True, 5, 1, False),
           (20, 16, 5, True, 'eval', 1, True, False, 0, 1, False),
           (20, 16, 5, False, 'given', 1, True, True, 2, 2, False),
           (16, 8, 3, False, 'train', 4, True, False, 0, 1, False),
           (1024, 16, 129, True, 'train', 4, True, True, 2, 1, False)]       # the grid-stride loop, three trips of bn_fin_fill


@pytest.mark.parametrize('C,L,b,same,mode,shards,bias,drop,n_prev,ws,alias', A_CASES)
def test_node_mix_fwd_next(C, L, b, same, mode, shards, bias, drop, n_prev, ws, alias):
    from bmnas import lib
    pool = Pool()
    m = _Mix(pool, 1, b, C, L, same=same, drop=drop, mode=mode, shards=shards, bias=bias,
             zero_col=1 if (C, mode) == (16, 'eval') else None)
    g = _gen(11 + C + n_prev)
    prevs = [_f32(g, b, C, L) for _ in range(n_prev)]
    if alias:
        prevs[1] = prevs[0]
    pd = [_d(p) for p in prevs]
    if alias:
        pd[1] = pd[0]
    w = _f32(g, (n_prev + 1) * ws)
    wd = _d(w)
    out = pool.new(b, C, L)
    z = pool.new(b, C, L) if n_prev else None
    lib.node_mix_fwd(m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan, m.dv['gamma'], out, b, C, L, m.dglu, m.dfc,
                     m.fin, nxt=(pd, wd, ws, z) if n_prev else None)
    pool.check()
    s = m.fwd()
    assert_close_scaled('s', out, s, rel=R_FWD)
    if n_prev:
        assert_close_scaled('z_next', z, mr.next_fwd(prevs, w[::ws][:n_prev + 1], s), rel=R_FWD)
        _same('w', wd, w)
        for j in range(n_prev):
            _same(f'prev[{j}]', pd[j], prevs[j])
    m.check_inputs()
    m.check_fin()


# ------------------------------------------------------------------------------------------- B. bmnas_node_mix_ln_fwd
#          C, L, b, mode, drop, sums, same         instantiation <VPT, BS>: need = ceil(C L / 4 / BS), BS = 512 iff b <= 256
B_CASES = [(4, 4, 1, 'given', False, True, False),          # and C L / 4 >= 512            <1,256> cl4 4: whole waves idle
           (64, 16, 5, 'train', True, True, True),          # <1,256> cl4 256, exact
           (80, 16, 5, 'given', True, False, False),        # <2,256> cl4 320: the second trip is partly filled
           (128, 16, 1, 'train', False, True, True),        # <1,512> cl4 512
           (192, 16, 5, 'given', True, True, False),        # <2,512> cl4 768
           (320, 16, 5, 'eval', False, True, True),         # <3,512> cl4 1280
           (448, 16, 5, 'train', True, True, False),        # <4,512> cl4 1792: the fourth trip is partly filled
           (576, 16, 1, 'given', True, True, True),         # <8,512> cl4 2304: trips 6 to 8 are empty
           (192, 16, 257, 'given', False, True, True),      # <3,256> b 257 selects BS 256 at any width
           (256, 16, 257, 'train', True, False, False),     # <4,256>
           (320, 16, 257, 'given', True, True, True)]       # <8,256> need 5


def _ln_fwd_compare(m, pre, out, stats, sums, resid, ln_w, ln_b):
    want = mr.mix_ln_fwd(m.fwd(), resid, ln_w, ln_b)
    assert_close_scaled('pre', pre, want['pre'], rel=R_FWD)
    assert_close_scaled('out', out, want['out'], rel=R_LN)
    assert_close_scaled('stats: mean', stats[:, 0], want['stats'][:, 0], rel=R_LN)
    assert_close_scaled('stats: rstd', stats[:, 1], want['stats'][:, 1], rel=R_LN)
    if sums is not None:
        assert_close_scaled('out_sums: S(o)', sums[:, 0], want['out_sums'][:, 0], rel=R_LN)
        assert_close_scaled('out_sums: S(o^2)', sums[:, 1], want['out_sums'][:, 1], rel=R_LN)
    return want


@pytest.mark.parametrize('C,L,b,mode,drop,sums,same', B_CASES)
def test_node_mix_ln_fwd(C, L, b, mode, drop, sums, same):
    from bmnas import lib
    pool = Pool()
    m = _Mix(pool, 2, b, C, L, same=same, drop=drop, mode=mode, shards=3)
    g = _gen(21 + C + b)
    resid, ln_w, ln_b = _f32(g, b, C, L), (_randn(g, C, L) * 0.3 + 1.0).float(), (_randn(g, C, L) * 0.2).float()
    rd, wd, bd = _d(resid), _d(ln_w), _d(ln_b)
    pre, out, stats = pool.new(b, C, L), pool.new(b, C, L), pool.new(b, 2)
    osum = pool.new(b, 2) if sums else None
    lib.node_mix_ln_fwd(m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan, m.dv['gamma'], rd, wd, bd, pre, out, stats,
                        b, C, L, m.dglu, m.dfc, m.fin, out_sums=osum)
    pool.check()
    _ln_fwd_compare(m, pre, out, stats, osum, resid, ln_w, ln_b)
    for k, t, ref in (('resid', rd, resid), ('ln_w', wd, ln_w), ('ln_b', bd, ln_b)):
        _same(k, t, ref)
    m.check_inputs()
    m.check_fin()


def test_node_mix_ln_fwd_offset_resid():
    """lazy_ln_ref.offset_resid (a sample mean of ~30 with part means 20 apart): max(1e-4, 3 x the error of the separate
    launches bmnas_node_mix_fwd + bmnas_cat_ln_fwd against the same float64 reference), the offset rule of
    tests/test_lazy_ln_kernels_gpu.py; both errors are printed"""
    from bmnas import lib
    b, C, L = 5, 192, 16
    pool = Pool()
    m = _Mix(pool, 3, b, C, L, same=True, drop=True)
    g = _gen(31)
    resid = lr.offset_resid(g, b, C, L).float()
    ln_w, ln_b = (_randn(g, C, L) * 0.3 + 1.0).float(), (_randn(g, C, L) * 0.2).float()
    rd, wd, bd = _d(resid), _d(ln_w), _d(ln_b)
    pre, out, stats, osum = pool.new(b, C, L), pool.new(b, C, L), pool.new(b, 2), pool.new(b, 2)
    lib.node_mix_ln_fwd(m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan, m.dv['gamma'], rd, wd, bd, pre, out, stats,
                        b, C, L, m.dglu, m.dfc, m.fin, out_sums=osum)
    s_p, out_p, stats_p, sums_p = pool.new(b, C, L), pool.new(b, C, L), pool.new(b, 2), pool.new(b, 2)
    lib.node_mix_fwd(m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan, m.dv['gamma'], s_p, b, C, L, m.dglu, m.dfc)
    lib.cat_ln_fwd([s_p], rd, wd, bd, out_p, stats_p, b, C, L, False, out_sums=sums_p)
    pool.check()
    want = mr.mix_ln_fwd(m.fwd(), resid, ln_w, ln_b)
    assert_close_scaled('pre', pre, want['pre'], rel=R_FWD)

    def err(got, ref):
        got, ref = got.detach().double().cpu(), ref.double()
        return float((got - ref).abs().max() / max(float(ref.abs().max()), 1e-30))

    for name, got, pin, ref in [('out', out, out_p, want['out']), ('mean', stats[:, 0], stats_p[:, 0], want['stats'][:, 0]),
                                ('rstd', stats[:, 1], stats_p[:, 1], want['stats'][:, 1]),
                                ('S(o)', osum[:, 0], sums_p[:, 0], want['out_sums'][:, 0]),
                                ('S(o^2)', osum[:, 1], sums_p[:, 1], want['out_sums'][:, 1])]:
        e_s, e_p = err(got, ref), err(pin, ref)
        bound = max(1e-4, 3.0 * e_p)
        print(f'offset {name}: fused {e_s:.2e}, separate launches {e_p:.2e}, bound {bound:.2e}')
        assert e_s == e_s and e_s <= bound, (name, e_s, e_p, bound)


# ------------------------------------------------------------------- C. bmnas_node_mix_bwd / _bwd_next (node_mix_bwd_k)
def _dest(pool, how, old):
    """'null' | 'ow' (NaN before, overwritten) | 'acc' (a previous value, accumulated)"""
    if how == 'null':
        return None
    return pool.new(*old.shape, base=old if how == 'acc' else None)


def _check_dxy(m, r, dx, dy, old_x, old_y):
    for name, t, old in (('dx', dx, old_x), ('dy', dy, old_y)):
        if t is None:
            continue
        if r[name + '_rule'] == 'keep':
            _same(name + ' (no Sum term, accumulate bit set)', t, old)
        elif r[name + '_rule'] == 'zero':
            assert float(t.abs().max()) == 0.0, name + ' (no Sum term, accumulate bit clear) is not zero-filled'
        else:
            assert_close_scaled(name, t, r[name], rel=R_DV)


def _check_dgamma(name, buf, prev, want, abs_sum, ncol):
    """buf (shards, stride): the shards add up to prev + want in the first ncol columns; the others are untouched"""
    if buf is None:
        return
    _dot_close(name, buf[:, :ncol].double().sum(0), want, abs_sum, prev[:, :ncol].double().sum(0))
    if buf.shape[1] > ncol:
        _same(name + ' beyond its columns', buf[:, ncol:], prev[:, ncol:])


#          C, L, b, same, drop, dg, dx, dy, n_prev, gz2, g_in, inplace, null_mid, pacc, alias, dw_shards, exact
C_CASES = [(4, 4, 1, False, False, (1, 4), 'ow', 'ow', 0, 0, 1, 0, 0, 0, 0, 1, False),         # cl4 4
           (4, 4, 2, True, True, None, 'acc', 'null', 1, 0, 0, 0, 0, 1, 0, 1, False),
           (20, 8, 3, False, True, (3, 8), 'acc', 'acc', 2, 1, 1, 0, 0, 0b10, 1, 3, False),    # cl4 40, L 8: two-lane rows
           (20, 8, 5, True, False, (1, 4), 'ow', 'null', 3, 1, 1, 1, 1, 0b101, 0, 1, True),
           (20, 16, 9, False, True, (3, 8), 'null', 'ow', 4, 0, 1, 0, 1, 0b1010, 0, 3, False),  # cl4 80: 16 slots in block 2
           (20, 16, 3, False, False, (1, 4), 'ow', 'acc', 5, 1, 0, 0, 1, 0b10101, 1, 1, True),
           (20, 16, 2, True, True, (3, 8), 'null', 'null', 0, 0, 1, 0, 0, 0, 0, 1, False),
           (20, 16, 5, False, True, None, 'acc', 'ow', 5, 0, 1, 1, 0, 0b11111, 0, 3, False),
           (4, 4, 9, False, False, (3, 8), 'ow', 'ow', 2, 1, 1, 0, 0, 0, 0, 1, True),
           (20, 8, 1, False, True, (1, 4), 'null', 'acc', 0, 0, 1, 0, 0, 0, 0, 1, False),
           (512, 16, 33, True, True, (3, 8), 'acc', 'null', 1, 1, 1, 0, 0, 1, 0, 3, False)]    # pick_chunk 8, last chunk: 1 sample


@pytest.mark.parametrize('C,L,b,same,drop,dg,dx,dy,n_prev,gz2,g_in,inplace,null_mid,pacc,alias,dw_shards,exact', C_CASES)
def test_node_mix_bwd_next(C, L, b, same, drop, dg, dx, dy, n_prev, gz2, g_in, inplace, null_mid, pacc, alias, dw_shards,
                           exact):
    from bmnas import lib
    pool = Pool()
    m = _Mix(pool, 4, b, C, L, same=same, drop=drop, exact=exact, zero_col=0 if (C, b) == (20, 2) else None)
    M = m.M
    g = _gen(41 + C + b + n_prev)
    gin = _f32(g, b, C, L)
    old_x, old_y, prev_bg = _f32(g, b, C, L), _f32(g, b, C, L), _f32(g, 2 * M)
    dxd, dyd = _dest(pool, dx, old_x), _dest(pool, dy, old_y)
    acc = (1 if dx == 'acc' else 0) | (2 if dy == 'acc' else 0)
    dV, bn_grad = pool.new(b, M, L), pool.new(2 * M, base=prev_bg)
    prev_dg = dgd = None
    if dg is not None:
        prev_dg = 0.5 * _f32(g, dg[0], dg[1])
        dgd = pool.new(dg[0], dg[1], base=prev_dg)
    gd = _d(gin)
    nxt = rn = None
    if n_prev:
        ws = 1 + n_prev % 2
        prevs = [_f32(g, b, C, L) for _ in range(n_prev)]
        w = _f32(g, (n_prev + 1) * ws)
        s_in, gz = _f32(g, b, C, L), _f32(g, b, C, L)
        gz2t = _f32(g, b, C, L) if gz2 else None
        dest = [f'd{j}' for j in range(n_prev)]
        if null_mid and n_prev >= 3:
            dest[1] = None
        if alias:
            dest[1] = 'd0'                                   # (alias cases have no NULL in the middle)
        old = {k: _f32(g, b, C, L) for k in sorted(set(d_ for d_ in dest if d_ is not None))}
        first = {}
        for j, k in enumerate(dest):                         # a buffer starts as NaN unless its FIRST write accumulates
            if k is not None and k not in first:
                first[k] = pacc >> j & 1
        bufs = {k: pool.new(b, C, L, base=old[k] if first[k] else None) for k in old}
        dws = (n_prev + 1) * ws + 3
        prev_dw = 0.5 * _f32(g, dw_shards, dws)
        dwd = pool.new(dw_shards, dws, base=prev_dw)
        g_out = gd if (inplace and g_in) else pool.new(b, C, L)
        wd, sd, gzd, gz2d, pd = _d(w), _d(s_in), _d(gz), _d(gz2t), [_d(p) for p in prevs]
        nxt = (pd, [None if k is None else bufs[k] for k in dest], pacc, wd, ws, dwd, dw_shards, dws, sd, gzd, gz2d, g_out)
        rn = mr.next_bwd(prevs, w[::ws][:n_prev + 1], s_in, gz, gz2t, gin if g_in else None,
                         {k: (old[k] if first[k] else torch.zeros(b, C, L)) for k in old}, dest, pacc)
        g_mix = rn['g_out']
    else:
        g_mix = gin.double()
    lib.node_mix_bwd(gd if (g_in or not n_prev) else None, m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan,
                     m.dv['gamma'], dgd, dxd, dyd, acc, dV, bn_grad, b, C, L, m.dglu, m.dfc,
                     dg_shards=1 if dg is None else dg[0], dg_stride=0 if dg is None else dg[1], nxt=nxt)
    pool.check()
    r = m.bwd(g_mix, dx_old=None if dxd is None else old_x, dy_old=None if dyd is None else old_y, acc_mask=acc,
              prev_bn_grad=prev_bg)
    assert_close_scaled('dV', dV, r['dV'], rel=R_DV)
    assert_close_scaled('bn_grad: sum dV u_hat', bn_grad[:M], r['bn_grad'][:M], rel=R_GRAD)
    assert_close_scaled('bn_grad: sum dV', bn_grad[M:], r['bn_grad'][M:], rel=R_GRAD)
    _check_dxy(m, r, dxd, dyd, old_x, old_y)
    _check_dgamma('dgamma', dgd, prev_dg, r['dgamma'], r['dgamma_abs'], 4)
    if exact:
        assert float(dV[:, m.exact, :2].abs().max()) == 0.0, 'df at vf == 0 exactly'
        assert float(r['dV'][:, m.exact, :2].abs().max()) == 0.0
    if n_prev:
        assert_close_scaled('g_out', g_out, rn['g_out'], rel=R_DV)
        for k in bufs:
            assert_close_scaled('dprev ' + k, bufs[k], rn['dprev'][k], rel=R_DV)
        idx = [j * ws for j in range(n_prev + 1)]
        _dot_close('dw', dwd[:, idx].double().sum(0), rn['dw'], rn['dw_abs'], prev_dw[:, idx].double().sum(0))
        rest = [i for i in range(dws) if i not in idx]
        _same('dw between its strides', dwd[:, rest], prev_dw[:, rest])
        for name, t, ref in [('w', wd, w), ('s', sd, s_in), ('gz', gzd, gz)] + [(f'prev[{j}]', pd[j], prevs[j])
                                                                                 for j in range(n_prev)]:
            _same(name, t, ref)
    if not (n_prev and inplace and g_in):
        _same('g', gd, gin)
    m.check_inputs()
    m.check_fin()


# ------------------------------------------------------------------------------------------- D. bmnas_node_mix_ln_bwd
#          C, L, b, same, drop, g_in, dresid, dx, dy, dg          <VPT1, VPT2>: cl4 <= 512 <1,1>, <= 1024 <2,1>, else <4,2>
D_CASES = [(2, 4, 1, True, False, True, 'null', 'ow', 'null', (1, 4)),        # <1,1> cl4 2: each half one float4
           (6, 8, 3, False, True, False, 'ow', 'acc', 'ow', (3, 8)),          # <1,1> cl4 12
           (128, 16, 3, True, True, True, 'acc', 'acc', 'null', (3, 8)),      # <1,1> cl4 512, exact
           (130, 16, 1, False, False, True, 'ow', 'ow', 'acc', None),         # <2,1> cl4 520: its lower boundary
           (256, 16, 3, True, True, False, 'acc', 'ow', 'null', (1, 4)),      # <2,1> cl4 1024, exact
           (258, 16, 1, False, True, True, 'null', 'null', 'ow', (3, 8)),     # <4,2> cl4 1032
           (512, 16, 3, True, False, True, 'ow', 'acc', 'null', (1, 4)),      # <4,2> cl4 2048, the limit
           (16, 8, 128, True, True, True, 'acc', 'ow', 'null', (3, 8))]       # b 128, the limit


@pytest.mark.parametrize('C,L,b,same,drop,g_in,dresid,dx,dy,dg', D_CASES)
def test_node_mix_ln_bwd(C, L, b, same, drop, g_in, dresid, dx, dy, dg):
    from bmnas import lib
    assert lib.node_mix_ln_bwd_ok(b, C, L)
    pool = Pool()
    m = _Mix(pool, 5, b, C, L, same=same, drop=drop)
    M = m.M
    g = _gen(51 + C + b)
    gy, pre = _f32(g, b, C, L), (_randn(g, b, C, L) * 1.5 + 0.2).float()
    ln_w = (_randn(g, C, L) * 0.3 + 1.0).float()
    _, mean, rstd, _ = lr.node_ln(pre, ln_w, torch.zeros(C, L))
    stats = torch.stack([mean, rstd], 1).float().contiguous()
    old_r, old_x, old_y, prev_bg = _f32(g, b, C, L), _f32(g, b, C, L), _f32(g, b, C, L), _f32(g, 2 * M)
    gind = pool.new(b, C, L) if g_in else None
    drd, dxd, dyd = _dest(pool, dresid, old_r), _dest(pool, dx, old_x), _dest(pool, dy, old_y)
    acc = (1 if dx == 'acc' else 0) | (2 if dy == 'acc' else 0)
    dV, bn_grad = pool.new(b, M, L), pool.new(2 * M, base=prev_bg)
    prev_dg = dgd = None
    if dg is not None:
        prev_dg = 0.5 * _f32(g, dg[0], dg[1])
        dgd = pool.new(dg[0], dg[1], base=prev_dg)
    gyd, pred, wd, std = _d(gy), _d(pre), _d(ln_w), _d(stats)
    lib.node_mix_ln_bwd(gyd, pred, wd, std, gind, drd, dresid == 'acc', m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'],
                        m.chan, m.dv['gamma'], dgd, dxd, dyd, acc, dV, bn_grad, b, C, L, m.dglu, m.dfc,
                        dg_shards=1 if dg is None else dg[0], dg_stride=0 if dg is None else dg[1])
    pool.check()
    want_g, want_r = mr.mix_ln_bwd(gy, pre, ln_w, stats, None if drd is None else old_r, dresid == 'acc')
    r = m.bwd(want_g, dx_old=None if dxd is None else old_x, dy_old=None if dyd is None else old_y, acc_mask=acc,
              prev_bn_grad=prev_bg)
    if gind is not None:
        assert_close_scaled('g_in', gind, want_g, rel=R_DV)
    if drd is not None:
        assert_close_scaled('dresid', drd, want_r, rel=R_DV)
    assert_close_scaled('dV', dV, r['dV'], rel=R_DV)
    assert_close_scaled('bn_grad: sum dV u_hat', bn_grad[:M], r['bn_grad'][:M], rel=R_GRAD)
    assert_close_scaled('bn_grad: sum dV', bn_grad[M:], r['bn_grad'][M:], rel=R_GRAD)
    _check_dxy(m, r, dxd, dyd, old_x, old_y)
    _check_dgamma('dgamma', dgd, prev_dg, r['dgamma'], r['dgamma_abs'], 4)
    for name, t, ref in (('g', gyd, gy), ('pre', pred, pre), ('ln_w', wd, ln_w), ('stats', std, stats)):
        _same(name, t, ref)
    m.check_inputs()
    m.check_fin()


@pytest.mark.parametrize('b,C,L', [(129, 4, 4), (1, 514, 16)])
def test_node_mix_ln_bwd_refuses_what_it_cannot_take(b, C, L):
    """one BatchNorm atomic pair per channel per sample: b <= 128; <4,2,512> covers C L / 4 <= 2048.  Nothing is launched:
    every output still holds its NaN"""
    from bmnas import lib
    assert not lib.node_mix_ln_bwd_ok(b, C, L)
    pool = Pool()
    t = lambda *s: torch.zeros(*s, device=dev())
    outs = [pool.new(b, C, L), pool.new(b, 3 * C, L), pool.new(6 * C)]
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.node_mix_ln_bwd(t(b, C, L), t(b, C, L), t(C, L), t(b, 2), outs[0], None, False, t(b, C, L), t(b, C, L),
                            t(b, C, L), t(b, 3 * C, L), t(12 * C), t(4), None, None, None, 0, outs[1], outs[2], b, C, L,
                            lib.NO_DROP, lib.NO_DROP)
    pool.check()
    assert all(bool(torch.isnan(o).all()) for o in outs)


# ------------------------------------------------------------------------- E. bmnas_node_mix_sel_act_fwd / _bwd
def _perm_cols(mask, permuted):
    """the gamma column of every kind: list order (identity) or the present kinds reversed"""
    present = [k for k in range(4) if mask >> k & 1]
    order = present[::-1] if permuted else present
    cols = [-1] * 4
    for pos, k in enumerate(order):
        cols[k] = pos
    return cols, [KINDS[k] for k in order]


def _sel_case(mask, act, permuted, b, C, L, *, drop=True, fwd_mode='given', do_bwd=True, seed=6, dg=(3, 8), dx='ow',
              dy='acc', same=False):
    from bmnas import lib
    cols, prims = _perm_cols(mask, permuted)
    sel = lib.make_node_sel(prims)
    assert lib.node_sel_mask(sel) == mask and list(sel.col) == cols
    assert lib.node_mix_sel_ok(mask, b, C, L)
    fc_act = lib.FC_ACT_MISH if act == 'mish' else lib.FC_ACT_RELU
    n = len(prims)
    # ---- forward (its own problem where the finalisation runs in the kernel: the backward takes chan as given)
    pool = Pool()
    m = _Mix(pool, seed, b, C, L, mask=mask, act=act, cols=cols, same=same, drop=drop, mode=fwd_mode, shards=2,
             mish_span=(act == 'mish' and fwd_mode == 'given'), site=mask)
    out = pool.new(b, C, L)
    lib.node_mix_sel_fwd(m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan, m.dv['gamma'], sel, out, b, C, L, m.dglu,
                         m.dfc, m.fin, fc_act=fc_act)
    pool.check()
    assert_close_scaled('s', out, m.fwd(), rel=R_FWD)
    m.check_inputs()
    m.check_fin()
    if not do_bwd:
        return
    if fwd_mode != 'given':
        pool = Pool()
        m = _Mix(pool, seed + 1, b, C, L, mask=mask, act=act, cols=cols, same=same, drop=drop, mish_span=act == 'mish',
                 site=mask)
    M = m.M
    g = _gen(61 + mask + b)
    gin, old_x, old_y = _f32(g, b, C, L), _f32(g, b, C, L), _f32(g, b, C, L)
    prev_bg = _f32(g, max(2 * M, 1))[:2 * M]
    dxd, dyd = _dest(pool, dx, old_x), _dest(pool, dy, old_y)
    acc = (1 if dx == 'acc' else 0) | (2 if dy == 'acc' else 0)
    dV = pool.new(b, M, L) if M else None
    bn_grad = pool.new(2 * M, base=prev_bg) if M else None
    prev_dg = 0.5 * _f32(g, dg[0], dg[1])
    dgd = pool.new(dg[0], dg[1], base=prev_dg)
    gd = _d(gin)
    lib.node_mix_sel_bwd(gd, m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan, m.dv['gamma'], sel, dgd, dxd, dyd, acc,
                         dV, bn_grad, b, C, L, m.dglu, m.dfc, dg_shards=dg[0], dg_stride=dg[1], fc_act=fc_act)
    pool.check()
    r = m.bwd(gin, dx_old=None if dxd is None else old_x, dy_old=None if dyd is None else old_y, acc_mask=acc,
              prev_bn_grad=prev_bg if M else None)
    if M:
        assert_close_scaled('dV', dV, r['dV'], rel=R_DV)
        assert_close_scaled('bn_grad: sum dV u_hat', bn_grad[:M], r['bn_grad'][:M], rel=R_GRAD)
        assert_close_scaled('bn_grad: sum dV', bn_grad[M:], r['bn_grad'][M:], rel=R_GRAD)
    _check_dxy(m, r, dxd, dyd, old_x, old_y)
    _check_dgamma('dgamma', dgd, prev_dg, r['dgamma'], r['dgamma_abs'], n)
    _same('g', gd, gin)
    m.check_inputs()
    m.check_fin()


E_CASES = [(mk, 'relu') for mk in range(1, 16)] + [(mk, 'mish') for mk in range(8, 16)]


@pytest.mark.parametrize('permuted', [False, True])
@pytest.mark.parametrize('mask,act', E_CASES)
def test_node_mix_sel_every_instantiation(mask, act, permuted):
    """(b, C, L) = (5, 16, 8); identity columns with chan given, reversed columns with the finalisation in the forward
    kernel (M = C | 2 C | 3 C rows); dropout at every site the mask has; dx overwritten, dy accumulated — without Sum: dx
    zero-filled, dy bit-unchanged"""
    _sel_case(mask, act, permuted, 5, 16, 8, fwd_mode='train' if permuted else 'given')


@pytest.mark.parametrize('mask,act', [(15, 'relu'), (12, 'mish'), (6, 'relu')])
def test_node_mix_sel_without_dropout(mask, act):
    _sel_case(mask, act, True, 5, 16, 8, drop=False, fwd_mode='eval', dx='acc', dy='ow', dg=(1, 4))


def test_node_mix_sel_sum_alone_takes_any_c():
    """['Sum'] at C 3, L 4, b 2: no conv and no attention, C L / 4 = 3; x is y with dy NULL: 2 g0 g into dx"""
    _sel_case(1, 'relu', False, 2, 3, 4, drop=False, dg=(1, 1), dx='acc', dy='null', same=True)


def test_node_mix_sel_sum_alone_forward_at_l_12():
    _sel_case(1, 'relu', False, 3, 5, 12, drop=False, do_bwd=False)


@pytest.mark.parametrize('mask,act', [(12, 'relu'), (9, 'mish'), (12, 'mish'), (9, 'relu')])
@pytest.mark.parametrize('b,C,L', [(3, 16, 8), (5, 80, 4)])
def test_node_mix_sel_backward_edges(mask, act, b, C, L):
    """b 3: fewer samples than the four sample lanes; C 80, L 4: C L / 4 = 80, the second 64-slot block holds 16"""
    _sel_case(mask, act, True, b, C, L, dx='null' if mask == 12 else 'ow', dy='ow')


# ------------------------------------------------------------------------- F. bmnas_node_mix_conv_fwd (mix_conv_fwd_k)
#          n_src, C, L, b, ldw_pad, shards, mode, drop         kpw = ceil((n_src + 1) C / 16 / 4) -> <2|3|4|6|8|12>
F_CASES = [(1, 64, 4, 7, 0, 0, 'given', False),        # kpw 2; L 4, b 7: the last n-group holds 3 of 4 samples
           (2, 64, 8, 3, 4, 1, 'train', True),         # kpw 3; L 8, b 3: the last n-group holds 1 of 2
           (3, 64, 16, 2, 0, 3, 'eval', False),        # kpw 4
           (2, 128, 4, 7, 4, 3, 'train', True),        # kpw 6
           (3, 128, 8, 3, 0, 1, 'given', True),        # kpw 8
           (2, 192, 16, 2, 4, 3, 'train', False),      # 36 blocks, kpw 9: <12> with 12 block slots past the end of K
           (2, 256, 8, 3, 0, 0, 'given', True)]        # 48 blocks: fills <12>


@pytest.mark.parametrize('n_src,C,L,b,ldw_pad,shards,mode,drop', F_CASES)
def test_node_mix_conv_fwd(n_src, C, L, b, ldw_pad, shards, mode, drop):
    from bmnas import lib
    assert lib.node_mix_conv_fwd_ok(b, C, L, n_src)
    pool = Pool()
    m = _Mix(pool, 7, b, C, L, same=n_src % 2 == 1, drop=drop, mode=mode, shards=2)
    g = _gen(71 + C + n_src)
    K = (n_src + 1) * C
    ldw = K + ldw_pad
    srcs = [(_randn(g, b, C, L) + 0.25).float() for _ in range(n_src)]
    W, bias = (_randn(g, C, ldw) / float(K) ** 0.5).float(), (_randn(g, C) * 2.0 + 1.0).float()
    prev_stat = _f32(g, max(shards, 1), C, 2)[:shards]
    sd, Wd, bd = [_d(s_) for s_ in srcs], _d(W), _d(bias)
    mix_out, V = pool.new(b, C, L), pool.new(b, C, L)
    stat = pool.new(shards, C, 2, base=prev_stat) if shards else None
    lib.node_mix_conv_fwd(m.dv['x'], m.dv['y'], m.dv['p1'], m.dv['U'], m.chan, m.dv['gamma'], mix_out, m.dglu, m.dfc,
                          m.fin, sd, Wd, ldw, bd, V, stat, shards, b, C, L)
    pool.check()
    s = m.fwd()
    assert_close_scaled('mix_out', mix_out, s, rel=R_FWD)
    want_V, want_stat = mr.mix_conv(srcs, s, W, bias, shards)
    assert_close_scaled('V', V, want_V, rel=R_FWD)
    if shards:
        want_stat = want_stat + prev_stat.double()
        assert_close_scaled('stat: sum d', stat[:, :, 0], want_stat[:, :, 0], rel=R_GRAD)
        assert_close_scaled('stat: sum d^2', stat[:, :, 1], want_stat[:, :, 1], rel=R_M2)
    for q in range(n_src):
        _same(f'srcs[{q}]', sd[q], srcs[q])
    _same('W', Wd, W)
    _same('bias', bd, bias)
    m.check_inputs()
    m.check_fin()


def test_node_mix_conv_fwd_refuses_three_sources_at_c_256():
    """64 blocks of 16 channels: kpw 16 > 12.  Nothing is launched"""
    from bmnas import lib
    b, C, L = 2, 256, 8
    assert not lib.node_mix_conv_fwd_ok(b, C, L, 3)
    pool = Pool()
    t = lambda *s: torch.zeros(*s, device=dev())
    mix_out, V = pool.new(b, C, L), pool.new(b, C, L)
    with pytest.raises(lib.BmnasError, match=E_LIMIT):
        lib.node_mix_conv_fwd(t(b, C, L), t(b, C, L), t(b, C, L), t(b, 3 * C, L), t(12 * C), t(4), mix_out, lib.NO_DROP,
                              lib.NO_DROP, lib.NO_FIN, [t(b, C, L)] * 3, t(C, 4 * C), 4 * C, t(C), V, None, 0, b, C, L)
    pool.check()
    assert bool(torch.isnan(mix_out).all()) and bool(torch.isnan(V).all())


# ------------------------------------------------ G. the mix backward as the epilogue of bmnas_conv1x1_bwd_all_mix
_FORCED = [k for k in ('BMNAS_CONV_PIPE', 'BMNAS_FUSE_ATTN_GEMM', 'BMNAS_FUSE_BWD_PAIR') if os.environ.get(k) is not None]


@pytest.mark.parametrize('drop', [False, True])
@pytest.mark.parametrize('M,n_src,q,acc_dx,dg', [(16, 2, 0, 0, (1, 4)), (16, 2, 1, 1, (3, 8)), (80, 3, 0, 1, (3, 8)),
                                                 (80, 3, 2, 0, (1, 4)), (256, 2, 0, 0, (3, 8)), (256, 2, 1, 1, (1, 4))])
def test_mix_backward_in_the_conv_data_gradient_tiles(M, n_src, q, acc_dx, dg, drop):
    """shapes of group H of tests/test_conv_kernels_gpu.py (b 5, L 8; kpw 1, 2, 4) with C_src = the mix's C = M: source q's
    data gradient is the mix's g (x is y, dy absent: 2 g0 g into dx)"""
    from bmnas import lib
    b, L, C = 5, 8, M
    assert lib.conv1x1_bwd_all_mix_ok(b, L, M, n_src, C)
    pool = Pool()
    m = _Mix(pool, 8, b, C, L, same=True, drop=drop)
    K = n_src * C
    g = _gen(81 + M + q)
    dU = _f32(g, b, M, L)
    W = (_randn(g, M, K) / float(M) ** 0.5).float()
    srcs = [(_randn(g, b, C, L) + 0.25).float() for _ in range(n_src)]
    mask = 0b101 & ~(1 << q) & ((1 << n_src) - 1)               # the mix source is overwritten: it feeds nothing else
    prevs = [_f32(g, b, C, L) for _ in range(n_src)]
    pW, pb, old_x, prev_bg = _f32(g, M, K), _f32(g, M), _f32(g, b, C, L), _f32(g, 6 * C)
    prev_dg = 0.5 * _f32(g, dg[0], dg[1])
    dsts = [pool.new(b, C, L, base=p if (mask >> j) & 1 else None) for j, p in enumerate(prevs)]
    dW, db = pool.new(M, K, base=pW), pool.new(M, base=pb)
    dxd = pool.new(b, C, L, base=old_x if acc_dx else None)
    dV, bn_grad, dgd = pool.new(b, 3 * C, L), pool.new(6 * C, base=prev_bg), pool.new(dg[0], dg[1], base=prev_dg)
    dUd, Wd, sd = _d(dU), _d(W), [_d(s_) for s_ in srcs]
    lib.conv_family_calls(reset=True)
    lib.conv1x1_bwd_all(dUd, Wd, K, dsts, C, mask, b, L, M, 0, sd, dW, K, db, 0,
                        mix=(q, m.dv['U'], m.chan, m.dv['x'], m.dv['p1'], m.dv['gamma'], dgd, dg[0], dg[1], dxd, acc_dx, dV,
                             bn_grad, m.dglu, m.dfc))
    pool.check()
    got = {k for k, v in lib.conv_family_calls(reset=True).items() if v > 0}
    if not _FORCED:
        assert got == {'bwd_pair'}, got
    want_d = cr.conv_bwd_data(dU, W, 0, C, prevs, mask)
    want_W, want_b = cr.conv_bwd_weight(dU, srcs, pW, pb)
    for j in range(n_src):
        assert_close_scaled(f'dsrc{j}', dsts[j], want_d[j], rel=R_DV)
    assert_close_scaled('dW', dW, want_W, rel=R_GRAD)
    assert_close_scaled('dbias', db, want_b, rel=R_GRAD)
    r = m.bwd(want_d[q], dx_old=old_x, dy_old=None, acc_mask=acc_dx, prev_bn_grad=prev_bg)
    assert_close_scaled('dV', dV, r['dV'], rel=R_DV)
    assert_close_scaled('bn_grad: sum dV u_hat', bn_grad[:3 * C], r['bn_grad'][:3 * C], rel=R_GRAD)
    assert_close_scaled('bn_grad: sum dV', bn_grad[3 * C:], r['bn_grad'][3 * C:], rel=R_GRAD)
    assert_close_scaled('dx', dxd, r['dx'], rel=R_DV)
    _check_dgamma('dgamma', dgd, prev_dg, r['dgamma'], r['dgamma_abs'], 4)
    _same('dU', dUd, dU)
    _same('W', Wd, W)
    m.check_inputs()
    m.check_fin()
