// The NodeMixedOp mix, per element — the ONE definition every mix kernel compiles:
//
//   s = g0 (x + y) + g1 p1 + g2 drop(va sigmoid(vg)) + g3 drop(act(vf))       va | vg | vf = BatchNorm(U rows)
//
// act = relu: ConcatFC.  act = mish (ACT = kActMish; nodemix_sel.hip alone instantiates it): CatConvMish, which takes
// ConcatFC's slot — mask bit 3, the C rows behind the GLU rows, gamma column 3, the drop_fc site.
//
// and its backward: dgamma, the gamma-weighted gradients da | dg | df of the BatchNorm outputs, their per-channel
// BatchNorm sums sw = sum d xhat, sb = sum d, and the dx / dy write.  Both directions are specialised on the presence
// mask of nodemix_sel.hip (bit 0 Sum, 1 ScaleDotAttn, 2 LinearGLU, 3 ConcatFC); the default list is mask 15.  An
// absent term's operands are never read here, so whatever the caller passes for them compiles to nothing.
//
// Callers: node_mix_fwd_k, node_mix_ln_fwd_k, node_mix_bwd_k, node_mix_ln_bwd_k, bn_glu_fwd_k / bn_glu_bwd_k (the GLU
// term alone) in bnmix.hip; node_mix_pre_fwd_k, node_mix_lnp_bwd_k in lazyln.hip; mix_conv_fwd_k in mixconv.hip;
// mix_ep_tile in conv1x1.hip; node_mix_sel_fwd_k / node_mix_sel_bwd_k in nodemix_sel.hip.
#pragma once
#include "common.hpp"
#include "mish.hpp"

namespace {

enum { kSum = 1, kAttn = 2, kGlu = 4, kFc = 8, kMixAll = 15 };

__device__ __forceinline__ float4 affine4(float4 u, float sc, float sh) {
  return make_float4(fmaf(u.x, sc, sh), fmaf(u.y, sc, sh), fmaf(u.z, sc, sh), fmaf(u.w, sc, sh));
}
__device__ __forceinline__ float sigmoidf(float v) { return 1.f / (1.f + __expf(-v)); }

// LinearGLU: drop(va sigmoid(vg)), and its gradients for an incoming gm = (weight) g m
__device__ __forceinline__ float glu_term(float va, float sg, float m) { return va * sg * m; }
__device__ __forceinline__ void glu_grad(float gm, float va, float sg, float& da, float& dg) {
  da = gm * sg;
  dg = gm * va * sg * (1.f - sg);
}
// ConcatFC: drop(relu(vf)); CatConvMish (reference node_operations.py:58-82), in the same slot: drop(mish(vf))
template <int ACT = kActRelu>
__device__ __forceinline__ float fc_term(float vf, float m) {
  if constexpr (ACT == kActMish) return act_f(vf, 1) * m;
  else return fmaxf(vf, 0.f) * m;
}

// ---- forward.  Association order of the present terms: ((g0 s + g1 p) + g2 t2) + g3 t3  (s = x + y)
template <int MASK, int ACT = kActRelu>
__device__ __forceinline__ float mix_fwd(float g0, float g1, float g2, float g3, float s, float p, float va, float vg,
                                         float vf, float m2, float m3) {
  float o = 0.f;
  if constexpr (MASK & kSum) o = g0 * s;
  if constexpr (MASK & kAttn) o = (MASK & kSum) ? o + g1 * p : g1 * p;
  if constexpr (MASK & kGlu)
    o = (MASK & (kSum | kAttn)) ? o + g2 * glu_term(va, sigmoidf(vg), m2) : g2 * glu_term(va, sigmoidf(vg), m2);
  if constexpr (MASK & kFc)
    o = (MASK & (kSum | kAttn | kGlu)) ? o + g3 * fc_term<ACT>(vf, m3) : g3 * fc_term<ACT>(vf, m3);
  return o;
}
template <int MASK, int ACT = kActRelu>
__device__ __forceinline__ float4 mix_fwd4(float g0, float g1, float g2, float g3, float4 s, float4 p, float4 va,
                                           float4 vg, float4 vf, float4 m2, float4 m3) {
  return make_float4(mix_fwd<MASK, ACT>(g0, g1, g2, g3, s.x, p.x, va.x, vg.x, vf.x, m2.x, m3.x),
                     mix_fwd<MASK, ACT>(g0, g1, g2, g3, s.y, p.y, va.y, vg.y, vf.y, m2.y, m3.y),
                     mix_fwd<MASK, ACT>(g0, g1, g2, g3, s.z, p.z, va.z, vg.z, vf.z, m2.z, m3.z),
                     mix_fwd<MASK, ACT>(g0, g1, g2, g3, s.w, p.w, va.w, vg.w, vf.w, m2.w, m3.w));
}

// ---- backward.  The BatchNorm constants of one channel's NB conv blocks (chan = mean | rstd | scale | shift, M each)
template <int NB>
struct ChanBn {
  float mu[NB], rs[NB], sc[NB], sh[NB];
};
template <int NB>
__device__ __forceinline__ ChanBn<NB> chan_load(const float* chan, int M, int C, int c) {
  ChanBn<NB> b;
#pragma unroll
  for (int k = 0; k < NB; ++k) {
    b.mu[k] = chan[k * C + c];
    b.rs[k] = chan[M + k * C + c];
    b.sc[k] = chan[2 * M + k * C + c];
    b.sh[k] = chan[3 * M + k * C + c];
  }
  return b;
}

// conv blocks of U under a mask: LinearGLU's a | gate first, then ConcatFC's
template <int MASK>
struct MixRows {
  static constexpr int kFo = (MASK & kGlu) ? 2 : 0;                  // ConcatFC's block
  static constexpr int kMc = kFo + ((MASK & kFc) ? 1 : 0);           // blocks present
  static constexpr int kNb = kMc > 0 ? kMc : 1;                      // array extent (nothing of it is touched at 0)
};

// One float4 of the mix backward: gv = gradient of the mix output, xy = x + y, ua | ug | uf = RAW conv outputs.
// dgam[q], sw[k], sb[k] accumulate; da | dg | df are the gradients of the present blocks' BatchNorm outputs.
template <int MASK, int ACT = kActRelu>
__device__ __forceinline__ void mix_bwd4(float g2, float g3, float4 gv, float4 xy, float4 pv, float4 ua, float4 ug,
                                         float4 uf, float4 m2, float4 m3, const ChanBn<MixRows<MASK>::kNb>& bn,
                                         float (&dgam)[4], float4& da4, float4& dg4, float4& df4,
                                         float (&sw)[MixRows<MASK>::kNb], float (&sb)[MixRows<MASK>::kNb]) {
  constexpr int FO = MixRows<MASK>::kFo;
  const float gq[4] = {gv.x, gv.y, gv.z, gv.w};
  const float xq[4] = {xy.x, xy.y, xy.z, xy.w}, pq[4] = {pv.x, pv.y, pv.z, pv.w};
  const float uaq[4] = {ua.x, ua.y, ua.z, ua.w}, ugq[4] = {ug.x, ug.y, ug.z, ug.w}, ufq[4] = {uf.x, uf.y, uf.z, uf.w};
  const float m2q[4] = {m2.x, m2.y, m2.z, m2.w}, m3q[4] = {m3.x, m3.y, m3.z, m3.w};
  float da[4] = {0.f, 0.f, 0.f, 0.f}, dg[4] = {0.f, 0.f, 0.f, 0.f}, df[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if constexpr (MASK & kSum) dgam[0] += gq[t] * xq[t];
    if constexpr (MASK & kAttn) dgam[1] += gq[t] * pq[t];
    if constexpr (MASK & kGlu) {
      const float va = fmaf(uaq[t], bn.sc[0], bn.sh[0]), vg = fmaf(ugq[t], bn.sc[1], bn.sh[1]);
      const float sg = sigmoidf(vg);
      dgam[2] += gq[t] * glu_term(va, sg, m2q[t]);
      glu_grad(g2 * gq[t] * m2q[t], va, sg, da[t], dg[t]);
      sw[0] += da[t] * (uaq[t] - bn.mu[0]) * bn.rs[0];
      sw[1] += dg[t] * (ugq[t] - bn.mu[1]) * bn.rs[1];
      sb[0] += da[t]; sb[1] += dg[t];
    }
    if constexpr (MASK & kFc) {
      const float vf = fmaf(ufq[t], bn.sc[FO], bn.sh[FO]);
      if constexpr (ACT == kActMish) {
        dgam[3] += gq[t] * fc_term<ACT>(vf, m3q[t]);
        df[t] = g3 * gq[t] * m3q[t] * dact_f(vf, 1);
      } else {
        dgam[3] += gq[t] * fc_term(vf, m3q[t]);
        df[t] = (vf > 0.f) ? g3 * gq[t] * m3q[t] : 0.f;
      }
      sw[FO] += df[t] * (ufq[t] - bn.mu[FO]) * bn.rs[FO];
      sb[FO] += df[t];
    }
  }
  da4 = make_float4(da[0], da[1], da[2], da[3]);
  dg4 = make_float4(dg[0], dg[1], dg[2], dg[3]);
  df4 = make_float4(df[0], df[1], df[2], df[3]);
}

// The Sum term's input gradients: dx (=|+=) g0 g, dy likewise; x is y (dy == NULL) sends both halves to dx.
// `st` is the caller's 16-byte store.  Two forms: the destinations' old values arrive with the caller's first loads
// (zero where the accumulate bit is clear) ...
template <typename St>
__device__ __forceinline__ void mix_dxy_store(St st, float* dx, float* dy, int64_t e, float4 gv, float g0, float4 oldx,
                                              float4 oldy) {
  const float4 d0 = f4_scale(gv, g0);
  if (dx != nullptr) st(dx + e, f4_add((dy == nullptr) ? f4_scale(d0, 2.f) : d0, oldx));
  if (dy != nullptr) st(dy + e, f4_add(d0, oldy));
}
// ... or are fetched here, under the bit (the kernels that walk a chunk of samples)
template <typename St>
__device__ __forceinline__ void mix_dxy_store(St st, float* dx, float* dy, int64_t e, float4 gv, float g0,
                                              uint32_t acc_mask) {
  const float4 d0 = f4_scale(gv, g0);
  if (dx != nullptr) {
    float4 v = (dy == nullptr) ? f4_scale(d0, 2.f) : d0;
    if (acc_mask & 1u) v = f4_add(v, ld4(dx + e));
    st(dx + e, v);
  }
  if (dy != nullptr) {
    float4 v = d0;
    if (acc_mask & 2u) v = f4_add(v, ld4(dy + e));
    st(dy + e, v);
  }
}

}  // namespace
