// The arithmetic of one packed 16 x 16 attention tile, per lane — the ONE definition both attention families compile.
//
// Layout.  16 / L problems of L positions each (L in {4, 8, 16}) sit side by side on the 16-wide dimension of
// v_mfma_f32_16x16x4_f32; a block-diagonal mask (`same`) keeps them apart.  With lo = lane & 15, h = lane >> 4, a lane
// holds four elements of a tile matrix T: T[i = lo][j = 4 h + r], r = 0 .. 3 — a product over channels comes out of the
// MFMA like that (as T^T[j][i]), and a product over positions takes it like that as its A operand.  The transposed
// view T[i = 4 h + r][j = lo] goes through a 16 x 17 LDS image, which the callers keep written out (see below).
//
// Association order of every sum — callers rely on it bit for bit:
//   contract_channels  k-steps t0 .. t1 - 1 of 4 channels each; groups of four alternate two accumulators (acc0, acc1,
//                      acc0, acc1), a tail of single steps goes to acc0, the result is acc0[r] + acc1[r]; inside an
//                      accumulator the steps add in ascending t, inside a step the MFMA's own order
//   tile_softmax       max and sum: the lane's four registers in ascending r, then the xor-16 partner, then the xor-32
//                      partner; p = exp(sc - max) * (1 / den)
//   tile_softmax_bwd   rowdot: dP[r] p[r] in ascending r, then xor 16, then xor 32; ds = (p (dP - rowdot)) inv
//   tile_apply         the four MFMAs r = 0 .. 3 chained on one accumulator
//
// Callers: attn_probs (scores, each wave its quarter of C, which it then adds across waves through LDS), sdpa_fwd_body
// and sdpa_bwd_body in sdpa_body.hpp — compiled by sdpa.hip as sdpa_ln_fwd_k / sdpa_ln_bwd_k and by conv1x1.hip inside
// its four merged conv + attention kernels; mha_core_fwd_k / mha_core_bwd_k in mha.hip (one wave owns a tile and
// contracts all d channels of its head).
#pragma once
#include "common.hpp"

namespace {

// out[r] = T^T[j = 4h + r][i = lo] = sum_c A[c][j] B[c][i]: A supplies the rows j, B the columns i.  ab / bb point at
// (problem of row lo, channel 0, position of row lo); k-step t reads channel 4 t + h, at (4 t + h) * L.  A caller whose
// t0 is not wave-uniform to the compiler (threadIdx.x >> 6) passes t1 as t0 + n: the trip count then is, and the
// loop guards stay scalar (per-lane guards cost the sdpa kernels 4 AGPRs and up to a wave of occupancy).
__device__ __forceinline__ void contract_channels(const float* __restrict__ ab, const float* __restrict__ bb, int t0,
                                                  int t1, int L, int h, float out[4]) {
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  const int64_t st = (int64_t)4 * L;
  int t = t0;
  for (; t + 3 < t1; t += 4) {                    // 8 loads in flight, then 4 MFMAs
    const int64_t o0 = (int64_t)(4 * t + h) * L;
    const float a0 = ab[o0], b0 = bb[o0];
    const float a1 = ab[o0 + st], b1 = bb[o0 + st];
    const float a2 = ab[o0 + 2 * st], b2 = bb[o0 + 2 * st];
    const float a3 = ab[o0 + 3 * st], b3 = bb[o0 + 3 * st];
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, b0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, b1, acc1, 0, 0, 0);
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, b2, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, b3, acc1, 0, 0, 0);
  }
  for (; t < t1; ++t) {
    const int64_t o0 = (int64_t)(4 * t + h) * L;
    acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(ab[o0], bb[o0], acc0, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) out[r] = acc0[r] + acc1[r];
}

// p[r] = softmax_j(raw * inv)[i = lo][j = 4h + r] over the j of row i's own problem (`same`: rows lo and 4h .. 4h + 3
// belong to one problem); 0 elsewhere.  A row's 16 columns are the four registers of the four lanes lo + 16 h.
__device__ __forceinline__ void tile_softmax(const float raw[4], float inv, bool same, float p[4]) {
  float sc[4], mx = -INFINITY;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    sc[r] = same ? raw[r] * inv : -INFINITY;
    mx = fmaxf(mx, sc[r]);
  }
  mx = xor16_max(mx);
  mx = xor32_max(mx);
  float den = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    p[r] = same ? __expf(sc[r] - mx) : 0.f;
    den += p[r];
  }
  den = xor16_sum(den);
  den = xor32_sum(den);
  const float rden = 1.f / den;
#pragma unroll
  for (int r = 0; r < 4; ++r) p[r] *= rden;
}

// ds = dS * inv for S = raw * inv, P = softmax(S): what the gradients of the two score operands contract with.  dP is
// the gradient of the probabilities the product over positions used (a caller with dropout on P scales it first).
__device__ __forceinline__ void tile_softmax_bwd(const float p[4], const float dP[4], float inv, float ds[4]) {
  float rowdot = 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) rowdot += dP[r] * p[r];
  rowdot = xor16_sum(rowdot);
  rowdot = xor32_sum(rowdot);
#pragma unroll
  for (int r = 0; r < 4; ++r) ds[r] = p[r] * (dP[r] - rowdot) * inv;
}

// acc[c][i] += sum_r a[r] v[c][j = 4h + r] — the product over positions for 16 channels (lane lo = channel c, v = four
// consecutive positions of it), a = T[i = lo][j = 4h + r]; with the transposed view of T it sums over i instead.
__device__ __forceinline__ f32x4 tile_apply(const float a[4], float4 v, f32x4 acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], v.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], v.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], v.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], v.w, acc, 0, 0, 0);
  return acc;
}

}  // namespace
