// LayerNorm over a whole sample (C, L) — the ONE definition of its per-element arithmetic and of its epsilon:
//
//   mean = S(v) / D,  var = S((v - mean)^2) / D,  rstd = 1 / sqrt(var + kLnEps),  o = (v - mean) rstd w + b
//   backward, with xhat = (x - mean) rstd and dxh = gy w:   m1 = S(dxh) / D,  m2 = S(dxh xhat) / D,
//   dx = rstd (dxh - m1 - xhat m2)
//
// What differs between the kernels — loads and their clamped addressing, the mix / BatchNorm / ReLU / dropout that
// fills the sample, stores — stays in the kernels.  Callers: cat_ln_fwd_k / cat_ln_bwd_k (layernorm.hip),
// node_mix_ln_fwd_k / node_mix_ln_bwd_k, bn_relu_ln_fwd_k / bn_relu_ln_bwd_k (bnmix.hip), mixsum_pair_fwd_lazy_k /
// node_mix_lnp_bwd_k (lazyln.hip), sdpa_fwd_body / sdpa_bwd_body (sdpa_body.hpp), head_fwd_k / head_bwd_k (head.hip);
// lazy_combine (lazy_ln.hpp) takes the epsilon.
// NOT here: the forward's second pass (six accumulators, their reduction, the output-sum identities), which the three
// per-sample forward kernels keep written out.  hipcc simplifies a __forceinline__ function on its own BEFORE it
// inlines it, and that block comes out with other packed / fused forms through a call, whether it takes the register
// arrays or one float4 at a time: other bits in the one-float4-per-thread kernels' output sums, more scratch in
// cat_ln_fwd_k<16, 512> (profiles/r23_ln_sample.txt).
#pragma once
#include "common.hpp"

namespace {

constexpr float kLnEps = 1e-5f;      // nn.LayerNorm's default, every LayerNorm of the network

__device__ __forceinline__ float ln_xhat(float x, float mean, float rstd) { return (x - mean) * rstd; }
__device__ __forceinline__ float4 ln_xhat4(float4 x, float mean, float rstd) {
  return make_float4(ln_xhat(x.x, mean, rstd), ln_xhat(x.y, mean, rstd), ln_xhat(x.z, mean, rstd),
                     ln_xhat(x.w, mean, rstd));
}
__device__ __forceinline__ float ln_apply(float v, float mean, float rstd, float w, float b) {
  return (v - mean) * rstd * w + b;
}
__device__ __forceinline__ float4 ln_apply4(float4 v, float mean, float rstd, float4 w, float4 b) {
  return make_float4(ln_apply(v.x, mean, rstd, w.x, b.x), ln_apply(v.y, mean, rstd, w.y, b.y),
                     ln_apply(v.z, mean, rstd, w.z, b.z), ln_apply(v.w, mean, rstd, w.w, b.w));
}
__device__ __forceinline__ float ln_dx(float dxh, float xh, float m1, float m2, float rstd) {
  return rstd * (dxh - m1 - xh * m2);
}
__device__ __forceinline__ float4 ln_dx4(float4 dxh, float4 xh, float m1, float m2, float rstd) {
  return make_float4(ln_dx(dxh.x, xh.x, m1, m2, rstd), ln_dx(dxh.y, xh.y, m1, m2, rstd),
                     ln_dx(dxh.z, xh.z, m1, m2, rstd), ln_dx(dxh.w, xh.w, m1, m2, rstd));
}

// The backward's two sums behind ONE barrier, which is the caller's (bn_relu_ln_bwd_k puts more partials in front of
// it): ln_bwd_sums_put, __syncthreads(), ln_bwd_sums_get.  `red` holds 2 NW floats and is written once per launch.
template <int NW>
__device__ __forceinline__ void ln_bwd_sums_put(float s1, float s2, float* red) {
  s1 = wave_sum(s1);
  s2 = wave_sum(s2);
  if ((threadIdx.x & 63) == 0) {
    red[threadIdx.x >> 6] = s1;
    red[NW + (threadIdx.x >> 6)] = s2;
  }
}
template <int NW>
__device__ __forceinline__ void ln_bwd_sums_get(const float* red, const float inv_d, float& m1, float& m2) {
  m1 = red[0];
  m2 = red[NW];
#pragma unroll
  for (int w = 1; w < NW; ++w) {
    m1 += red[w];
    m2 += red[NW + w];
  }
  m1 *= inv_d;
  m2 *= inv_d;
}

}  // namespace
