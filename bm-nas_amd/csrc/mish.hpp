// Mish and its derivative, per element — the ONE definition of every kernel that applies it: the FC_Mish edges of
// fcedge.hip (reference models/search/darts/operations.py:48-65) and the CatConvMish step primitive (reference
// models/search/darts/node_operations.py:58-82) in bnmix.hip (bn_mish_fwd_k / bn_mish_bwd_k) and, through
// mix_terms.hpp, nodemix_sel.hip.
#pragma once
#include "common.hpp"

namespace {

// mish(u) = u tanh(softplus(u)); with n = e^u: tanh(log(1 + n)) = q / (q + 2), q = n (n + 2) — no cancellation for
// u -> -inf.  torch's softplus returns u itself above 20, where tanh is 1 in fp32.
__device__ __forceinline__ float mish_t(float u, float& q) {
  const float n = expf(fminf(u, 20.f));
  q = n * (n + 2.f);
  return u > 20.f ? 1.f : q / (q + 2.f);
}
__device__ __forceinline__ float act_f(float u, int mish) {
  if (!mish) return fmaxf(u, 0.f);
  float q;
  return u * mish_t(u, q);
}
// act'(u): [u > 0] | tanh(sp) + u sigmoid(u) (1 - tanh(sp)^2), 1 - t^2 = 4 (q + 1) / (q + 2)^2
__device__ __forceinline__ float dact_f(float u, int mish) {
  if (!mish) return u > 0.f ? 1.f : 0.f;
  if (u > 20.f) return 1.f;
  float q;
  const float t = mish_t(u, q);
  const float n = expf(u);
  const float sg = n / (1.f + n);
  const float r = 1.f / (q + 2.f);
  return t + u * sg * 4.f * (q + 1.f) * r * r;
}
__device__ __forceinline__ float4 act4(float4 u, int mish) {
  return make_float4(act_f(u.x, mish), act_f(u.y, mish), act_f(u.z, mish), act_f(u.w, mish));
}
__device__ __forceinline__ float4 dact4(float4 u, int mish) {
  return make_float4(dact_f(u.x, mish), dact_f(u.y, mish), dact_f(u.z, mish), dact_f(u.w, mish));
}

// The activation of a conv + BatchNorm tail as a compile-time choice (the FC slot of the NodeMixedOp mix, the
// standalone BatchNorm tails of bnmix.hip)
enum { kActRelu = 0, kActMish = 1 };

}  // namespace
