// The unrolled (second-order) architecture step of DARTS (Liu et al. 2019, eq. 7-8) — what the reference's
// `architect.step(..., unrolled=args.unrolled)` (models/search/darts/train_search.py:151, flag at :42 and at
// main_darts_found_ntu.py:48) asks of an Architect whose unrolled body was stripped (models/search/darts/architect.py:9-29
// keeps only `network_weight_decay`) — as four launches over the descriptor table, the (tensor, chunk) list and the 8-float
// rows of adam.hip.  A descriptor's columns mean here:
//   param = w,  grad = the vector of the pass (the train gradient g, then v = dL_val/dw'),  exp_avg = the weight optimizer's
//   momentum_buffer (NULL allowed),  exp_avg_sq = a backup tensor of w's size
// so bmnas_grad_sqnorm_multi serves ||v|| unchanged.  Arithmetic = DARTS' own statements, operation by operation, every
// operation rounded on its own (no fused multiply-add):
//   virtual step   bak = p;  d = g (+ wd * p if wd != 0);  d = buf * mu + d (momentum);  p = p + neg_eta * d
//                  (theta.sub(eta, moment + dtheta), dtheta = grad + wd * theta, moment = momentum_buffer * momentum)
//   perturb        R = r / ||v||;  p = bak + (sign * R) * v        (w+ and w- both from the backup, never w+ - 2R v)
//   restore        p = bak
//   combine        ig = (gp - gn) / (2 * R);  da = da - eta * ig   ((x - y).div_(2R), g.sub_(eta, ig))
// HBM-streaming: virtual step 2 reads + 2 writes = 16 B/param (20 B with momentum), perturb 12 B, restore 8 B.
#include "multi_tensor.hpp"
#include "../../include/bmnas_hip.h"

namespace {

struct VirtHyp {
  float neg_eta, mu, wd;
};

// No contraction anywhere: a term switched off by its scalar (wd == 0 is a branch; mu == 0 gives buf * 0 + d = d) must
// leave the bits of the sequence without it, and the sequence itself is a numpy fp32 one.
template <bool MOMENTUM>
__device__ __forceinline__ float virt1(float p, float g, float buf, bool mom, const VirtHyp& h) {
#pragma clang fp contract(off)
  float d = g;
  if (h.wd != 0.f) d = g + h.wd * p;
  if constexpr (MOMENTUM) {
    if (mom) d = buf * h.mu + d;
  }
  return p + h.neg_eta * d;
}

// bak = p; p = the virtual step.  `buf` (exp_avg) is read and never written; without MOMENTUM it is not dereferenced, and
// with it a tensor whose exp_avg is NULL (no momentum_buffer yet, beside tensors that have one) takes no momentum term —
// one branch per workgroup.
template <bool MOMENTUM>
__global__ __launch_bounds__(256) void unroll_virtual_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                        const int32_t* __restrict__ chunks,
                                                        const float* __restrict__ hyp) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  const float* hr = hyp + 8 * t.hyp_row;
  VirtHyp h;
  h.neg_eta = hr[0]; h.mu = hr[1]; h.wd = hr[2];
  float* __restrict__ bak = t.exp_avg_sq;
  uintptr_t al = (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)bak;
  bool mom = false;
  if constexpr (MOMENTUM) {
    mom = t.exp_avg != nullptr;
    al |= (uintptr_t)t.exp_avg;
  }
  walk_chunk(t.numel, ci, al, [&](int64_t e) {
    const float4 p = ld4(t.param + e);
    const float4 g = ld4(t.grad + e);
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (MOMENTUM) {
      if (mom) b = ld4(t.exp_avg + e);
    }
    float4 q;
    q.x = virt1<MOMENTUM>(p.x, g.x, b.x, mom, h);
    q.y = virt1<MOMENTUM>(p.y, g.y, b.y, mom, h);
    q.z = virt1<MOMENTUM>(p.z, g.z, b.z, mom, h);
    q.w = virt1<MOMENTUM>(p.w, g.w, b.w, mom, h);
    st4_wtg<5>(bak + e, p);
    st4_wtg<5>(t.param + e, q);
  }, [&](int64_t i) {
    const float p = t.param[i], g = t.grad[i];
    float b = 0.f;
    if constexpr (MOMENTUM) {
      if (mom) b = t.exp_avg[i];
    }
    bak[i] = p;
    t.param[i] = virt1<MOMENTUM>(p, g, b, mom, h);
  });
}

// The norm is the one adam.hip's clip_coef takes (norm_from_partials).  R = r / norm, no epsilon: a zero ||v|| gives
// inf, and inf * 0 = NaN in the parameters, as DARTS' `R = r / _concat(vector).norm()` does.
__global__ __launch_bounds__(256) void unroll_perturb_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                        const int32_t* __restrict__ chunks,
                                                        const float* __restrict__ partials, int n_parts,
                                                        const float* __restrict__ r, float sign,
                                                        float* __restrict__ R_out) {
  __shared__ float red[4];
  const float R = r[0] / norm_from_partials(partials, n_parts, red);
  if (blockIdx.x == 0 && threadIdx.x == 0) R_out[0] = R;
  const float s = mul_alone(sign, R);
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  const float* __restrict__ bak = t.exp_avg_sq;
  walk_chunk(t.numel, ci, (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)bak, [&](int64_t e) {
    const float4 b = ld4(bak + e);
    const float4 v = ld4(t.grad + e);
    float4 q;
    q.x = b.x + mul_alone(s, v.x);
    q.y = b.y + mul_alone(s, v.y);
    q.z = b.z + mul_alone(s, v.z);
    q.w = b.w + mul_alone(s, v.w);
    st4_wtg<5>(t.param + e, q);
  }, [&](int64_t i) { t.param[i] = bak[i] + mul_alone(s, t.grad[i]); });
}

// p = bak.  `grad` is not read: a NaN in v cannot leak into w.
__global__ __launch_bounds__(256) void unroll_restore_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                        const int32_t* __restrict__ chunks) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  const float* __restrict__ bak = t.exp_avg_sq;
  walk_chunk(t.numel, ci, (uintptr_t)t.param | (uintptr_t)bak,
             [&](int64_t e) { st4_wtg<5>(t.param + e, ld4(bak + e)); }, [&](int64_t i) { t.param[i] = bak[i]; });
}

__device__ __forceinline__ float comb1(float da, float gp, float gn, float two_R, float eta) {
#pragma clang fp contract(off)
  const float d = gp - gn;
  const float ig = d / two_R;
  return da - eta * ig;
}

// Over an alpha table: param = d(alpha) (read and written), grad = g+, exp_avg = g-.
__global__ __launch_bounds__(256) void unroll_combine_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                        const int32_t* __restrict__ chunks,
                                                        const float* __restrict__ hyp, const float* __restrict__ R) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  const float eta = hyp[0];
  const float two_R = mul_alone(2.f, R[0]);
  const float* __restrict__ gn = t.exp_avg;
  walk_chunk(t.numel, ci, (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)gn, [&](int64_t e) {
    const float4 a = ld4(t.param + e), p = ld4(t.grad + e), n = ld4(gn + e);
    float4 q;
    q.x = comb1(a.x, p.x, n.x, two_R, eta);
    q.y = comb1(a.y, p.y, n.y, two_R, eta);
    q.z = comb1(a.z, p.z, n.z, two_R, eta);
    q.w = comb1(a.w, p.w, n.w, two_R, eta);
    st4_wtg<5>(t.param + e, q);
  }, [&](int64_t i) { t.param[i] = comb1(t.param[i], t.grad[i], gn[i], two_R, eta); });
}

}  // namespace

extern "C" int bmnas_unroll_virtual_step(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                         const float* hyp, int flags, void* stream) {
  if (flags & ~BMNAS_UNROLL_MOMENTUM) return BMNAS_E_ARG;
  if (!tensors || !chunks || !hyp || n_chunks < 0) return BMNAS_E_ARG;
  if (n_chunks == 0) return 0;
  if (flags & BMNAS_UNROLL_MOMENTUM)
    hipLaunchKernelGGL(unroll_virtual_k<true>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, hyp);
  else
    hipLaunchKernelGGL(unroll_virtual_k<false>, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, hyp);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_unroll_perturb(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                    const float* partials, int n_parts, const float* r, float sign, float* R_out,
                                    void* stream) {
  if (!tensors || !chunks || !partials || !r || !R_out || n_chunks <= 0) return BMNAS_E_ARG;   // (a norm is needed)
  if (!(sign == 1.f || sign == -1.f)) return BMNAS_E_ARG;
  if (n_parts != norm_parts(n_chunks)) return BMNAS_E_ARG;           // what the norm launch wrote
  hipLaunchKernelGGL(unroll_perturb_k, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, partials,
                     n_parts, r, sign, R_out);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_unroll_restore(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                    void* stream) {
  if (!tensors || !chunks || n_chunks < 0) return BMNAS_E_ARG;
  if (n_chunks == 0) return 0;
  hipLaunchKernelGGL(unroll_restore_k, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_unroll_combine(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                    const float* hyp, const float* R, void* stream) {
  if (!tensors || !chunks || !hyp || !R || n_chunks < 0) return BMNAS_E_ARG;
  if (n_chunks == 0) return 0;
  hipLaunchKernelGGL(unroll_combine_k, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, hyp, R);
  BMNAS_CHECK_LAUNCH();
  return 0;
}
