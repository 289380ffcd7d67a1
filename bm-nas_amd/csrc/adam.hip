// Multi-tensor Adam: the w- and alpha-updates of the search loop
// (torch.optim.Adam built at mmimdb_darts_searchable.py:28-33, stepped at
// train_searchable/mmimdb.py:101 and architect.py:24) as ONE launch over every tensor of
// the optimizer instead of ~10 foreach launches x param groups.
//
// Arithmetic = torch.optim.Adam / torch.optim.AdamW (torch 2.10's _single_tensor_adam; maximize off),
// operation by operation:
//   p   = p * f                                      (decoupled weight decay: f = float(1 - lr * wd))
//   g   = grad + wd * p                              (L2 weight decay, only if wd != 0)
//   m   = lerp(m, g, 1 - beta1)
//   v   = v * beta2 + (1 - beta2) * g * g
//   vm  = maximum(vm, v)                             (amsgrad; NaN-propagating, as torch.maximum)
//   p  += -(lr / bc1) * ( m / ( sqrt(amsgrad ? vm : v) / sqrt(bc2) + eps ) )
// adam_multi_k / adam_multi_clip_k are the kernels with both switches off (L2, no running maximum);
// adam_multi_ex_k<CLIP, DECOUPLED, AMSGRAD> holds every other combination (bmnas_adam_multi_ex).
// The step-dependent scalars (-(lr/bc1), sqrt(bc2), f) are computed by the host in double, as
// torch does, and handed over in a small device table (`hyp`, 8 floats per row) that the host
// refreshes before every launch: a captured hipGraph replays with new learning rates / step
// counts without re-capture.
// HBM-streaming: 4 reads + 3 writes per element = 28 B/param; amsgrad: 5 reads + 4 writes = 36 B/param.
//
// Multi-tensor SGD with momentum (bmnas_sgd_multi; the weight optimizer of the DARTS drivers, reference
// models/search/darts/train_search.py:84-88 and train.py:78, clipped at train_search.py:158) walks the same descriptor
// table, chunk list and 8-float rows.  Arithmetic = torch.optim.SGD (torch 2.10's _single_tensor_sgd; maximize off),
// operation by operation, every operation rounded on its own:
//   g   = c * grad                                   (clipping only)
//   g   = g + wd * p                                 (only if wd != 0)
//   buf = buf * mu + damp1 * g                       (momentum; torch's first step, buf = clone(g), is the row
//                                                     mu = 0, damp1 = 1 over a zero-filled buffer: no branch)
//   g   = nesterov ? g + mu_n * buf : buf
//   p   = p + neg_lr * g
// HBM-streaming: 2 reads + 1 write per element = 12 B/param; with momentum 3 reads + 2 writes = 20 B/param.
#include "multi_tensor.hpp"
#include <cstring>
#include "../../include/bmnas_hip.h"

namespace {

struct Hyp {
  float neg_step, bc2_sqrt, beta2, eps, wd, w1, w2;
};

// DECOUPLED: h.wd holds f = float(1 - lr * weight_decay) and the decay is a product of its own on the parameter
// (mul_alone: never contracted into the update's multiply-add, so that f == 1 leaves the bits of the undecayed step); the
// gradient is not touched.  AMSGRAD: `vm` is the running maximum of v, and the denominator is built from it; compare and
// select, v winning when it is NaN — torch.maximum (fmaxf would drop a NaN).  Both false: the update as it always was.
template <bool DECOUPLED, bool AMSGRAD>
__device__ __forceinline__ void adam1(float& p, float g, float& m, float& v, float& vm, const Hyp& h) {
  if constexpr (DECOUPLED) {
    p = mul_alone(p, h.wd);
  } else {
    if (h.wd != 0.f) g = g + h.wd * p;
  }
  const float d = g - m;
  m = (h.w1 < 0.5f) ? m + h.w1 * d : g - d * (1.f - h.w1);      // at::lerp's two branches
  v = v * h.beta2 + h.w2 * (g * g);
  float s = v;
  if constexpr (AMSGRAD) {
    vm = (v > vm || v != v) ? v : vm;
    s = vm;
  }
  const float denom = sqrtf(s) / h.bc2_sqrt + h.eps;
  p = p + h.neg_step * (m / denom);
}

// One workgroup's chunk.  CLIP: the gradient is scaled by the clip coefficient `c` first — torch clips `.grad`, then
// Adam adds wd * p — as a product of its own (__fmul_rn: never contracted into the weight-decay multiply-add, so that
// c == 1 leaves the bits of the unclipped step).  CLIP = false is the kernel as it always was: `c` is not read.
// AMSGRAD: max_exp_avg_sq[ti] is tensor ti's running maximum (one pointer per descriptor; not read otherwise).
template <bool CLIP, bool DECOUPLED = false, bool AMSGRAD = false>
__device__ __forceinline__ void adam_chunk(const bmnas_adam_tensor_t* __restrict__ tensors,
                                           const int32_t* __restrict__ chunks, const float* __restrict__ hyp, float c,
                                           float* const* __restrict__ max_exp_avg_sq = nullptr) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  const float* hr = hyp + 8 * t.hyp_row;
  Hyp h;
  h.neg_step = hr[0]; h.bc2_sqrt = hr[1]; h.beta2 = hr[3]; h.eps = hr[4]; h.wd = hr[5];
  h.w1 = hr[6]; h.w2 = hr[7];
  float* mx = nullptr;
  if constexpr (AMSGRAD) mx = max_exp_avg_sq[ti];
  uintptr_t al = (uintptr_t)t.param | (uintptr_t)t.grad | (uintptr_t)t.exp_avg | (uintptr_t)t.exp_avg_sq;
  if constexpr (AMSGRAD) al |= (uintptr_t)mx;
  walk_chunk(t.numel, ci, al, [&](int64_t e) {
    float4 p = ld4(t.param + e), m = ld4(t.exp_avg + e), v = ld4(t.exp_avg_sq + e);
    float4 g = ld4(t.grad + e);
    float4 vm = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (AMSGRAD) vm = ld4(mx + e);
    if constexpr (CLIP) g = make_float4(__fmul_rn(g.x, c), __fmul_rn(g.y, c), __fmul_rn(g.z, c), __fmul_rn(g.w, c));
    adam1<DECOUPLED, AMSGRAD>(p.x, g.x, m.x, v.x, vm.x, h);
    adam1<DECOUPLED, AMSGRAD>(p.y, g.y, m.y, v.y, vm.y, h);
    adam1<DECOUPLED, AMSGRAD>(p.z, g.z, m.z, v.z, vm.z, h);
    adam1<DECOUPLED, AMSGRAD>(p.w, g.w, m.w, v.w, vm.w, h);
    st4_wtg<5>(t.param + e, p);
    st4_wtg<5>(t.exp_avg + e, m);
    st4_wtg<5>(t.exp_avg_sq + e, v);
    if constexpr (AMSGRAD) st4_wtg<5>(mx + e, vm);
  }, [&](int64_t i) {
    float p = t.param[i], m = t.exp_avg[i], v = t.exp_avg_sq[i];
    float g = t.grad[i];
    float vm = 0.f;
    if constexpr (AMSGRAD) vm = mx[i];
    if constexpr (CLIP) g = __fmul_rn(g, c);
    adam1<DECOUPLED, AMSGRAD>(p, g, m, v, vm, h);
    t.param[i] = p;
    t.exp_avg[i] = m;
    t.exp_avg_sq[i] = v;
    if constexpr (AMSGRAD) mx[i] = vm;
  });
}

__global__ __launch_bounds__(256) void adam_multi_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                    const int32_t* __restrict__ chunks,
                                                    const float* __restrict__ hyp) {
  adam_chunk<false>(tensors, chunks, hyp, 1.f);
}

// ---- global gradient-norm clipping (torch.nn.utils.clip_grad_norm_, norm_type 2) -----------------------------------
// Two launches, no atomics, no zero-fill: grad_sqnorm_multi_k leaves one partial sum of squares per workgroup of a FIXED
// grid; every workgroup of the consumer adds the partials in one fixed order, so all of them — and every run, and every
// data-parallel replica — derive the same bits.
__global__ __launch_bounds__(256) void grad_sqnorm_multi_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                           const int32_t* __restrict__ chunks, int n_chunks,
                                                           float* __restrict__ partials) {
  __shared__ float red[4];
  float acc = 0.f;
  for (int c = blockIdx.x; c < n_chunks; c += gridDim.x) {        // chunks w, w + G, w + 2G, ... in that order
    const bmnas_adam_tensor_t t = tensors[chunks[2 * c]];
    walk_chunk(t.numel, chunks[2 * c + 1], (uintptr_t)t.grad, [&](int64_t e) {
      const float4 g = ld4(t.grad + e);
      acc += g.x * g.x;
      acc += g.y * g.y;
      acc += g.z * g.z;
      acc += g.w * g.w;
    }, [&](int64_t i) { acc += t.grad[i] * t.grad[i]; });
  }
  const float total = block_sum256(acc, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// The norm and torch's coefficient: max_norm / (norm + 1e-6) clamped to <= 1 by a compare and select
// (a NaN norm gives a NaN coefficient, as torch.clamp does; fminf would give 1).  Every thread of the block gets both.
__device__ __forceinline__ float clip_coef(const float* __restrict__ partials, int n_parts,
                                           const float* __restrict__ clip, float* red, float& norm) {
  norm = norm_from_partials(partials, n_parts, red);
  const float c = clip[0] / (norm + 1e-6f);
  return (c > 1.f) ? 1.f : c;
}

__global__ __launch_bounds__(256) void adam_multi_clip_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                         const int32_t* __restrict__ chunks,
                                                         const float* __restrict__ hyp,
                                                         const float* __restrict__ partials, int n_parts,
                                                         const float* __restrict__ clip, float* __restrict__ norm_out) {
  __shared__ float red[4];
  float norm;
  const float c = clip_coef(partials, n_parts, clip, red, norm);
  if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
  adam_chunk<true>(tensors, chunks, hyp, c);
}

// Every combination but "both off": decoupled weight decay and / or the amsgrad running maximum, with or without the
// clip coefficient — one instantiation per launch (all tensors of an optimizer agree on the switches).
template <bool CLIP, bool DECOUPLED, bool AMSGRAD>
__global__ __launch_bounds__(256) void adam_multi_ex_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                       const int32_t* __restrict__ chunks,
                                                       const float* __restrict__ hyp,
                                                       float* const* __restrict__ max_exp_avg_sq,
                                                       const float* __restrict__ partials, int n_parts,
                                                       const float* __restrict__ clip, float* __restrict__ norm_out) {
  float c = 1.f;
  if constexpr (CLIP) {
    __shared__ float red[4];
    float norm;
    c = clip_coef(partials, n_parts, clip, red, norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
  }
  adam_chunk<CLIP, DECOUPLED, AMSGRAD>(tensors, chunks, hyp, c, max_exp_avg_sq);
}

__global__ __launch_bounds__(256) void grad_scale_multi_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                          const int32_t* __restrict__ chunks,
                                                          const float* __restrict__ partials, int n_parts,
                                                          const float* __restrict__ clip, float* __restrict__ norm_out) {
  __shared__ float red[4];
  float norm;
  const float c = clip_coef(partials, n_parts, clip, red, norm);
  if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
  const bmnas_adam_tensor_t t = tensors[chunks[2 * blockIdx.x]];
  float* __restrict__ grad = const_cast<float*>(t.grad);
  walk_chunk(t.numel, chunks[2 * blockIdx.x + 1], (uintptr_t)grad, [&](int64_t e) {
    const float4 g = ld4(grad + e);
    st4_wtg<5>(grad + e, make_float4(__fmul_rn(g.x, c), __fmul_rn(g.y, c), __fmul_rn(g.z, c), __fmul_rn(g.w, c)));
  }, [&](int64_t i) { grad[i] = __fmul_rn(grad[i], c); });
}

// ---- multi-tensor SGD (torch.optim.SGD) ---------------------------------------------------------------------------
// A row of `hyp`: { -lr, mu, 1 - dampening, mu_n, weight_decay, 0, 0, 0 }.  mu multiplies the buffer, mu_n the nesterov
// term: both are the group's momentum, except in a first-step row (mu = 0, damp1 = 1: buf = 0 * 0 + 1 * g = g).
struct SgdHyp {
  float neg_lr, mu, damp1, mu_n, wd;
};

// No contraction anywhere in the update: torch issues every operation as a launch of its own, each rounded once, and a
// term that is switched off by its scalar (damp1 == 1, c == 1) must leave the bits of the sequence without it —
// fma(damp1, g, buf * mu) would round differently from buf * mu + g.
template <bool MOMENTUM, bool NESTEROV>
__device__ __forceinline__ void sgd1(float& p, float g, float& buf, const SgdHyp& h) {
#pragma clang fp contract(off)
  if (h.wd != 0.f) g = g + h.wd * p;
  if constexpr (MOMENTUM) {
    buf = buf * h.mu + h.damp1 * g;
    g = NESTEROV ? g + h.mu_n * buf : buf;
  }
  p = p + h.neg_lr * g;
}

// One workgroup's chunk, as adam_chunk.  exp_avg of a descriptor is the momentum buffer; exp_avg_sq is not read, and
// with MOMENTUM false neither is exp_avg (both may be null).
template <bool CLIP, bool MOMENTUM, bool NESTEROV>
__device__ __forceinline__ void sgd_chunk(const bmnas_adam_tensor_t* __restrict__ tensors,
                                          const int32_t* __restrict__ chunks, const float* __restrict__ hyp, float c) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  const float* hr = hyp + 8 * t.hyp_row;
  SgdHyp h;
  h.neg_lr = hr[0]; h.mu = hr[1]; h.damp1 = hr[2]; h.mu_n = hr[3]; h.wd = hr[4];
  uintptr_t al = (uintptr_t)t.param | (uintptr_t)t.grad;
  if constexpr (MOMENTUM) al |= (uintptr_t)t.exp_avg;
  walk_chunk(t.numel, ci, al, [&](int64_t e) {
    float4 p = ld4(t.param + e);
    float4 g = ld4(t.grad + e);
    float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (MOMENTUM) b = ld4(t.exp_avg + e);
    if constexpr (CLIP) g = make_float4(mul_alone(g.x, c), mul_alone(g.y, c), mul_alone(g.z, c), mul_alone(g.w, c));
    sgd1<MOMENTUM, NESTEROV>(p.x, g.x, b.x, h);
    sgd1<MOMENTUM, NESTEROV>(p.y, g.y, b.y, h);
    sgd1<MOMENTUM, NESTEROV>(p.z, g.z, b.z, h);
    sgd1<MOMENTUM, NESTEROV>(p.w, g.w, b.w, h);
    st4_wtg<5>(t.param + e, p);
    if constexpr (MOMENTUM) st4_wtg<5>(t.exp_avg + e, b);
  }, [&](int64_t i) {
    float p = t.param[i], g = t.grad[i], b = 0.f;
    if constexpr (MOMENTUM) b = t.exp_avg[i];
    if constexpr (CLIP) g = mul_alone(g, c);
    sgd1<MOMENTUM, NESTEROV>(p, g, b, h);
    t.param[i] = p;
    if constexpr (MOMENTUM) t.exp_avg[i] = b;
  });
}

// One instantiation per launch: all tensors of an optimizer agree on the switches.
template <bool CLIP, bool MOMENTUM, bool NESTEROV>
__global__ __launch_bounds__(256) void sgd_multi_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                   const int32_t* __restrict__ chunks, const float* __restrict__ hyp,
                                                   const float* __restrict__ partials, int n_parts,
                                                   const float* __restrict__ clip, float* __restrict__ norm_out) {
  float c = 1.f;
  if constexpr (CLIP) {
    __shared__ float red[4];
    float norm;
    c = clip_coef(partials, n_parts, clip, red, norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) norm_out[0] = norm;
  }
  sgd_chunk<CLIP, MOMENTUM, NESTEROV>(tensors, chunks, hyp, c);
}

}  // namespace

extern "C" int bmnas_adam_chunk_elems(void) { return kChunk; }

extern "C" int bmnas_adam_multi(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                const float* hyp, void* stream) {
  if (!tensors || !chunks || !hyp || n_chunks < 0) return BMNAS_E_ARG;
  if (n_chunks == 0) return 0;
  hipLaunchKernelGGL(adam_multi_k, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, hyp);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_grad_norm_parts(void) { return kNormParts; }

extern "C" int bmnas_grad_sqnorm_multi(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                       float* partials, void* stream) {
  if (!tensors || !chunks || !partials || n_chunks <= 0) return BMNAS_E_ARG;
  const int g = norm_parts(n_chunks);
  hipLaunchKernelGGL(grad_sqnorm_multi_k, dim3(g), dim3(256), 0, (hipStream_t)stream, tensors, chunks, n_chunks,
                     partials);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

// `.grad` is NOT written: the clipped gradient exists only in registers (4 B per parameter of stores and a third
// launch saved); callers that read `.grad` after the step see the unclipped values.
extern "C" int bmnas_adam_multi_clip(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                     const float* hyp, const float* partials, int n_parts, const float* clip,
                                     float* norm_out, void* stream) {
  if (!tensors || !chunks || !hyp || !partials || !clip || !norm_out || n_chunks <= 0) return BMNAS_E_ARG;
  if (n_parts != norm_parts(n_chunks)) return BMNAS_E_ARG;   // what the norm launch wrote
  hipLaunchKernelGGL(adam_multi_clip_k, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, hyp,
                     partials, n_parts, clip, norm_out);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_adam_multi_ex(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                   const float* hyp, float* const* max_exp_avg_sq, int flags, const float* partials,
                                   int n_parts, const float* clip, float* norm_out, void* stream) {
  if (flags & ~(BMNAS_ADAM_AMSGRAD | BMNAS_ADAM_DECOUPLED)) return BMNAS_E_ARG;
  const bool ams = (flags & BMNAS_ADAM_AMSGRAD) != 0, dec = (flags & BMNAS_ADAM_DECOUPLED) != 0;
  if (ams != (max_exp_avg_sq != nullptr)) return BMNAS_E_ARG;
  const bool clipped = partials != nullptr;
  if ((clip != nullptr) != clipped || (norm_out != nullptr) != clipped) return BMNAS_E_ARG;
  if (flags == 0) {                                    // both switches off: the kernels that case always ran on
    return clipped ? bmnas_adam_multi_clip(tensors, chunks, n_chunks, hyp, partials, n_parts, clip, norm_out, stream)
                   : bmnas_adam_multi(tensors, chunks, n_chunks, hyp, stream);
  }
  if (!tensors || !chunks || !hyp || n_chunks < 0) return BMNAS_E_ARG;
  if (clipped && (n_chunks == 0 || n_parts != norm_parts(n_chunks))) return BMNAS_E_ARG;
  if (n_chunks == 0) return 0;
#define BMNAS_ADAM_EX(C, D, A)                                                                                       \
  hipLaunchKernelGGL((adam_multi_ex_k<C, D, A>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, \
                     hyp, max_exp_avg_sq, partials, n_parts, clip, norm_out)
  switch ((clipped ? 4 : 0) | flags) {
    case 1: BMNAS_ADAM_EX(false, false, true); break;
    case 2: BMNAS_ADAM_EX(false, true, false); break;
    case 3: BMNAS_ADAM_EX(false, true, true); break;
    case 5: BMNAS_ADAM_EX(true, false, true); break;
    case 6: BMNAS_ADAM_EX(true, true, false); break;
    default: BMNAS_ADAM_EX(true, true, true); break;
  }
#undef BMNAS_ADAM_EX
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_grad_scale_multi(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                      const float* partials, int n_parts, const float* clip, float* norm_out,
                                      void* stream) {
  if (!tensors || !chunks || !partials || !clip || !norm_out || n_chunks <= 0) return BMNAS_E_ARG;
  if (n_parts != norm_parts(n_chunks)) return BMNAS_E_ARG;
  hipLaunchKernelGGL(grad_scale_multi_k, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, partials,
                     n_parts, clip, norm_out);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

// `.grad` is NOT written, as in bmnas_adam_multi_clip.
extern "C" int bmnas_sgd_multi(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                               const float* hyp, int flags, const float* partials, int n_parts, const float* clip,
                               float* norm_out, void* stream) {
  if (flags & ~(BMNAS_SGD_MOMENTUM | BMNAS_SGD_NESTEROV)) return BMNAS_E_ARG;
  if (flags == BMNAS_SGD_NESTEROV) return BMNAS_E_ARG;                 // nesterov is a momentum method
  const bool clipped = partials != nullptr;
  if ((clip != nullptr) != clipped || (norm_out != nullptr) != clipped) return BMNAS_E_ARG;
  if (!tensors || !chunks || !hyp || n_chunks < 0) return BMNAS_E_ARG;
  if (clipped && (n_chunks == 0 || n_parts != norm_parts(n_chunks))) return BMNAS_E_ARG;
  if (n_chunks == 0) return 0;
#define BMNAS_SGD(C, M, N)                                                                                        \
  hipLaunchKernelGGL((sgd_multi_k<C, M, N>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, \
                     hyp, partials, n_parts, clip, norm_out)
  switch ((clipped ? 4 : 0) | flags) {
    case 0: BMNAS_SGD(false, false, false); break;
    case 1: BMNAS_SGD(false, true, false); break;
    case 3: BMNAS_SGD(false, true, true); break;
    case 4: BMNAS_SGD(true, false, false); break;
    case 5: BMNAS_SGD(true, true, false); break;
    default: BMNAS_SGD(true, true, true); break;
  }
#undef BMNAS_SGD
  BMNAS_CHECK_LAUNCH();
  return 0;
}

// ---- the batch into a captured step's static tensors: ONE launch (round 5) -----------------------------------------
// A replayed step reads its inputs from fixed addresses (bmnas.graph.GraphedTrainStep / GraphedForward): every call
// copies the caller's batch there first.  torch._foreach_copy_ is one launch only for lists it can batch (one dtype,
// and it fell back to a memcpy per tensor for the 8 + 1 small tensors of an NTU / Ego batch: 9 x 4.9 us in front of a
// 0.2 ms step); class-index labels (int64) were a copy of their own in any case.  Here up to kCopyMax (src, dst, bytes)
// triples of ANY dtype travel by value in the kernel arguments — no descriptor table to stage — and one grid of
// 16-byte lanes moves them all.  Replaces the reference's `.to(device)` hand-over of a batch only in so far as the
// batch is already on the device (train_searchable/mmimdb.py:60-63): host tensors keep torch's H2D copy.
namespace {
constexpr int kCopyMax = 16;
constexpr int kBlobWords = 64;                  // 256 bytes by value: eight rows of Adam scalars
struct CopyArgs {
  const void* src[kCopyMax];
  void* dst[kCopyMax];
  long long bytes[kCopyMax];
  int first[kCopyMax + 1];     // first workgroup of tensor i; first[n] = number of copy workgroups
  int n;
  // a few words that travel BY VALUE in the kernel arguments and are stored to device memory by one extra workgroup:
  // the per-step scalars of a captured optimizer step (learning rate / bias corrections, bmnas.optim.Adam) ride in
  // the launch that precedes the replay instead of an H2D copy node inside the graph (4.7 us per optimizer step)
  unsigned int* blob_dst;
  int blob_words;
  unsigned int blob[kBlobWords];
  // ... and one 64-bit device counter it advances: the dropout step counter of a captured step without a fused cell
  // prologue (found networks, evaluation forwards) — torch's `counter.add_(span)` node at the end of such a graph
  unsigned long long* add_dst;
  unsigned long long add_val;
};
constexpr int kCopyChunk = 256 * 16 * 4;        // bytes per workgroup: four 16-byte pieces per lane

__global__ __launch_bounds__(256) void copy_batch_k(CopyArgs a) {
  if ((int)blockIdx.x >= a.first[kCopyMax]) {                   // the blob's workgroup (last of the grid)
    if ((int)threadIdx.x < kBlobWords) {
      unsigned int v = a.blob[0];
#pragma unroll
      for (int i = 1; i < kBlobWords; ++i) v = ((int)threadIdx.x == i) ? a.blob[i] : v;   // selects: no indexed kernarg load
      if ((int)threadIdx.x < a.blob_words) a.blob_dst[threadIdx.x] = v;
    }
    if (threadIdx.x == 0 && a.add_dst != nullptr) a.add_dst[0] += a.add_val;
    return;
  }
  int ti = 0;
#pragma unroll
  for (int i = 1; i < kCopyMax; ++i) ti = (i < a.n && (int)blockIdx.x >= a.first[i]) ? i : ti;
  const char* __restrict__ s = (const char*)a.src[0];
  char* __restrict__ d = (char*)a.dst[0];
  long long nb = a.bytes[0];
  int f = a.first[0];
#pragma unroll
  for (int i = 1; i < kCopyMax; ++i) {        // selects over the by-value arrays: no indexed kernarg load
    const bool hit = ti == i;
    s = hit ? (const char*)a.src[i] : s;
    d = hit ? (char*)a.dst[i] : d;
    nb = hit ? a.bytes[i] : nb;
    f = hit ? a.first[i] : f;
  }
  const long long base = (long long)((int)blockIdx.x - f) * kCopyChunk;
  const long long full = nb & ~15ll;                            // bytes in whole 16-byte pieces
  if (s == nullptr) {
    // zero-fill job (workgroup-uniform): the accumulators a captured per-op step adds into with atomics (BatchNorm batch
    // sums, weight / affine gradients, the classifier's split-K output) are cleared by THIS launch, in front of the
    // replay, instead of by torch.zeros / zero_fill launches inside it (bmnas.functions.STEP_ARENA)
    const uint4 z4 = make_uint4(0u, 0u, 0u, 0u);
    if (((uintptr_t)d & 15) == 0) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const long long o = base + ((long long)r * 256 + threadIdx.x) * 16;
        if (o < full) st16_wt(d + o, z4);
      }
      if (full < nb && full >= base && full < base + kCopyChunk && (long long)threadIdx.x == ((full - base) >> 4) % 256)
        for (long long o = full; o < nb; ++o) d[o] = 0;
    } else {
      for (int r = 0; r < 4; ++r) {
        const long long o0 = base + ((long long)r * 256 + threadIdx.x) * 16;
        for (long long o = o0; o < nb && o < o0 + 16; ++o) d[o] = 0;
      }
    }
    return;
  }
  if ((((uintptr_t)s | (uintptr_t)d) & 15) == 0 && nb >= 16) {
    // four 16-byte pieces per lane, every load issued before the first store; scalars, not arrays (an indexed
    // per-lane array here was promoted to 16 KB of LDS per workgroup and the launch took 18 us for 9.4 MB)
    const long long o0 = base + (long long)threadIdx.x * 16, o1 = o0 + 4096, o2 = o0 + 8192, o3 = o0 + 12288;
    const bool f0 = o0 < full, f1 = o1 < full, f2 = o2 < full, f3 = o3 < full;
    const uint4 v0 = *reinterpret_cast<const uint4*>(s + (f0 ? o0 : 0));     // clamped: no load under a branch
    const uint4 v1 = *reinterpret_cast<const uint4*>(s + (f1 ? o1 : 0));
    const uint4 v2 = *reinterpret_cast<const uint4*>(s + (f2 ? o2 : 0));
    const uint4 v3 = *reinterpret_cast<const uint4*>(s + (f3 ? o3 : 0));
    if (f0) st16_wt(d + o0, v0);
    if (f1) st16_wt(d + o1, v1);
    if (f2) st16_wt(d + o2, v2);
    if (f3) st16_wt(d + o3, v3);
    // the last nb % 16 bytes: the lane whose piece would have held them
    if (full < nb && full >= base && full < base + kCopyChunk && (long long)threadIdx.x == ((full - base) >> 4) % 256)
      for (long long o = full; o < nb; ++o) d[o] = s[o];
  } else {
    for (int r = 0; r < 4; ++r) {
      const long long o0 = base + ((long long)r * 256 + threadIdx.x) * 16;
      for (long long o = o0; o < nb && o < o0 + 16; ++o) d[o] = s[o];
    }
  }
}
}  // namespace

extern "C" int bmnas_copy_batch_max(void) { return kCopyMax; }

extern "C" int bmnas_copy_blob_max(void) { return kBlobWords * 4; }

extern "C" int bmnas_copy_batch(const void* const* srcs, void* const* dsts, const long long* bytes, int n,
                                void* blob_dst, const void* blob, int blob_bytes, unsigned long long* add_dst,
                                unsigned long long add_val, void* stream) {
  if (n < 0 || n > kCopyMax || (n > 0 && (!srcs || !dsts || !bytes))) return BMNAS_E_ARG;
  if (blob_bytes < 0 || blob_bytes > kBlobWords * 4 || blob_bytes % 4 || (blob_bytes > 0 && (!blob_dst || !blob)))
    return BMNAS_E_ARG;
  CopyArgs a{};
  int g = 0, m = 0;
  for (int i = 0; i < n; ++i) {
    if (bytes[i] < 0 || (bytes[i] > 0 && !dsts[i])) return BMNAS_E_ARG;      // (srcs[i] == NULL: zero-fill dsts[i])
    if (bytes[i] == 0) continue;
    a.src[m] = srcs[i]; a.dst[m] = dsts[i]; a.bytes[m] = bytes[i]; a.first[m] = g;
    g += (int)((bytes[i] + kCopyChunk - 1) / kCopyChunk);
    ++m;
  }
  a.n = m;
  for (int i = m; i <= kCopyMax; ++i) a.first[i] = g;
  if (blob_bytes > 0) {
    a.blob_dst = static_cast<unsigned int*>(blob_dst);
    a.blob_words = blob_bytes / 4;
    memcpy(a.blob, blob, (size_t)blob_bytes);
  }
  a.add_dst = add_dst;
  a.add_val = add_val;
  if (blob_bytes > 0 || add_dst != nullptr) ++g;                // one more workgroup: it stores the blob / advances the counter
  if (g == 0) return 0;
  hipLaunchKernelGGL(copy_batch_k, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, a);
  BMNAS_CHECK_LAUNCH();
  return 0;
}
