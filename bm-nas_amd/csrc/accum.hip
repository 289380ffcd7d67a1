// Multi-tensor gradient combine: grad = sum_i w_i * part_i over the m micro-batch gradients of every tensor of a
// descriptor table, as ONE launch per optimizer step whatever m is.  Replaces autograd's AccumulateGrad over m backward
// passes (m adds per tensor) and, with w_i = n_i / N, the gradient reduction of nn.DataParallel in the reference's
// train_darts_model (models/search/ntu_darts_searchable.py): m mean-reduced micro-batch gradients weighted n_i / N are
// the gradient m data-parallel ranks would all-reduce.
//
// The grid, the (tensor, chunk) list and the alignment rule are those of adam.hip (multi_tensor.hpp).  The destination
// is the descriptor's `grad` field, written as bmnas_grad_scale_multi writes it; param, exp_avg, exp_avg_sq and hyp_row
// are not read.  parts[ti * m + i] is part i of tensor ti (device memory); the m weights travel BY VALUE in the kernel
// arguments (nothing to stage).
//
// Arithmetic, every operation rounded on its own (no fused multiply-add), over the non-NULL parts in ascending i:
//   acc = w_i0 * g_i0;   acc = acc + w_i * g_i
// A NULL part (that micro-batch gave the tensor no gradient) is left OUT, not added as zero; a tensor with no part at
// all gets +0.  w == 1 leaves the bits of the part: m = 1, w = 1 is a bit copy.  NaN propagates.
//
// All m loads of a lane are issued before the first is used (one memory round trip per lane, not m): a NULL part loads
// from the tensor's first non-NULL part instead — a line the lane holds anyway — and is dropped by a workgroup-uniform
// select, so no load sits under a branch.  m is a template parameter: the loop is unrolled, the parts stay in named
// registers (m float4 per lane) and the weights are compile-time kernel-argument offsets.  Write-through stores: the
// next launch (the norm, or the update) reads the result.  No atomics, no LDS.
// HBM-streaming: m reads + 1 write per element = 4 (m + 1) B/param.
#include "multi_tensor.hpp"
#include "../../include/bmnas_hip.h"

namespace {

struct AccumWeights {
  float w[BMNAS_ACCUM_MAX];
};

// acc + w * g with the product and the sum rounded separately
__device__ __forceinline__ float accum1(float acc, float w, float g) {
#pragma clang fp contract(off)
  const float t = w * g;
  return acc + t;
}

template <int M>
__global__ __launch_bounds__(256) void grad_combine_multi_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                            const int32_t* __restrict__ chunks,
                                                            const float* const* __restrict__ parts, AccumWeights aw) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  float* __restrict__ dst = const_cast<float*>(t.grad);
  const float* src[M];
  bool has[M];
  const float* any = nullptr;
  uintptr_t al = (uintptr_t)dst;
#pragma unroll
  for (int i = 0; i < M; ++i) {
    src[i] = parts[(int64_t)ti * M + i];
    has[i] = src[i] != nullptr;
    al |= (uintptr_t)src[i];
    any = (any == nullptr) ? src[i] : any;
  }
  if (any == nullptr) {                                    // no part at all (workgroup-uniform): +0, nothing loaded
    walk_chunk(t.numel, ci, (uintptr_t)dst, [&](int64_t e) {
      st4_wtg<5>(dst + e, make_float4(0.f, 0.f, 0.f, 0.f));
    }, [&](int64_t i) { dst[i] = 0.f; });
    return;
  }
#pragma unroll
  for (int i = 0; i < M; ++i) src[i] = has[i] ? src[i] : any;   // (`any` is one of the ORed pointers: `al` stands)
  walk_chunk(t.numel, ci, al, [&](int64_t e) {
    float4 g[M];
#pragma unroll
    for (int i = 0; i < M; ++i) g[i] = ld4(src[i] + e);
#pragma unroll
    for (int i = 0; i < M; ++i) pin4(g[i]);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool first = true;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if (!has[i]) continue;
      const float w = aw.w[i];
      if (first) {
        acc = make_float4(mul_alone(w, g[i].x), mul_alone(w, g[i].y), mul_alone(w, g[i].z), mul_alone(w, g[i].w));
        first = false;
      } else {
        acc = make_float4(accum1(acc.x, w, g[i].x), accum1(acc.y, w, g[i].y), accum1(acc.z, w, g[i].z),
                          accum1(acc.w, w, g[i].w));
      }
    }
    st4_wtg<5>(dst + e, acc);
  }, [&](int64_t j) {
    float g[M];
#pragma unroll
    for (int i = 0; i < M; ++i) g[i] = src[i][j];
#pragma unroll
    for (int i = 0; i < M; ++i) pin1(g[i]);
    float acc = 0.f;
    bool first = true;
#pragma unroll
    for (int i = 0; i < M; ++i) {
      if (!has[i]) continue;
      acc = first ? mul_alone(aw.w[i], g[i]) : accum1(acc, aw.w[i], g[i]);
      first = false;
    }
    dst[j] = acc;
  });
}

}  // namespace

extern "C" int bmnas_accum_max(void) { return BMNAS_ACCUM_MAX; }

extern "C" int bmnas_grad_combine_multi(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                                        const float* const* parts, int m, const float* weights, void* stream) {
  if (!tensors || !chunks || !parts || !weights || m < 1 || m > BMNAS_ACCUM_MAX || n_chunks < 0) return BMNAS_E_ARG;
  if (n_chunks == 0) return 0;
  AccumWeights aw{};
  for (int i = 0; i < m; ++i) aw.w[i] = weights[i];
#define BMNAS_COMBINE(M)                                                                                            \
  hipLaunchKernelGGL((grad_combine_multi_k<M>), dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, \
                     parts, aw)
  switch (m) {
    case 1: BMNAS_COMBINE(1); break;
    case 2: BMNAS_COMBINE(2); break;
    case 3: BMNAS_COMBINE(3); break;
    case 4: BMNAS_COMBINE(4); break;
    case 5: BMNAS_COMBINE(5); break;
    case 6: BMNAS_COMBINE(6); break;
    case 7: BMNAS_COMBINE(7); break;
    default: BMNAS_COMBINE(8); break;
  }
#undef BMNAS_COMBINE
  BMNAS_CHECK_LAUNCH();
  return 0;
}
