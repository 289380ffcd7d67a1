// Multi-tensor weight averaging (torch.optim.swa_utils.AveragedModel: EMA and SWA of a model's tensors) as ONE launch
// over the descriptor table, the (tensor, chunk) list and the alignment rule of adam.hip: `param` of a descriptor is the
// AVERAGED tensor (read, written), `grad` the LIVE one (read only), `hyp_row` selects a 32-byte row (bmnas_avg_row_t).
//
// Arithmetic = at::lerp(a, p, w), operation by operation, every operation rounded on its own:
//   d = p - a
//   a = |w| < 0.5 ? a + w * d : p - d * omw          (omw = 1 - w, formed by the host; the branch is on a row scalar)
// With w = 1 (omw = 0) the second form is p - d * 0 = p for finite values: the first update of torch's class — a copy —
// is a ROW, not a kernel variant, and one captured graph serves the first replay and the later ones.
// A row flagged BMNAS_AVG_RAW copies 32-bit words bitwise (numel counts words): integer buffers, and every buffer of
// an averager that keeps buffers in sync by copy.
// Lane 0 of workgroup 0 stores its row's count to n_averaged: a value the host passed, no read-modify-write.
// HBM-streaming: 2 reads + 1 write per element = 12 B/element (RAW: 8 B per word).  Plain stores: nothing in a training
// step reads the averaged tensors, so the hand-off write-through stores of common.hpp are not for this.
#include "multi_tensor.hpp"
#include "../../include/bmnas_hip.h"

namespace {

static_assert(sizeof(bmnas_avg_row_t) == 32, "bmnas_avg_row_t is a 32-byte row");

// LOW: |w| < 0.5.  No contraction: fma(w, d, a) would round once where torch's two launches round twice.
template <bool LOW>
__device__ __forceinline__ float avg1(float a, float p, float w, float omw) {
#pragma clang fp contract(off)
  const float d = p - a;
  return LOW ? a + mul_alone(w, d) : p - mul_alone(d, omw);
}

template <bool LOW>
__device__ __forceinline__ void avg_chunk(const bmnas_adam_tensor_t& t, int ci, float w, float omw) {
  float* __restrict__ avg = t.param;
  const float* __restrict__ live = t.grad;
  walk_chunk(t.numel, ci, (uintptr_t)avg | (uintptr_t)live, [&](int64_t e) {
    float4 a = ld4(avg + e);
    const float4 p = ld4(live + e);
    a.x = avg1<LOW>(a.x, p.x, w, omw);
    a.y = avg1<LOW>(a.y, p.y, w, omw);
    a.z = avg1<LOW>(a.z, p.z, w, omw);
    a.w = avg1<LOW>(a.w, p.w, w, omw);
    st4(avg + e, a);
  }, [&](int64_t i) { avg[i] = avg1<LOW>(avg[i], live[i], w, omw); });
}

__device__ __forceinline__ void raw_chunk(const bmnas_adam_tensor_t& t, int ci) {
  uint32_t* __restrict__ dst = reinterpret_cast<uint32_t*>(t.param);
  const uint32_t* __restrict__ src = reinterpret_cast<const uint32_t*>(t.grad);
  walk_chunk(t.numel, ci, (uintptr_t)dst | (uintptr_t)src, [&](int64_t e) {
    *reinterpret_cast<uint4*>(dst + e) = *reinterpret_cast<const uint4*>(src + e);
  }, [&](int64_t i) { dst[i] = src[i]; });
}

__global__ __launch_bounds__(256) void avg_multi_k(const bmnas_adam_tensor_t* __restrict__ tensors,
                                                   const int32_t* __restrict__ chunks,
                                                   const bmnas_avg_row_t* __restrict__ rows,
                                                   int64_t* __restrict__ n_averaged) {
  const int ti = chunks[2 * blockIdx.x], ci = chunks[2 * blockIdx.x + 1];
  const bmnas_adam_tensor_t t = tensors[ti];
  const bmnas_avg_row_t h = rows[t.hyp_row];
  if (blockIdx.x == 0 && threadIdx.x == 0) n_averaged[0] = h.count;
  // the three forms are workgroup-uniform: the row is
  if (h.flags & BMNAS_AVG_RAW) raw_chunk(t, ci);
  else if (fabsf(h.w) < 0.5f) avg_chunk<true>(t, ci, h.w, h.omw);
  else avg_chunk<false>(t, ci, h.w, h.omw);
}

}  // namespace

extern "C" int bmnas_avg_multi(const bmnas_adam_tensor_t* tensors, const int32_t* chunks, int n_chunks,
                               const bmnas_avg_row_t* rows, int64_t* n_averaged, void* stream) {
  if (!tensors || !chunks || !rows || !n_averaged || n_chunks <= 0) return BMNAS_E_ARG;
  hipLaunchKernelGGL(avg_multi_k, dim3(n_chunks), dim3(256), 0, (hipStream_t)stream, tensors, chunks, rows,
                     n_averaged);
  BMNAS_CHECK_LAUNCH();
  return 0;
}
