// The walk of the multi-tensor launches over a (tensor, chunk) list, per workgroup — the ONE definition adam.hip,
// unroll.hip and average.hip compile — and the norm both derive from the partials of bmnas_grad_sqnorm_multi.
//
// A launch has one workgroup of 256 lanes per entry (ti, ci) of the chunk list: chunk ci of tensor ti is elements
// ci * kChunk .. + kChunk - 1, four consecutive ones per lane.  A lane whose four lie inside the tensor, in a tensor
// whose pointers are all 16-byte aligned, takes them as float4 (`vec`); every other lane — a tensor offset by a float
// or two, the last lane of a tensor whose size is no multiple of four — takes its at most four elements one by one
// (`one`), so the scalar tail never is more than four elements of one lane.  The caller reads the entry and the
// descriptor itself (what else it reads there differs) and ORs into `al` exactly the descriptor pointers its two
// lambdas dereference:
//   adam_chunk          param | grad | exp_avg | exp_avg_sq (| max_exp_avg_sq[ti] with AMSGRAD)   adam.hip
//   sgd_chunk           param | grad (| exp_avg with MOMENTUM)
//   grad_sqnorm_multi_k grad             (grid-stride: one walk per chunk of the workgroup, in ascending order)
//   grad_scale_multi_k  grad
//   unroll_virtual_k    param | grad | exp_avg_sq (| exp_avg with MOMENTUM; NULL is aligned)        unroll.hip
//   unroll_perturb_k    param | grad | exp_avg_sq
//   unroll_restore_k    param | exp_avg_sq
//   unroll_combine_k    param | grad | exp_avg
//   avg_multi_k         param | grad             (param the averaged tensor, grad the live one; RAW rows: as words) average.hip
// Both lambdas capture by reference and are inlined: every kernel keeps the registers, LDS and occupancy it had with
// the walk written out (profiles/r19_optim_walk.txt).
#pragma once
#include "common.hpp"

namespace {

constexpr int kChunk = 1024;      // elements per workgroup (256 lanes x float4): bmnas_adam_chunk_elems()
constexpr int kNormParts = 256;   // bmnas_grad_norm_parts(): partials = lanes of the consumer's one block_sum256

// The grid of the norm launch, i.e. how many partials it wrote: what every consumer's n_parts must be.
constexpr int norm_parts(int n_chunks) { return n_chunks < kNormParts ? n_chunks : kNormParts; }

// a * b rounded on its own: the product carries no permission to contract, so the compiler cannot fold it into a
// neighbouring addition as a fused multiply-add (__fmul_rn is a plain `*` to this compiler, and p * f + s * q became
// fma(f, p, s * q): with f == 1 that is p + round(s * q), not the fma(s, q, p) of the undecayed step)
__device__ __forceinline__ float mul_alone(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}

// sqrt(sum of the partials), the partials added in ONE fixed order — lane i holds partial i, one block_sum256 — so every
// workgroup of every consumer, every run and every data-parallel replica derives the same bits.  All 256 lanes call it.
__device__ __forceinline__ float norm_from_partials(const float* __restrict__ partials, int n_parts, float* red) {
  const float v = ((int)threadIdx.x < n_parts) ? partials[threadIdx.x] : 0.f;
  return sqrtf(block_sum256(v, red));
}

// This lane's part of chunk ci of a tensor of `numel` elements: vec(e) over elements e .. e + 3, or one(i) per element.
template <class V, class S>
__device__ __forceinline__ void walk_chunk(int64_t numel, int ci, uintptr_t al, V vec, S one) {
  const int64_t e = (int64_t)ci * kChunk + threadIdx.x * 4;
  if (e >= numel) return;
  if ((al & 15) == 0 && e + 4 <= numel) {
    vec(e);
  } else {
    const int64_t end = (e + 4 < numel) ? e + 4 : numel;
    for (int64_t i = e; i < end; ++i) one(i);
  }
}

}  // namespace
