// Row-softmax backward of the architecture tensors (alpha / betas / gammas), shared by the
// stand-alone launch (bnmix.hip) and the backward epilogue launch (layernorm.hip).
#pragma once
#include "common.hpp"

namespace {

struct ArchPack {
  const float* a[BMNAS_MAX_PTRS];     // fwd: logits      bwd: softmax weights
  const float* b[BMNAS_MAX_PTRS];     //                  bwd: dweights
  float* o[BMNAS_MAX_PTRS];           // fwd: weights     bwd: dlogits
  int rows[BMNAS_MAX_PTRS], cols[BMNAS_MAX_PTRS];
  int n, n_shards;
  int64_t shard_stride;               // bwd: dweights are summed over n_shards copies
};

// one wavefront per row r (of the concatenation of all tensors; the SAME r in every lane of the wave):
// lane = (shard group, column); shards beyond 16 are walked by the same lane, in ascending order.
// r is made wave-uniform for the compiler too (readfirstlane), so that the walk over the tensors is scalar: every
// rows[] / cols[] entry comes out of the argument block in one batch of scalar loads, the row's tensor t is picked by
// selects, and the three pointers follow as scalar loads issued together — with a per-lane r each of them was a
// VECTOR load from the argument block plus a wait in front of the data load it feeds (pick_ptr, common.hpp).  Then
// one vector round trip: the weight and the shard copies (two per lane and trip, clamped, masked when added).
__device__ __forceinline__ void arch_softmax_bwd_row(const ArchPack& P, int r, int lane) {
  const int col = lane & 3, sg = lane >> 2;
  r = __builtin_amdgcn_readfirstlane(r);
  int t = -1, rt = 0;
#pragma unroll
  for (int q = 0; q < BMNAS_MAX_PTRS; ++q) {
    const bool here = t < 0 && q < P.n && r < P.rows[q];
    t = here ? q : t;
    rt = here ? r : rt;
    r -= (t < 0 && q < P.n) ? P.rows[q] : 0;
  }
  if (t < 0) return;                                               // (r beyond the last tensor: uniform)
  const int cols = P.cols[t];
  const float* __restrict__ ap = P.a[t];
  const float* __restrict__ bp = P.b[t];
  float* __restrict__ op = P.o[t];
  const bool live = col < cols;
  const int at = rt * cols + (live ? col : 0);                     // clamped address, no predicated loads
  const float* dwp = bp + at;
  const int ns = P.n_shards;                                       // (>= 1, host-checked)
  const int64_t stride = P.shard_stride;
  // shards sg and sg + 16 with the weight: the whole row at n_shards <= 32 ...
  const float wv = ap[at];
  const float v0 = dwp[(int64_t)(sg < ns ? sg : ns - 1) * stride];
  const float v1 = dwp[(int64_t)(sg + 16 < ns ? sg + 16 : ns - 1) * stride];
  float dw = 0.f;
  if (live && sg < ns) dw += v0;
  if (live && sg + 16 < ns) dw += v1;
  for (int s0 = 32; s0 < ns; s0 += 32) {                           // ... two more per lane and trip above that
    const int sa = s0 + sg, sb = sa + 16;
    const float va = dwp[(int64_t)(sa < ns ? sa : ns - 1) * stride];
    const float vb = dwp[(int64_t)(sb < ns ? sb : ns - 1) * stride];
    if (live && sa < ns) dw += va;
    if (live && sb < ns) dw += vb;
  }
  const float w = live ? wv : 0.f;
  dw = row_stride4_sum(dw);
  dw = xor16_sum(dw);
  dw = xor32_sum(dw);                                          // every lane: total of its column
  float dot = w * dw;
  dot += lane_xor1(dot);
  dot += lane_xor2(dot);                                       // sum over the 4 columns
  if (sg == 0 && live) op[at] = w * (dw - dot);
}

// host side: fill a pack from the C-ABI arrays; returns the total row count or a negative error
inline int fill_arch_pack(ArchPack& P, const float* const* a, const float* const* dw, float* const* out,
                          const int* rows, const int* cols, int n, int backward, int n_shards,
                          int64_t shard_stride) {
  if (!a || !out || !rows || !cols || n < 1 || (backward && !dw) || n_shards < 1) return BMNAS_E_ARG;
  if (n > BMNAS_MAX_PTRS) return BMNAS_E_LIMIT;
  int total = 0;
  for (int t = 0; t < n; ++t) {
    if (!a[t] || !out[t] || rows[t] < 1 || cols[t] < 1 || cols[t] > 4 || (backward && !dw[t]))
      return BMNAS_E_ARG;
    P.a[t] = a[t];
    P.b[t] = backward ? dw[t] : nullptr;
    P.o[t] = out[t];
    P.rows[t] = rows[t];
    P.cols[t] = cols[t];
    total += rows[t];
  }
  P.n = n;
  P.n_shards = n_shards;
  P.shard_stride = shard_stride;
  return total;
}

}  // namespace
