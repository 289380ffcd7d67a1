// K1 — architecture-weighted mixed-edge sum (FusionMixedOp summed over incoming edges).
// Pure HBM-streaming kernels: one float4 per lane per input, all n_in loads issued before
// the FMAs; the backward fuses the n_in dx writes with n_in dot products
// (wave shuffle -> LDS -> one atomic per workgroup per scalar).
// Algorithmic bytes: fwd (n_in + 1) * T, bwd (2 * n_in + 1) * T, T = n_elem * 4.
#include "common.hpp"
#include "../../include/bmnas_hip.h"
#include "launch.hpp"

namespace {

template <int NIN>
__global__ __launch_bounds__(256) void mixsum_fwd_k(PtrsIn xs, const float* __restrict__ w,
                                                    int w_stride, float* __restrict__ out,
                                                    int64_t n4) {
  float wj[NIN];
#pragma unroll
  for (int j = 0; j < NIN; ++j) wj[j] = w[j * w_stride];
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v[NIN];
#pragma unroll
    for (int j = 0; j < NIN; ++j) v[j] = reinterpret_cast<const float4*>(xs.p[j])[i];
    float4 acc = f4_scale(v[0], wj[0]);
#pragma unroll
    for (int j = 1; j < NIN; ++j) {
      acc.x = fmaf(wj[j], v[j].x, acc.x);
      acc.y = fmaf(wj[j], v[j].y, acc.y);
      acc.z = fmaf(wj[j], v[j].z, acc.z);
      acc.w = fmaf(wj[j], v[j].w, acc.w);
    }
    st4_wt(out + 4 * i, acc);
  }
}

template <int NIN>
__global__ __launch_bounds__(256) void mixsum_bwd_k(PtrsIn xs, PtrsOut dxs,
                                                    const float* __restrict__ w, int w_stride,
                                                    const float* __restrict__ g,
                                                    const float* __restrict__ g2, float* dw,
                                                    int dw_shards, int64_t dw_shard_stride,
                                                    uint32_t acc_mask, int64_t n4) {
  __shared__ float red[4 * NIN];
  float wj[NIN], part[NIN];
#pragma unroll
  for (int j = 0; j < NIN; ++j) {
    wj[j] = w[j * w_stride];
    part[j] = 0.f;
  }
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 g4 = reinterpret_cast<const float4*>(g)[i];
    {                                                        // (unconditional load: no wait at a join)
      const float4 g2v = reinterpret_cast<const float4*>(g2 != nullptr ? g2 : g)[i];
      g4 = f4_add(g4, g2 != nullptr ? g2v : make_float4(0.f, 0.f, 0.f, 0.f));
    }
    if (dw != nullptr) {
      float4 v[NIN];
#pragma unroll
      for (int j = 0; j < NIN; ++j) v[j] = reinterpret_cast<const float4*>(xs.p[j])[i];
#pragma unroll
      for (int j = 0; j < NIN; ++j) part[j] += f4_dot(g4, v[j]);
    }
    // dx_j: destinations may alias each other (the same state feeding two edges), so the
    // read-modify-writes stay in program order through non-restrict pointers.
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      float* d = dxs.p[j];
      if (d == nullptr) continue;
      float4 r = f4_scale(g4, wj[j]);
      if (acc_mask & (1u << j)) r = f4_add(r, reinterpret_cast<float4*>(d)[i]);
      st4_wt(d + 4 * i, r);
    }
  }
  if (dw == nullptr) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j < NIN; ++j) {
    float s = wave_sum(part[j]);
    if (lane == 0) red[wave * NIN + j] = s;
  }
  __syncthreads();
  if (threadIdx.x < NIN) {
    const int j = threadIdx.x;
    // hundreds of workgroups adding into the same n_in scalars serialise on the atomics:
    // spread them over dw_shards copies (summed by the arch-softmax backward)
    float* d = dw + (int64_t)(blockIdx.x % dw_shards) * dw_shard_stride;
    atomicAdd(d + j * w_stride, red[j] + red[NIN + j] + red[2 * NIN + j] + red[3 * NIN + j]);
  }
}


// K1 pair — the cell-level sum h = sum_j w_j x_j together with the first inner-cell sum of the
// step node it feeds.  In search mode FusionNode is called as node(h, h) (model_search.py:59), so
// NodeCell's first mixed sum (node_search.py:54) is z = (w2_0 + w2_1) * h: written from the same
// registers instead of a second launch that re-reads h twice.
template <int NIN>
__global__ __launch_bounds__(256) void mixsum_pair_fwd_k(PtrsIn xs, const float* __restrict__ w,
                                                         int w_stride, const float* __restrict__ w2,
                                                         int w2_stride, float* __restrict__ out,
                                                         float* __restrict__ out2, int64_t n4) {
  float wj[NIN];
#pragma unroll
  for (int j = 0; j < NIN; ++j) wj[j] = w[j * w_stride];
  const float s2 = w2[0] + w2[w2_stride];
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    float4 v[NIN];
#pragma unroll
    for (int j = 0; j < NIN; ++j) v[j] = reinterpret_cast<const float4*>(xs.p[j])[i];
    float4 acc = f4_scale(v[0], wj[0]);
#pragma unroll
    for (int j = 1; j < NIN; ++j) {
      acc.x = fmaf(wj[j], v[j].x, acc.x);
      acc.y = fmaf(wj[j], v[j].y, acc.y);
      acc.z = fmaf(wj[j], v[j].z, acc.z);
      acc.w = fmaf(wj[j], v[j].w, acc.w);
    }
    st4_wt(out + 4 * i, acc);
    st4_wt(out2 + 4 * i, f4_scale(acc, s2));
  }
}

// backward of the pair: G = gh + (w2_0 + w2_1) * gz is the full gradient of h (gh: what the other
// consumers of h already accumulated, may be null); dx_j (+)= w_j G, dw_j += <G, x_j>,
// dw2_0 += <gz, h>, dw2_1 += <gz, h>.
// DOTS = false (dw == dw2 == NULL at the C ABI): nobody differentiates the edge weights — the weight step of the search
// loop — so the NIN inputs and h, read only for the dot products, are not loaded: dx_j needs G alone.
template <int NIN, bool DOTS = true>
__global__ __launch_bounds__(256) void mixsum_pair_bwd_k(PtrsIn xs, PtrsOut dxs,
                                                         const float* __restrict__ w, int w_stride,
                                                         const float* __restrict__ w2, int w2_stride,
                                                         const float* __restrict__ h,
                                                         const float* __restrict__ gh,
                                                         const float* __restrict__ gz,
                                                         const float* __restrict__ gz2, float* dw,
                                                         float* dw2, int dw_shards,
                                                         int64_t dw_shard_stride, uint32_t acc_mask,
                                                         int64_t n4) {
  __shared__ float red[4 * (NIN + 1)];
  float wj[NIN], part[NIN + 1];
#pragma unroll
  for (int j = 0; j < NIN; ++j) {
    wj[j] = w[j * w_stride];
    part[j] = 0.f;
  }
  part[NIN] = 0.f;
  const float s2 = w2[0] + w2[w2_stride];
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += stride) {
    // every load unconditional (an absent optional operand reads gz again and is masked out): a load under `if` is
    // a branch whose join waits for vmcnt(0) — gz, gz2 and gh were three dependent round trips before the operands
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 z4 = reinterpret_cast<const float4*>(gz)[i];
    const float4 z2v = reinterpret_cast<const float4*>(gz2 != nullptr ? gz2 : gz)[i];
    float4 h4 = zero4;
    if constexpr (DOTS) h4 = reinterpret_cast<const float4*>(h)[i];
    const float4 ghv = reinterpret_cast<const float4*>(gh != nullptr ? gh : gz)[i];
    float4 v[NIN];
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      if constexpr (DOTS) v[j] = reinterpret_cast<const float4*>(xs.p[j])[i];
      else v[j] = zero4;
    }
    z4 = f4_add(z4, gz2 != nullptr ? z2v : zero4);
    const float4 g4 = f4_add(f4_scale(z4, s2), gh != nullptr ? ghv : zero4);
#pragma unroll
    for (int j = 0; j < NIN; ++j) part[j] += f4_dot(g4, v[j]);
    part[NIN] += f4_dot(z4, h4);
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      float* d = dxs.p[j];
      if (d == nullptr) continue;
      float4 r = f4_scale(g4, wj[j]);
      if (acc_mask & (1u << j)) r = f4_add(r, reinterpret_cast<float4*>(d)[i]);
      st4_wt(d + 4 * i, r);
    }
  }
  if constexpr (!DOTS) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j <= NIN; ++j) {
    float s = wave_sum(part[j]);
    if (lane == 0) red[wave * (NIN + 1) + j] = s;
  }
  __syncthreads();
  if (threadIdx.x <= NIN + 1) {
    const int j = threadIdx.x < NIN ? threadIdx.x : NIN;
    const float v = red[j] + red[NIN + 1 + j] + red[2 * (NIN + 1) + j] + red[3 * (NIN + 1) + j];
    const int64_t sh = (int64_t)(blockIdx.x % dw_shards) * dw_shard_stride;
    if (threadIdx.x < NIN) atomicAdd(dw + sh + j * w_stride, v);
    else atomicAdd(dw2 + sh + (threadIdx.x - NIN) * w2_stride, v);
  }
}

// The FIRST cell step's pair backward when the later steps' K1 backward launches left their input gradients to it
// (write-once: every step's mixed sum reads the same N cell inputs, model_search.py:58, so dx_j is a sum over the
// steps — instead of S read-modify-write passes over the N tensors, step t > 0 stores only its G_t
// (bmnas_mixsum_pair_bwd_lazy, g_full) and this launch writes   dx_j = w_j G + sum_t wm_t[j] G_t   once).
constexpr int kMaxMoreG = 2;
struct MoreG {
  const float* g[kMaxMoreG];     // G_t (n_elem)
  const float* w[kMaxMoreG];     // softmaxed edge weights of step t's sum: w[t][j * w_stride], j < NIN
};

template <int NIN, int NX, bool DOTS = true>
__global__ __launch_bounds__(256) void mixsum_pair_bwd_x_k(PtrsIn xs, PtrsOut dxs,
                                                           const float* __restrict__ w, int w_stride,
                                                           const float* __restrict__ w2, int w2_stride,
                                                           const float* __restrict__ h,
                                                           const float* __restrict__ gh,
                                                           const float* __restrict__ gz,
                                                           const float* __restrict__ gz2, float* dw,
                                                           float* dw2, int dw_shards,
                                                           int64_t dw_shard_stride, uint32_t acc_mask,
                                                           MoreG X, int64_t n4) {
  __shared__ float red[4 * (NIN + 1)];
  float wj[NIN], wx[NX][NIN], part[NIN + 1];
  // one trip's operands.  Every load unconditional (an absent optional operand reads gz again and is masked out): a
  // load under `if` is a branch whose join waits for vmcnt(0) — gz, gz2 and gh were three dependent round trips
  // before the operands
  struct Trip {
    float4 z4, z2v, h4, ghv, gx[NX], v[NIN];
  };
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  auto issue = [&](int64_t i) {
    Trip t;
    t.z4 = reinterpret_cast<const float4*>(gz)[i];
    t.z2v = reinterpret_cast<const float4*>(gz2 != nullptr ? gz2 : gz)[i];
    t.h4 = zero4;
    if constexpr (DOTS) t.h4 = reinterpret_cast<const float4*>(h)[i];
    t.ghv = reinterpret_cast<const float4*>(gh != nullptr ? gh : gz)[i];
#pragma unroll
    for (int k = 0; k < NX; ++k) t.gx[k] = reinterpret_cast<const float4*>(X.g[k])[i];
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      if constexpr (DOTS) t.v[j] = reinterpret_cast<const float4*>(xs.p[j])[i];
      else t.v[j] = zero4;
    }
    return t;
  };
  const int64_t stride = (int64_t)gridDim.x * 256;
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool live = i < n4;
  auto weights = [&]() {
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      wj[j] = w[j * w_stride];
#pragma unroll
      for (int k = 0; k < NX; ++k) wx[k][j] = X.w[k][j * w_stride];
    }
    return w2[0] + w2[w2_stride];
  };
#pragma unroll
  for (int j = 0; j <= NIN; ++j) part[j] = 0.f;
  // on: false for a lane without a first trip — it adds nothing and stores nothing, but its arithmetic is not put
  // under a branch (the compiler sinks a load into the branch that holds its only use)
  auto finish = [&](const Trip& t, int64_t i, float s2, bool on) {
    const float4 z4 = f4_add(t.z4, gz2 != nullptr ? t.z2v : zero4);
    const float4 g4 = f4_add(f4_scale(z4, s2), gh != nullptr ? t.ghv : zero4);
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      const float dj = f4_dot(g4, t.v[j]);
      part[j] += on ? dj : 0.f;
    }
    const float dh = f4_dot(z4, t.h4);
    part[NIN] += on ? dh : 0.f;
#pragma unroll
    for (int j = 0; j < NIN; ++j) {
      float* d = dxs.p[j];
      if (d == nullptr || !on) continue;
      float4 r = f4_scale(g4, wj[j]);
#pragma unroll
      for (int k = 0; k < NX; ++k) {
        r.x = fmaf(wx[k][j], t.gx[k].x, r.x);
        r.y = fmaf(wx[k][j], t.gx[k].y, r.y);
        r.z = fmaf(wx[k][j], t.gx[k].z, r.z);
        r.w = fmaf(wx[k][j], t.gx[k].w, r.w);
      }
      if (acc_mask & (1u << j)) r = f4_add(r, reinterpret_cast<float4*>(d)[i]);
      st4_w0<10>(d + 4 * i, r);
    }
  };
  // The edge weights sit behind pointers of the argument block.  Read in front of the loop they were a second scalar
  // round trip that every vector load waited for: the first trip's operands are requested BEFORE them (a lane without
  // a first trip repeats the last element, n4 >= 1: every lane reaches the barrier below).  pin4 (common.hpp) keeps
  // the first trip's arithmetic — and with it the waits for the operands — behind the weights' loads.
  Trip t = issue(live ? i : n4 - 1);
  __builtin_amdgcn_sched_barrier(0);
  const float s2 = weights();
  __builtin_amdgcn_sched_barrier(0);
  pin4(t.z4);
  pin4(t.z2v);
  pin4(t.ghv);
  if constexpr (DOTS) pin4(t.h4);
#pragma unroll
  for (int k = 0; k < NX; ++k) pin4(t.gx[k]);
  if constexpr (DOTS) {
#pragma unroll
    for (int j = 0; j < NIN; ++j) pin4(t.v[j]);
  }
  finish(t, i, s2, live);
  for (i += stride; i < n4; i += stride) finish(issue(i), i, s2, true);   // (grids above 2048 workgroups' worth only)
  if constexpr (!DOTS) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
  for (int j = 0; j <= NIN; ++j) {
    float s = wave_sum(part[j]);
    if (lane == 0) red[wave * (NIN + 1) + j] = s;
  }
  __syncthreads();
  if (threadIdx.x <= NIN + 1) {
    const int j = threadIdx.x < NIN ? threadIdx.x : NIN;
    const float v = red[j] + red[NIN + 1 + j] + red[2 * (NIN + 1) + j] + red[3 * (NIN + 1) + j];
    const int64_t sh = (int64_t)(blockIdx.x % dw_shards) * dw_shard_stride;
    if (threadIdx.x < NIN) atomicAdd(dw + sh + j * w_stride, v);
    else atomicAdd(dw2 + sh + (threadIdx.x - NIN) * w2_stride, v);
  }
}

}  // namespace

extern "C" int bmnas_mixsum_fwd(const float* const* xs, int n_in, const float* w, int w_stride,
                                float* out, int64_t n_elem, void* stream) {
  if (!xs || !w || !out || n_in < 1 || n_elem < 0 || w_stride < 1) return BMNAS_E_ARG;
  if (n_in > BMNAS_MAX_PTRS) return BMNAS_E_LIMIT;
  if (n_elem % 4 != 0) return BMNAS_E_SHAPE;
  if (n_elem == 0) return 0;
  PtrsIn p{};
  if (int e = fill_ptrs(p.p, xs, n_in)) return e;
  const int64_t n4 = n_elem / 4;
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_range<1, BMNAS_MAX_PTRS>(n_in, [&](auto N) {
        hipLaunchKernelGGL(mixsum_fwd_k<decltype(N)::value>, dim3(stream_grid(n4)), dim3(256), 0, st, p, w, w_stride,
                           out, n4);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_mixsum_bwd(const float* const* xs, float* const* dxs, int n_in,
                                const float* w, int w_stride, const float* g, const float* g2,
                                float* dw, int dw_shards, int64_t dw_shard_stride,
                                uint32_t accumulate_mask, int64_t n_elem, void* stream) {
  if (!xs || !dxs || !w || !g || n_in < 1 || n_elem < 0 || w_stride < 1 || dw_shards < 1)
    return BMNAS_E_ARG;
  if (n_in > BMNAS_MAX_PTRS) return BMNAS_E_LIMIT;
  if (n_elem % 4 != 0) return BMNAS_E_SHAPE;
  if (n_elem == 0) return 0;
  PtrsIn p{};
  PtrsOut d{};
  if (int e = fill_ptrs(p.p, xs, n_in)) return e;
  fill_ptrs_out(d.p, dxs, n_in);
  const int64_t n4 = n_elem / 4;
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_range<1, BMNAS_MAX_PTRS>(n_in, [&](auto N) {
        hipLaunchKernelGGL(mixsum_bwd_k<decltype(N)::value>, dim3(stream_grid(n4)), dim3(256), 0, st, p, d, w,
                           w_stride, g, g2, dw, dw_shards, dw_shard_stride, accumulate_mask, n4);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_mixsum_pair_fwd(const float* const* xs, int n_in, const float* w, int w_stride,
                                     const float* w2, int w2_stride, float* out, float* out2,
                                     int64_t n_elem, void* stream) {
  if (!xs || !w || !w2 || !out || !out2 || n_in < 1 || n_elem < 0 || w_stride < 1 || w2_stride < 1)
    return BMNAS_E_ARG;
  if (n_in > BMNAS_MAX_PTRS) return BMNAS_E_LIMIT;
  if (n_elem % 4 != 0) return BMNAS_E_SHAPE;
  if (n_elem == 0) return 0;
  PtrsIn p{};
  if (int e = fill_ptrs(p.p, xs, n_in)) return e;
  const int64_t n4 = n_elem / 4;
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_range<1, BMNAS_MAX_PTRS>(n_in, [&](auto N) {
        hipLaunchKernelGGL(mixsum_pair_fwd_k<decltype(N)::value>, dim3(stream_grid(n4)), dim3(256), 0, st, p, w,
                           w_stride, w2, w2_stride, out, out2, n4);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_mixsum_pair_bwd(const float* const* xs, float* const* dxs, int n_in,
                                     const float* w, int w_stride, const float* w2, int w2_stride,
                                     const float* h, const float* gh, const float* gz,
                                     const float* gz2, float* dw, float* dw2, int dw_shards,
                                     int64_t dw_shard_stride,
                                     uint32_t accumulate_mask, int64_t n_elem, void* stream) {
  if (!xs || !dxs || !w || !w2 || !h || !gz || n_in < 1 || n_elem < 0 || w_stride < 1 || w2_stride < 1 ||
      dw_shards < 1)
    return BMNAS_E_ARG;
  if ((dw == nullptr) != (dw2 == nullptr)) return BMNAS_E_ARG;      // both (the dot products wanted) or neither
  const bool dots = dw != nullptr;
  if (n_in > BMNAS_MAX_PTRS - 1) return BMNAS_E_LIMIT;
  if (n_elem % 4 != 0) return BMNAS_E_SHAPE;
  if (n_elem == 0) return 0;
  PtrsIn p{};
  PtrsOut d{};
  if (int e = fill_ptrs(p.p, xs, n_in)) return e;
  fill_ptrs_out(d.p, dxs, n_in);
  const int64_t n4 = n_elem / 4;
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_range<1, BMNAS_MAX_PTRS - 1>(n_in, [&](auto N) {
        dispatch_bool(dots, [&](auto DOTS) {
          hipLaunchKernelGGL((mixsum_pair_bwd_k<decltype(N)::value, decltype(DOTS)::value>), dim3(stream_grid(n4)),
                             dim3(256), 0, st, p, d, w, w_stride, w2, w2_stride, h, gh, gz, gz2, dw, dw2, dw_shards,
                             dw_shard_stride, accumulate_mask, n4);
        });
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_mixsum_pair_bwd_x(const float* const* xs, float* const* dxs, int n_in,
                                       const float* w, int w_stride, const float* w2, int w2_stride,
                                       const float* h, const float* gh, const float* gz,
                                       const float* gz2, float* dw, float* dw2, int dw_shards,
                                       int64_t dw_shard_stride, uint32_t accumulate_mask,
                                       const float* const* g_more, const float* const* w_more, int n_more,
                                       int64_t n_elem, void* stream) {
  if (n_more == 0)
    return bmnas_mixsum_pair_bwd(xs, dxs, n_in, w, w_stride, w2, w2_stride, h, gh, gz, gz2, dw, dw2, dw_shards,
                                 dw_shard_stride, accumulate_mask, n_elem, stream);
  if (!xs || !dxs || !w || !w2 || !h || !gz || !g_more || !w_more || n_in < 1 || n_elem < 0 || w_stride < 1 ||
      w2_stride < 1 || dw_shards < 1)
    return BMNAS_E_ARG;
  if ((dw == nullptr) != (dw2 == nullptr)) return BMNAS_E_ARG;      // both (the dot products wanted) or neither
  const bool dots = dw != nullptr;
  if (n_more < 0 || n_more > kMaxMoreG || n_in > BMNAS_MAX_PTRS - 1) return BMNAS_E_LIMIT;
  if (n_elem % 4 != 0) return BMNAS_E_SHAPE;
  if (n_elem == 0) return 0;
  PtrsIn p{};
  PtrsOut d{};
  if (int e = fill_ptrs(p.p, xs, n_in)) return e;
  fill_ptrs_out(d.p, dxs, n_in);
  MoreG X{};
  for (int t = 0; t < n_more; ++t) {
    if (!g_more[t] || !w_more[t]) return BMNAS_E_ARG;
    X.g[t] = g_more[t];
    X.w[t] = w_more[t];
  }
  const int64_t n4 = n_elem / 4;
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_range<1, BMNAS_MAX_PTRS - 1>(n_in, [&](auto N) {
        dispatch_range<1, kMaxMoreG>(n_more, [&](auto NX) {
          dispatch_bool(dots, [&](auto DOTS) {
            hipLaunchKernelGGL((mixsum_pair_bwd_x_k<decltype(N)::value, decltype(NX)::value, decltype(DOTS)::value>),
                               dim3(stream_grid(n4)), dim3(256), 0, st, p, d, w, w_stride, w2, w2_stride, h, gh, gz,
                               gz2, dw, dw2, dw_shards, dw_shard_stride, accumulate_mask, X, n4);
          });
        });
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}
