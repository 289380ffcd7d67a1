// K6 / K7 — channel-concat (+ residual) + LayerNorm([D/L, L]) (+ ReLU), one workgroup per
// sample: the whole (D = n_src*C*L)-element sample lives in registers (VPT float4 per
// thread), two block reductions (mean, then centred second moment), one coalesced write.
// Algorithmic bytes fwd: (n_src [+1 resid] + n_src) * T (+ 2*D*4 params), T = b*C*L*4.
#include "common.hpp"
#include <cstdlib>
#include "../../include/bmnas_hip.h"
#include "arch_body.hpp"
#include "ln_sample.hpp"
#include "launch.hpp"

namespace {

struct LnSrc {
  const float* p[4];
};
struct LnDst {
  float* p[4];
};

// float4 index i (within the concatenated sample) -> pointer into source q
__device__ __forceinline__ const float* src_ptr(const LnSrc& s, int i4, int cl4, int sample) {
  const int q = i4 / cl4;
  const int off = i4 - q * cl4;
  return pick_ptr(s.p, q) + ((int64_t)sample * cl4 + off) * 4;      // (never s.p[q]: an indexed kernarg LOAD, common.hpp)
}

// BS = threads per workgroup: 512 when the batch leaves CUs idle (one workgroup per sample), so
// that a sample is spread over twice the waves and each thread's dependent chain is half as long.
template <int VPT, int BS>
__global__ __launch_bounds__(BS) void cat_ln_fwd_k(LnSrc srcs, const float* __restrict__ resid,
                                                    const float* __restrict__ ln_w,
                                                    const float* __restrict__ ln_b,
                                                    float* __restrict__ out,
                                                    float* __restrict__ stats, int cl4, int d4,
                                                    int relu, float* __restrict__ osum) {
  __shared__ float red[8];
  __shared__ float red6[8 * 6];
  const int s = blockIdx.x;
  float4 v[VPT], lw[VPT], lb[VPT];
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * BS;
    if (i < d4) {
      v[k] = ld4(src_ptr(srcs, i, cl4, s));
      if (resid != nullptr) v[k] = f4_add(v[k], ld4(resid + ((int64_t)s * d4 + i) * 4));
      lw[k] = ld4(ln_w + (int64_t)i * 4);          // requested with the sample: no second round
      lb[k] = ld4(ln_b + (int64_t)i * 4);          // trip after the two reductions
      sum += f4_hsum(v[k]);
    } else {
      v[k] = lw[k] = lb[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
  const float inv_d = 1.f / (float)(d4 * 4);
  const float mean = block_sum_fresh<BS / 64>(sum, red) * inv_d;     // (first use of red: no barrier in front)
  // second pass: the centred second moment and — same reduction round, when asked for — what the
  // per-sample sums of the OUTPUT need (see node_mix_ln_fwd_k; without ReLU only)
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  const bool sums = osum != nullptr && !relu;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * BS;
    if (i < d4) {
      const float4 c = make_float4(v[k].x - mean, v[k].y - mean, v[k].z - mean, v[k].w - mean);
      acc[0] += f4_dot(c, c);
      if (sums) {
        const float4 cw = f4_mul(c, lw[k]);
        acc[1] += f4_hsum(cw);
        acc[2] += f4_dot(cw, cw);
        acc[3] += f4_dot(cw, lb[k]);
        acc[4] += f4_hsum(lb[k]);
        acc[5] += f4_dot(lb[k], lb[k]);
      }
    }
  }
  if (sums) {
    block_sum_lead_fresh<BS / 64, 6>(acc, red6);
  } else {
    acc[0] = block_sum_fresh<BS / 64>(acc[0], red6);         // (red6, not red: threads may still be reading the mean)
  }
  const float var = acc[0] * inv_d;
  const float rstd = 1.f / sqrtf(var + kLnEps);
  if (threadIdx.x == 0) {
    stats[2 * s] = mean;
    stats[2 * s + 1] = rstd;
    if (sums) {
      osum[2 * s] = rstd * acc[1] + acc[4];
      osum[2 * s + 1] = rstd * rstd * acc[2] + 2.f * rstd * acc[3] + acc[5];
    }
  }
  float os = 0.f, oq = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * BS;
    if (i < d4) {
      float4 o = ln_apply4(v[k], mean, rstd, lw[k], lb[k]);
      if (relu) {
        o.x = fmaxf(o.x, 0.f); o.y = fmaxf(o.y, 0.f); o.z = fmaxf(o.z, 0.f); o.w = fmaxf(o.w, 0.f);
      }
      st4_wtg<3>(out + ((int64_t)s * d4 + i) * 4, o);
      os += f4_hsum(o);
      oq += f4_dot(o, o);
    }
  }
  // with ReLU the sums cannot be derived from the moments: reduce the outputs themselves
  if (osum != nullptr && relu) {
    os = block_sum_fresh<BS / 64>(os, red);                  // (red's readers all passed the second reduction's barrier)
    oq = block_sum<BS / 64>(oq, red6);
    if (threadIdx.x == 0) {
      osum[2 * s] = os;
      osum[2 * s + 1] = oq;
    }
  }
}

template <int VPT, int BS>
__global__ __launch_bounds__(BS) void cat_ln_bwd_k(const float* __restrict__ g, LnSrc srcs,
                                                    const float* __restrict__ resid,
                                                    const float* __restrict__ ln_w,
                                                    const float* __restrict__ ln_b,
                                                    const float* __restrict__ stats, LnDst dsrcs,
                                                    float* dresid, uint32_t acc_mask, float* dln_w,
                                                    float* dln_b, int cl4, int d4, int relu,
                                                    float* __restrict__ scrub, int64_t scrub4) {
  __shared__ float red[2 * (BS / 64)];
  const int s = blockIdx.x;
  // side job: clear the caller's accumulation arena (saves a memset launch per backward)
  for (int64_t i = (int64_t)blockIdx.x * BS + threadIdx.x; i < scrub4; i += (int64_t)gridDim.x * BS)
    st4_wtg<3>(scrub + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
  const float mean = stats[2 * s], rstd = stats[2 * s + 1];
  float4 xh[VPT], dxh[VPT];
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * BS;
    if (i < d4) {
      float4 x = ld4(src_ptr(srcs, i, cl4, s));
      if (resid != nullptr) x = f4_add(x, ld4(resid + ((int64_t)s * d4 + i) * 4));
      const float4 w = ld4(ln_w + (int64_t)i * 4);
      float4 gy = ld4(g + ((int64_t)s * d4 + i) * 4);
      const float4 h = ln_xhat4(x, mean, rstd);
      if (relu) {
        const float4 bb = ld4(ln_b + (int64_t)i * 4);
        if (h.x * w.x + bb.x <= 0.f) gy.x = 0.f;
        if (h.y * w.y + bb.y <= 0.f) gy.y = 0.f;
        if (h.z * w.z + bb.z <= 0.f) gy.z = 0.f;
        if (h.w * w.w + bb.w <= 0.f) gy.w = 0.f;
      }
      if (dln_w != nullptr) {
        float* pw = dln_w + (int64_t)i * 4;
        float* pb = dln_b + (int64_t)i * 4;
        atomicAdd(pw + 0, gy.x * h.x); atomicAdd(pw + 1, gy.y * h.y);
        atomicAdd(pw + 2, gy.z * h.z); atomicAdd(pw + 3, gy.w * h.w);
        atomicAdd(pb + 0, gy.x); atomicAdd(pb + 1, gy.y);
        atomicAdd(pb + 2, gy.z); atomicAdd(pb + 3, gy.w);
      }
      const float4 d = f4_mul(gy, w);
      xh[k] = h;
      dxh[k] = d;
      s1 += f4_hsum(d);
      s2 += f4_dot(d, h);
    } else {
      xh[k] = make_float4(0.f, 0.f, 0.f, 0.f);
      dxh[k] = xh[k];
    }
  }
  const float inv_d = 1.f / (float)(d4 * 4);
  // both sums behind ONE barrier (two block_sum calls were four; `red` is written once per launch)
  ln_bwd_sums_put<BS / 64>(s1, s2, red);
  __syncthreads();
  float m1, m2;
  ln_bwd_sums_get<BS / 64>(red, inv_d, m1, m2);
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = threadIdx.x + k * BS;
    if (i < d4) {
      const float4 dx = ln_dx4(dxh[k], xh[k], m1, m2, rstd);
      const int q = i / cl4;
      const int off = i - q * cl4;
      float* d = pick_ptr(dsrcs.p, q);
      if (d != nullptr) {
        float* a = d + ((int64_t)s * cl4 + off) * 4;
        st4_wtg<3>(a, (acc_mask & (1u << q)) ? f4_add(dx, ld4(a)) : dx);
      }
      if (dresid != nullptr) {
        float* a = dresid + ((int64_t)s * d4 + i) * 4;
        st4_wtg<3>(a, (acc_mask & (1u << 31)) ? f4_add(dx, ld4(a)) : dx);
      }
    }
  }
}


// LayerNorm affine gradients dln_w[e] = sum_s gy[s,e]*x_hat[s,e], dln_b[e] = sum_s gy[s,e]:
// a reduction over SAMPLES per element.  Workgroup = 64 float4 columns x 4 sample lanes
// (one wave per sample lane -> 1 KiB coalesced rows); each thread walks its share of the
// sample chunk, the four lanes are summed through LDS, one atomic per element per chunk
// (b/16 x fewer atomics than doing it per sample).  prenorm: srcs[0] already holds x_hat.
struct LnAffineProb {
  const float* g;
  const float* gscale;
  LnSrc srcs;
  const float* resid;
  const float* ln_w;
  const float* ln_b;
  const float* stats;
  float* dln_w;
  float* dln_b;
  int cl4, d4, relu, prenorm;
};

constexpr int kMaxLnProbs = 8;
struct LnAffineBatch {
  LnAffineProb p[kMaxLnProbs];
  int n, b, chunk;
};

// The loads of FOUR sample trips (x, gy, resid, stats) go out together, before the first FMA, from clamped addresses
// and without a branch around any of them: an absent operand (resid, stats under prenorm, ln_w / ln_b without ReLU,
// gscale) reads g instead and is dropped by a select.  A sample chunk of 16 (b <= 256) is one such group = one memory
// round trip per workgroup; the loop form — load under `if`, s_waitcnt vmcnt(0) at the join, per trip — was 8 to 12.
// Longer chunks run in groups of four trips.  aw / ab still accumulate in sample order.
// P's fields are copied into registers first: P is B.p[blockIdx.z], a run-time index into the argument block, and
// inside the loop every use was a scalar load of its own.
__device__ __forceinline__ void ln_affine_body(const LnAffineProb& P, int b, int chunk, float4 (*red)[3][64]) {
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int d4 = P.d4, cl4 = P.cl4;
  const bool relu = P.relu != 0, prenorm = P.prenorm != 0;
  const float* __restrict__ g = P.g;
  const float* gscale = P.gscale;
  const float* resid = P.resid;
  const float* stats = P.stats;
  const float* ln_w = P.ln_w;
  const float* ln_b = P.ln_b;
  float* dln_w = P.dln_w;
  float* dln_b = P.dln_b;
  const float* src[4] = {sgpr_ptr(P.srcs.p[0]), sgpr_ptr(P.srcs.p[1]), sgpr_ptr(P.srcs.p[2]), sgpr_ptr(P.srcs.p[3])};
  const int i0 = blockIdx.x * 64 + col;
  const bool active = i0 < d4;
  const int i = active ? i0 : d4 - 1;                                // clamped: an idle lane repeats the last column
  const int q = i / cl4;
  const int off = i - q * cl4;
  const float* xsrc = src[0];                                        // (selects over SGPR pointers, pick_ptr)
#pragma unroll
  for (int qq = 1; qq < 4; ++qq) xsrc = (q == qq) ? src[qq] : xsrc;
  const bool has_r = !prenorm && resid != nullptr, has_st = !prenorm;
  const float* rp = has_r ? resid : g;
  const float* sp = has_st ? stats : g;                              // (g holds >= 4 b floats)
  const float4 w = ld4((relu ? ln_w : g) + (int64_t)i * 4);
  const float4 bb = ld4((relu ? ln_b : g) + (int64_t)i * 4);
  const float gsv = (gscale != nullptr ? gscale : g)[0];           // (selected behind the first batch, below)
  float4 aw = make_float4(0.f, 0.f, 0.f, 0.f), ab = aw;
  const int s_beg = blockIdx.y * chunk;
  int s_end = s_beg + chunk;
  if (s_end > b) s_end = b;
  for (int sg = s_beg; sg < s_end; sg += 16) {
    float4 xv[4], gv[4], rv[4];
    float mean[4], rstd[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int s_raw = sg + 4 * k + sl;
      const int s = s_raw < s_end ? s_raw : s_end - 1;
      xv[k] = ld4(xsrc + ((int64_t)s * cl4 + off) * 4);
      gv[k] = ld4(g + ((int64_t)s * d4 + i) * 4);
      rv[k] = ld4(rp + ((int64_t)s * d4 + i) * 4);
      mean[k] = sp[2 * s];
      rstd[k] = sp[2 * s + 1];
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                    // (pin4, common.hpp: the batch stays a batch)
      pin4(xv[k]);
      pin4(gv[k]);
      pin4(rv[k]);
      pin1(mean[k]);
      pin1(rstd[k]);
    }
    float gs = gsv;
    pin1(gs);                                                        // (not hoisted in front of the loop: a wait there)
    gs = gscale != nullptr ? gs : 1.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (sg + 4 * k + sl < s_end) {
        float4 x = xv[k];
        float4 gy = f4_scale(gv[k], gs);
        float4 h = x;
        if (!prenorm) {
          if (has_r) x = f4_add(x, rv[k]);
          h = make_float4((x.x - mean[k]) * rstd[k], (x.y - mean[k]) * rstd[k], (x.z - mean[k]) * rstd[k],
                          (x.w - mean[k]) * rstd[k]);
        }
        if (relu) {
          if (h.x * w.x + bb.x <= 0.f) gy.x = 0.f;
          if (h.y * w.y + bb.y <= 0.f) gy.y = 0.f;
          if (h.z * w.z + bb.z <= 0.f) gy.z = 0.f;
          if (h.w * w.w + bb.w <= 0.f) gy.w = 0.f;
        }
        aw = f4_add(aw, f4_mul(gy, h));
        ab = f4_add(ab, gy);
      }
    }
  }
  if (sl > 0) {
    red[0][sl - 1][col] = aw;
    red[1][sl - 1][col] = ab;
  }
  __syncthreads();
  if (sl == 0 && active) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      aw = f4_add(aw, red[0][k][col]);
      ab = f4_add(ab, red[1][k][col]);
    }
    float* pw = dln_w + (int64_t)i * 4;
    float* pb = dln_b + (int64_t)i * 4;
    atomicAdd(pw + 0, aw.x); atomicAdd(pw + 1, aw.y); atomicAdd(pw + 2, aw.z); atomicAdd(pw + 3, aw.w);
    atomicAdd(pb + 0, ab.x); atomicAdd(pb + 1, ab.y); atomicAdd(pb + 2, ab.z); atomicAdd(pb + 3, ab.w);
  }
}

// blockIdx.z selects the problem: every LayerNorm of a backward pass (K7, the K6 of each step
// node, the attention LNs) in ONE launch at the end of the pass instead of five ~4.5 us ones.
__global__ __launch_bounds__(256) void ln_affine_bwd_k(LnAffineBatch B) {
  __shared__ float4 red[2][3][64];
  const LnAffineProb& P = B.p[blockIdx.z];
  if ((int)blockIdx.x * 64 >= P.d4) return;              // block-uniform: this problem is narrower
  ln_affine_body(P, B.b, B.chunk, red);
}

// Partial sums left by the head's backward (head.hip): out[e] = sum_c part[c][e], float4 stream.
constexpr int kMaxSums = 2;
struct SumPack {
  const float* part[kMaxSums];
  float* out[kMaxSums];
  long long n4[kMaxSums];
  int n_chunk[kMaxSums];
  int n;
  int reps;                      // z-slices (of gridDim.x * gridDim.y workgroups) per sum
};

// The two launches that end a fused cell's backward, as one: blockIdx.z < B.n are the LayerNorm
// affine problems above, the z = B.n slice walks the rows of the architecture tensors (four rows
// per workgroup, one wavefront each) for the row-softmax backward.  Independent work.
__global__ __launch_bounds__(256) void backward_epilogue_k(LnAffineBatch B, ArchPack A, int arch_rows, SumPack S) {
  __shared__ float4 red[2][3][64];
  if ((int)blockIdx.z > B.n) {                                   // z = B.n + 1 + i * reps + r: slice r of the i-th partial sum
    const int k = (int)blockIdx.z - B.n - 1;
    const int i = k / S.reps, rep = k - i * S.reps;
    const long long per = (long long)gridDim.x * gridDim.y;
    const long long n4 = S.n4[i], wg = rep * per + (long long)blockIdx.y * gridDim.x + blockIdx.x;
    const float* __restrict__ part = S.part[i];
    float* __restrict__ out = S.out[i];
    const int nc = S.n_chunk[i];
    const long long step = (long long)S.reps * per * 256;
    // an element's chunks are requested four at a time (clamped, masked) and added in chunk order: one round trip per
    // element at n_chunk <= 4 instead of one per chunk
    for (long long e = wg * 256 + threadIdx.x; e < n4; e += step) {
      float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
      for (int c0 = 0; c0 < nc; c0 += 4) {
        float4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = ld4(part + 4 * (e + (long long)(c0 + k < nc ? c0 + k : nc - 1) * n4));
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int k = 0; k < 4; ++k) pin4(v[k]);
#pragma unroll
        for (int k = 0; k < 4; ++k)
          if (c0 + k < nc) t = (c0 + k == 0) ? v[k] : f4_add(t, v[k]);
      }
      st4_wtg<3>(out + 4 * e, t);
    }
    return;
  }
  if ((int)blockIdx.z == B.n) {
    // (the wave index through readfirstlane: the row is wave-uniform, arch_body.hpp)
    const int r = ((int)blockIdx.y * (int)gridDim.x + (int)blockIdx.x) * 4 +
                  __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (r < arch_rows) arch_softmax_bwd_row(A, r, threadIdx.x & 63);
    return;
  }
  const LnAffineProb& P = B.p[blockIdx.z];
  if ((int)blockIdx.x * 64 >= P.d4) return;
  ln_affine_body(P, B.b, B.chunk, red);
}

}  // namespace

extern "C" int bmnas_cat_ln_fwd(const float* const* srcs, int n_src, const float* resid,
                                const float* ln_w, const float* ln_b, float* out, float* stats,
                                int b, int C, int L, int relu, float* out_sums, void* stream) {
  if (!srcs || !ln_w || !ln_b || !out || !stats || n_src < 1 || b < 0 || C < 1 || L < 1)
    return BMNAS_E_ARG;
  if (n_src > 4) return BMNAS_E_LIMIT;
  if (resid && n_src != 1) return BMNAS_E_ARG;
  if ((C * L) % 4 != 0) return BMNAS_E_SHAPE;
  if (b == 0) return 0;
  LnSrc s{};
  if (int e = fill_ptrs(s.p, srcs, n_src)) return e;
  const int cl4 = C * L / 4, d4 = cl4 * n_src;
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_ln<1, 2, 3, 4, 8, 16>(ln_launch_shape(b, d4), [&](auto V, auto BS) {
        hipLaunchKernelGGL((cat_ln_fwd_k<decltype(V)::value, decltype(BS)::value>), dim3(b), dim3(decltype(BS)::value),
                           0, st, s, resid, ln_w, ln_b, out, stats, cl4, d4, relu, out_sums);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_cat_ln_bwd(const float* g, const float* const* srcs, int n_src,
                                const float* resid, const float* ln_w, const float* ln_b,
                                const float* stats, float* const* dsrcs, float* dresid,
                                uint32_t accumulate_mask, float* dln_w, float* dln_b, int b, int C,
                                int L, int relu, float* scrub, int64_t scrub_n, void* stream) {
  if (!g || !srcs || !ln_w || !ln_b || !stats || !dsrcs || n_src < 1 || b < 0 || C < 1 || L < 1)
    return BMNAS_E_ARG;
  if (scrub_n < 0 || (scrub_n > 0 && !scrub) || scrub_n % 4) return BMNAS_E_ARG;
  if ((dln_w == nullptr) != (dln_b == nullptr)) return BMNAS_E_ARG;
  if (n_src > 4) return BMNAS_E_LIMIT;
  if (resid && n_src != 1) return BMNAS_E_ARG;
  if ((C * L) % 4 != 0) return BMNAS_E_SHAPE;
  if (b == 0) return 0;
  LnSrc s{};
  LnDst d{};
  if (int e = fill_ptrs(s.p, srcs, n_src)) return e;
  fill_ptrs_out(d.p, dsrcs, n_src);
  const int cl4 = C * L / 4, d4 = cl4 * n_src;
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_ln<1, 2, 3, 4, 8, 16>(ln_launch_shape(b, d4), [&](auto V, auto BS) {
        hipLaunchKernelGGL((cat_ln_bwd_k<decltype(V)::value, decltype(BS)::value>), dim3(b), dim3(decltype(BS)::value),
                           0, st, g, s, resid, ln_w, ln_b, stats, d, dresid, accumulate_mask, dln_w, dln_b, cl4, d4,
                           relu, scrub, scrub_n / 4);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

namespace {
int fill_prob(LnAffineProb& P, const float* g, const float* gscale, const float* const* srcs, int n_src,
              const float* resid, const float* ln_w, const float* ln_b, const float* stats, float* dln_w,
              float* dln_b, int C, int L, int relu, int prenorm) {
  if (!g || !srcs || !dln_w || !dln_b || n_src < 1 || C < 1 || L < 1) return BMNAS_E_ARG;
  if (!prenorm && !stats) return BMNAS_E_ARG;
  if (relu && (!ln_w || !ln_b)) return BMNAS_E_ARG;
  if (n_src > 4) return BMNAS_E_LIMIT;
  if (resid && n_src != 1) return BMNAS_E_ARG;
  if ((C * L) % 4 != 0) return BMNAS_E_SHAPE;
  P = LnAffineProb{};
  if (int e = fill_ptrs(P.srcs.p, srcs, n_src)) return e;
  P.g = g; P.gscale = gscale; P.resid = resid; P.ln_w = ln_w; P.ln_b = ln_b; P.stats = stats;
  P.dln_w = dln_w; P.dln_b = dln_b;
  P.cl4 = C * L / 4; P.d4 = P.cl4 * n_src; P.relu = relu; P.prenorm = prenorm;
  return 0;
}

// the n problems of the multi-problem entries, element i of every list (a null list: absent for all)
int fill_probs(LnAffineBatch& B, int n_prob, const float* const* g, const float* const* gscale,
               const float* const* const* srcs, const int* n_src, const float* const* resid,
               const float* const* ln_w, const float* const* ln_b, const float* const* stats, float* const* dln_w,
               float* const* dln_b, const int* C, int L, const int* relu, const int* prenorm) {
  for (int i = 0; i < n_prob; ++i)
    if (int e = fill_prob(B.p[i], g[i], gscale ? gscale[i] : nullptr, srcs[i], n_src[i],
                          resid ? resid[i] : nullptr, ln_w ? ln_w[i] : nullptr, ln_b ? ln_b[i] : nullptr,
                          stats ? stats[i] : nullptr, dln_w[i], dln_b[i], C[i], L, relu[i], prenorm[i]))
      return e;
  return 0;
}

// samples per workgroup of the LayerNorm affine reductions: 16 up to 256 samples (smaller chunks = more
// atomics: measured slower, 6.5 vs 4.6 us at b = 128), then b / 16 — every chunk ends in one atomic per
// element, and at b = 1024 sixteen-sample chunks meant 1.5 M atomics per pass
// Deterministic mode (bmnas_set_deterministic): ONE chunk — every element receives a single add onto its zero-filled
// slot, so the result does not depend on the order workgroups finish in.
int g_ln_deterministic = 0;
inline int ln_affine_chunk(int b) {
  if (g_ln_deterministic) return b;
  return b <= 256 ? 16 : (b + 15) / 16;
}

// sets B.chunk; grid of the B.n affine problems: 64 float4 columns x one sample chunk per workgroup, z = problem
dim3 ln_affine_grid(LnAffineBatch& B) {
  B.chunk = ln_affine_chunk(B.b);
  int maxd4 = 0;
  for (int i = 0; i < B.n; ++i) maxd4 = B.p[i].d4 > maxd4 ? B.p[i].d4 : maxd4;
  return dim3((maxd4 + 63) / 64, (B.b + B.chunk - 1) / B.chunk, B.n);
}

int launch_ln_affine(LnAffineBatch& B, hipStream_t st) {
  const dim3 grid = ln_affine_grid(B);
  hipLaunchKernelGGL(ln_affine_bwd_k, grid, dim3(256), 0, st, B);
  BMNAS_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int bmnas_ln_affine_bwd(const float* g, const float* gscale, const float* const* srcs,
                                   int n_src, const float* resid, const float* ln_w,
                                   const float* ln_b, const float* stats, float* dln_w, float* dln_b,
                                   int b, int C, int L, int relu, int prenorm, void* stream) {
  if (b < 0) return BMNAS_E_ARG;
  LnAffineBatch B{};
  if (int e = fill_prob(B.p[0], g, gscale, srcs, n_src, resid, ln_w, ln_b, stats, dln_w, dln_b, C, L, relu,
                        prenorm))
    return e;
  if (b == 0) return 0;
  B.n = 1;
  B.b = b;
  return launch_ln_affine(B, (hipStream_t)stream);
}

extern "C" int bmnas_ln_affine_bwd_multi(int n_prob, const float* const* g, const float* const* gscale,
                                         const float* const* const* srcs, const int* n_src,
                                         const float* const* resid, const float* const* ln_w,
                                         const float* const* ln_b, const float* const* stats,
                                         float* const* dln_w, float* const* dln_b, int b, const int* C,
                                         int L, const int* relu, const int* prenorm, void* stream) {
  if (n_prob < 1 || b < 0 || !g || !srcs || !n_src || !dln_w || !dln_b || !C || !relu || !prenorm)
    return BMNAS_E_ARG;
  if (n_prob > kMaxLnProbs) return BMNAS_E_LIMIT;
  LnAffineBatch B{};
  if (int e = fill_probs(B, n_prob, g, gscale, srcs, n_src, resid, ln_w, ln_b, stats, dln_w, dln_b, C, L, relu,
                         prenorm))
    return e;
  if (b == 0) return 0;
  B.n = n_prob;
  B.b = b;
  return launch_ln_affine(B, (hipStream_t)stream);
}

extern "C" int bmnas_backward_epilogue(int n_prob, const float* const* g, const float* const* gscale,
                                       const float* const* const* srcs, const int* n_src,
                                       const float* const* resid, const float* const* ln_w,
                                       const float* const* ln_b, const float* const* stats,
                                       float* const* dln_w, float* const* dln_b, int b, const int* C,
                                       int L, const int* relu, const int* prenorm,
                                       const float* const* arch_w, const float* const* arch_dw,
                                       float* const* arch_out, const int* arch_rows, const int* arch_cols,
                                       int n_arch, int n_shards, int64_t shard_stride, int n_sums,
                                       const float* const* sum_part, float* const* sum_out,
                                       const int* sum_chunks, const int64_t* sum_n, void* stream) {
  if (n_prob < 1 || b < 1 || !g || !srcs || !n_src || !dln_w || !dln_b || !C || !relu || !prenorm)
    return BMNAS_E_ARG;
  if (n_prob > kMaxLnProbs || n_sums > kMaxSums) return BMNAS_E_LIMIT;
  if (n_sums < 0 || (n_sums > 0 && (!sum_part || !sum_out || !sum_chunks || !sum_n))) return BMNAS_E_ARG;
  SumPack S{};
  for (int i = 0; i < n_sums; ++i) {
    if (!sum_part[i] || !sum_out[i] || sum_chunks[i] < 1 || sum_n[i] < 0 || sum_n[i] % 4) return BMNAS_E_ARG;
    S.part[i] = sum_part[i]; S.out[i] = sum_out[i]; S.n_chunk[i] = sum_chunks[i]; S.n4[i] = sum_n[i] / 4;
  }
  S.n = n_sums;
  LnAffineBatch B{};
  if (int e = fill_probs(B, n_prob, g, gscale, srcs, n_src, resid, ln_w, ln_b, stats, dln_w, dln_b, C, L, relu,
                         prenorm))
    return e;
  ArchPack A{};
  // (n_arch == 0: no architecture tensors — the per-op path's end-of-backward launch: affine reductions + chunk sums)
  const int total = n_arch > 0 ? fill_arch_pack(A, arch_w, arch_dw, arch_out, arch_rows, arch_cols, n_arch, 1, n_shards,
                                                shard_stride)
                               : 0;
  if (total < 0) return total;
  B.n = n_prob;
  B.b = b;
  dim3 grid = ln_affine_grid(B);                      // (z: set below, once the partial sums' slices are counted)
  // the arch slice needs one wavefront per row, four per workgroup (LayerNorm workgroups past a
  // problem's width return at once, so widening the grid for tiny shapes costs nothing)
  const unsigned need_x = (unsigned)((total + 4 * (int)grid.y - 1) / (4 * (int)grid.y));
  if (grid.x < need_x) grid.x = need_x;
  // ... and a partial sum gets one workgroup per 256 float4 of its output, up to 256 workgroups: on NTU / Ego's narrow
  // LayerNorm grids (4 column blocks x 3-4 sample chunks) the head's (O + 3) x D partials were walked by 12-16
  // workgroups, 8-14 rounds of n_chunk dependent loads each — the longest chain of the launch (Ego b48: 11.3 us)
  // (as S.reps z-slices per sum rather than a wider grid.x: that would multiply the LayerNorm slices' idle workgroups
  // too — measured +0.9 us at NTU b64)
  long long max_n4 = 0;
  for (int i = 0; i < n_sums; ++i) max_n4 = S.n4[i] > max_n4 ? S.n4[i] : max_n4;
  long long want_wg = (max_n4 + 255) / 256;
  if (want_wg > 256) want_wg = 256;
  const long long per = (long long)grid.x * grid.y;
  S.reps = (int)((want_wg + per - 1) / per);
  if (S.reps < 1) S.reps = 1;
  grid.z = (unsigned)(B.n + 1 + n_sums * S.reps);
  hipLaunchKernelGGL(backward_epilogue_k, grid, dim3(256), 0, (hipStream_t)stream, B, A, total, S);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

// BMNAS_DETERMINISTIC (bmnas.cell.DETERMINISTIC): run-to-run bit-identical results.  The host library keeps one
// flag per source that has a choice to make (no relocatable device code / shared globals in this build): here the
// LayerNorm-affine reductions take one sample chunk, in conv1x1.hip the weight-gradient tiles walk the whole batch.
extern "C" int bmnas_ln_set_deterministic(int on) {
  g_ln_deterministic = on ? 1 : 0;
  return 0;
}
