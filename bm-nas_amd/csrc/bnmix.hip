// BatchNorm bookkeeping + the elementwise halves of K2/K4/K5: BN-apply + GLU / ReLU +
// dropout + gamma-weighted NodeMixedOp combine, and their backward (phase A: activation
// backward + per-channel batch reductions; phase B: BatchNorm input gradient).
// All HBM-streaming float4 kernels.  In the backward a thread owns one (channel, l4) slot
// and walks a chunk of samples, so the per-channel sums stay in registers and cost one
// atomic per channel per workgroup.
#include "common.hpp"
#include "../../include/bmnas_hip.h"
#include "arch_body.hpp"
#include "bn_fin.hpp"
#include "ln_sample.hpp"
#include "mix_common.hpp"
#include "mish.hpp"
#include <algorithm>
#include <cstdlib>

namespace {

// bn_finalize_k in cumulative-momentum mode leaves the counters alone — every channel's wavefront reads counter 0 as
// the launch found it, in whatever order the workgroups run — and this launch behind it increments them
__global__ void bn_count_k(int64_t* nbt, int n_nbt) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n_nbt) nbt[i] += 1;
}

__global__ __launch_bounds__(256) void bn_finalize_k(const float* __restrict__ part, int n_part,
                                                     int b, int L, int M,
                                                     const float* __restrict__ bn_w,
                                                     const float* __restrict__ bn_b,
                                                     float* running_mean, float* running_var,
                                                     int64_t* nbt, int n_nbt, int training,
                                                     float mom, int cum, float* __restrict__ chan) {
  // one wavefront per channel: lanes stride over that channel's partials (part[m][p][2]),
  // Chan's parallel-variance combine, two wave reductions
  const int lane = threadIdx.x & 63;
  const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  float mean, rstd;
  if (training) {
    const int N = b * L;
    const float2* pm = reinterpret_cast<const float2*>(part) + (int64_t)m * n_part;
    // the first kKeep partials of a lane stay in registers for the second pass (batch <= 4096
    // columns per lane-stride: one memory round trip instead of two); the rest are re-read
    constexpr int kKeep = 4;
    float2 keep[kKeep];
    float tot = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const int p = lane + 64 * k;
      keep[k] = (p < n_part) ? pm[p] : make_float2(0.f, 0.f);
      tot += keep[k].x;
    }
    for (int p = lane + 64 * kKeep; p < n_part; p += 64) tot += pm[p].x;
    tot = wave_sum(tot);
    mean = tot / (float)N;
    float m2 = 0.f;
#pragma unroll
    for (int k = 0; k < kKeep; ++k) {
      const int p = lane + 64 * k;
      if (p < n_part) {
        int cnt = N - 16 * p;
        cnt = cnt > 16 ? 16 : cnt;
        const float d = keep[k].x / (float)cnt - mean;
        m2 += keep[k].y + (float)cnt * d * d;
      }
    }
    for (int p = lane + 64 * kKeep; p < n_part; p += 64) {
      int cnt = N - 16 * p;
      cnt = cnt > 16 ? 16 : cnt;
      const float2 v = pm[p];
      const float d = v.x / (float)cnt - mean;
      m2 += v.y + (float)cnt * d * d;
    }
    m2 = wave_sum(m2);
    const float var = m2 / (float)N;
    rstd = 1.f / sqrtf(var + kEpsBn);
    if (lane == 0) {
      if (running_mean != nullptr) {
        if (cum) mom = 1.f / (float)(nbt[0] + 1);
        running_mean[m] = (1.f - mom) * running_mean[m] + mom * mean;
        const float unbiased = m2 / (float)(N - 1);
        running_var[m] = (1.f - mom) * running_var[m] + mom * unbiased;
      }
      if (!cum && m < n_nbt && nbt != nullptr) nbt[m] += 1;
    }
  } else {
    mean = running_mean[m];
    rstd = 1.f / sqrtf(running_var[m] + kEpsBn);
  }
  if (lane == 0) {
    const float scale = bn_w[m] * rstd;
    chan[m] = mean;
    chan[M + m] = rstd;
    chan[2 * M + m] = scale;
    chan[3 * M + m] = bn_b[m] - mean * scale;
  }
}


// The NEXT inner step's mixed sum riding in this step's mix kernel (NodeCell, node_search.py:54):
// z_next = sum_{j < n} w_j prev_j + w_n s, with s the state this kernel produces — one launch and one
// read of s fewer per inner step.  Backward: MixNextB (the whole bmnas_mixsum_bwd of that sum).
constexpr int kMixPrev = 5;
struct MixNextF {
  const float* prev[kMixPrev];
  const float* w;            // w[j * ws], j = 0 .. n
  float* z;
  int n, ws;
};
struct MixNextB {
  const float* prev[kMixPrev];
  float* dprev[kMixPrev];    // (=|+= by acc bit j) w_j G; nullable
  const float* w;
  float* dw;                 // dw[j * ws] += <G, prev_j> (j < n), dw[n * ws] += <G, s>; sharded like bmnas_mixsum_bwd
  const float* s;            // the state this step produced (forward output)
  const float* gz;           // G = gz + gz2: gradient of z_next
  const float* gz2;          // nullable
  const float* g_in;         // what other consumers of s already accumulated; nullable
  float* g_out;              // g_in + w_n G: the gradient this kernel (and the attention backward after it) uses
  int64_t dw_stride;
  int n, ws, dw_shards;
  uint32_t acc;
};

// s = g0*(x+y) + g1*p1 + g2*drop(va*sigmoid(vg)) + g3*drop(relu(vf))
template <int NP>
__global__ __launch_bounds__(256) void node_mix_fwd_k(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ p1,
    const float* __restrict__ U, float* __restrict__ chan, BnFin fin, const float* __restrict__ gamma,
    float* __restrict__ out, int b, int C, int L, DropCfg dglu, DropCfg dfc, MixNextF N) {
  extern __shared__ float fin_lds[];
  const int cl4 = C * L / 4, l4n = L / 4, M = 3 * C;
  float* sc = fin_lds;
  float* sh = fin_lds + M;
  const DropRt rglu = drop_begin(dglu), rfc = drop_begin(dfc);
  bn_fin_fill<256>(fin, chan, M, b * L, sc, sh, blockIdx.x == 0);
  const float g0 = gamma[0], g1 = gamma[1], g2 = gamma[2], g3 = gamma[3];
  const int64_t total = (int64_t)b * cl4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int s = (int)(i / cl4);
    const int r = (int)(i - (int64_t)s * cl4);
    const int c = r / l4n;
    const int64_t e = i * 4;
    const int64_t ub = ((int64_t)s * M) * L + (int64_t)r * 4;      // (s, c, l) inside U's first C block
    const float4 va = affine4(ld4(U + ub), sc[c], sh[c]);
    const float4 vg = affine4(ld4(U + ub + (int64_t)C * L), sc[C + c], sh[C + c]);
    const float4 vf = affine4(ld4(U + ub + (int64_t)2 * C * L), sc[2 * C + c], sh[2 * C + c]);
    const float4 m2 = drop_mult4(rglu, (uint64_t)e), m3 = drop_mult4(rfc, (uint64_t)e);
    const float4 xv = ld4(x + e), yv = ld4(y + e), pv = ld4(p1 + e);
    const float4 o = mix_fwd4<kMixAll>(g0, g1, g2, g3, f4_add(xv, yv), pv, va, vg, vf, m2, m3);
    st4_wtg<2>(out + e, o);
    if (NP > 0) {
      float4 z = f4_scale(o, N.w[NP * N.ws]);
#pragma unroll
      for (int j = 0; j < NP; ++j) {
        const float wj = N.w[j * N.ws];
        const float4 pj = ld4(N.prev[j] + e);
        z.x = fmaf(wj, pj.x, z.x); z.y = fmaf(wj, pj.y, z.y); z.z = fmaf(wj, pj.z, z.z); z.w = fmaf(wj, pj.w, z.w);
      }
      st4_wtg<2>(N.z + e, z);
    }
  }
}


// K2 + K6 fused (node_multiplier == 1, last inner step): the gamma-mix result never goes to
// memory on its own — one workgroup per sample forms s, adds the residual X, keeps the sample
// in registers for the two LayerNorm reductions and writes pre = s + X (saved for backward)
// and out = LN(pre).  Saves one launch and 3 T of traffic per step node.
template <int VPT, int BS>
__global__ __launch_bounds__(BS) void node_mix_ln_fwd_k(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ p1,
    const float* __restrict__ U, float* __restrict__ chan, BnFin fin, const float* __restrict__ gamma,
    const float* __restrict__ resid, const float* __restrict__ ln_w, const float* __restrict__ ln_b,
    float* __restrict__ pre, float* __restrict__ out, float* __restrict__ stats, int b, int C, int L,
    DropCfg dglu, DropCfg dfc, float* __restrict__ osum) {
  __shared__ float red[8];
  __shared__ float red6[8 * 6];
  extern __shared__ float fin_lds[];
  const int cl4 = C * L / 4, l4n = L / 4, M = 3 * C;
  const int smp = blockIdx.x;
  float* sc = fin_lds;
  float* sh = fin_lds + M;
  const float g0 = gamma[0], g1 = gamma[1], g2 = gamma[2], g3 = gamma[3];
  const DropRt rglu = drop_begin(dglu), rfc = drop_begin(dfc);
  float4 v[VPT], lw[VPT], lb[VPT];
  // every global load of the sample first (raw conv outputs included), THEN the BatchNorm
  // finalisation (its own memory round trip + a barrier), then the arithmetic: the two latencies
  // overlap instead of adding up
  float4 ua[VPT], ug[VPT], uf[VPT], xv[VPT], yv[VPT], pv[VPT], rv[VPT];
  // (clamped addresses, not `if (r < cl4)` around the loads: the predicated form compiled to branches whose
  // join copied every loaded register — behind s_waitcnt vmcnt(4..0) — BEFORE the BatchNorm finalisation's own
  // loads were issued: two dependent round trips instead of the one this ordering is for)
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r0 = threadIdx.x + k * BS;
    const int r = r0 < cl4 ? r0 : cl4 - 1;
    v[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    lw[k] = ld4(ln_w + (int64_t)r * 4);
    lb[k] = ld4(ln_b + (int64_t)r * 4);
    const int64_t e = ((int64_t)smp * cl4 + r) * 4;
    const int64_t ub = ((int64_t)smp * M) * L + (int64_t)r * 4;
    ua[k] = ld4(U + ub);
    ug[k] = ld4(U + ub + (int64_t)C * L);
    uf[k] = ld4(U + ub + (int64_t)2 * C * L);
    xv[k] = ld4(x + e);
    yv[k] = ld4(y + e);
    pv[k] = ld4(p1 + e);
    rv[k] = ld4(resid + e);
  }
  bn_fin_fill<BS>(fin, chan, M, b * L, sc, sh, blockIdx.x == 0);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    if (r < cl4) {
      const int c = r / l4n;
      const int64_t e = ((int64_t)smp * cl4 + r) * 4;
      const float4 va = affine4(ua[k], sc[c], sh[c]);
      const float4 vg = affine4(ug[k], sc[C + c], sh[C + c]);
      const float4 vf = affine4(uf[k], sc[2 * C + c], sh[2 * C + c]);
      const float4 m2 = drop_mult4(rglu, (uint64_t)e), m3 = drop_mult4(rfc, (uint64_t)e);
      const float4 o = mix_fwd4<kMixAll>(g0, g1, g2, g3, f4_add(xv[k], yv[k]), pv[k], va, vg, vf, m2, m3);
      v[k] = f4_add(o, rv[k]);
      st4_wtg<2>(pre + e, v[k]);
      sum += f4_hsum(v[k]);
    }
  }
  const float inv_d = 1.f / (float)(cl4 * 4);
  const float mean = block_sum_fresh<BS / 64>(sum, red) * inv_d;     // (first use of red: no barrier in front)
  // second pass: the centred second moment and — same reduction round — what the per-sample sums of
  // the OUTPUT o = c * rstd * w + b (c = v - mean) need:  sum o = rstd * S(c w) + S(b),
  // sum o^2 = rstd^2 * S(c^2 w^2) + 2 rstd * S(c w b) + S(b^2)   (for the head's K7 LayerNorm)
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    if (r < cl4) {
      const float4 cdev = make_float4(v[k].x - mean, v[k].y - mean, v[k].z - mean, v[k].w - mean);
      acc[0] += f4_dot(cdev, cdev);
      if (osum != nullptr) {
        const float4 cw = f4_mul(cdev, lw[k]);
        acc[1] += f4_hsum(cw);
        acc[2] += f4_dot(cw, cw);
        acc[3] += f4_dot(cw, lb[k]);
        acc[4] += f4_hsum(lb[k]);
        acc[5] += f4_dot(lb[k], lb[k]);
      }
    }
  }
  if (osum != nullptr) {
    block_sum_lead_fresh<BS / 64, 6>(acc, red6);
  } else {
    acc[0] = block_sum_fresh<BS / 64>(acc[0], red6);        // (red6, not red: threads may still be reading the mean)
  }
  const float var = acc[0] * inv_d;
  const float rstd = 1.f / sqrtf(var + kLnEps);
  if (threadIdx.x == 0) {
    stats[2 * smp] = mean;
    stats[2 * smp + 1] = rstd;
    if (osum != nullptr) {
      osum[2 * smp] = rstd * acc[1] + acc[4];
      osum[2 * smp + 1] = rstd * rstd * acc[2] + 2.f * rstd * acc[3] + acc[5];
    }
  }
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    if (r < cl4) {
      st4_wtg<2>(out + ((int64_t)smp * cl4 + r) * 4, ln_apply4(v[k], mean, rstd, lw[k], lb[k]));
    }
  }
}


template <int NP>
__global__ __launch_bounds__(256) void node_mix_bwd_k(
    const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ y,
    const float* __restrict__ p1, const float* __restrict__ U, const float* __restrict__ chan,
    const float* __restrict__ gamma, float* dgamma, int dg_shards, int64_t dg_stride, float* dx,
    float* dy, uint32_t acc_mask, float* __restrict__ dV, float* bn_grad, int b, int C, int L,
    int chunk, DropCfg dglu, DropCfg dfc, MixNextB N) {
  __shared__ float red16[16];
  __shared__ float redn[4 * (NP + 1)];
  float part[NP + 1], wn[NP + 1];
#pragma unroll
  for (int j = 0; j <= NP; ++j) {
    part[j] = 0.f;
    wn[j] = (NP > 0) ? N.w[j * N.ws] : 0.f;
  }
  __shared__ float csum[3][6][64];
  const int cl4 = C * L / 4, l4n = L / 4, M = 3 * C;
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;   // 64 slots x 4 sample lanes
  const int r = blockIdx.x * 64 + col;               // float4 slot inside one sample's (C, L) tile
  const bool active = r < cl4;
  const int c = active ? r / l4n : 0;
  const float g0 = gamma[0], g2 = gamma[2], g3 = gamma[3];
  const DropRt rglu = drop_begin(dglu), rfc = drop_begin(dfc);
  const ChanBn<3> bn = chan_load<3>(chan, M, C, c);
  float dgam[4] = {0.f, 0.f, 0.f, 0.f};
  float sw[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
  const int s_beg = blockIdx.y * chunk;
  int s_end = s_beg + chunk;
  if (s_end > b) s_end = b;
  if (active) {
    for (int s = s_beg + sl; s < s_end; s += 4) {
      const int64_t e = ((int64_t)s * cl4 + r) * 4;
      const int64_t ub = ((int64_t)s * M) * L + (int64_t)r * 4;
      const float4 ua = ld4(U + ub), ug = ld4(U + ub + (int64_t)C * L), uf = ld4(U + ub + (int64_t)2 * C * L);
      float4 gv;
      if (NP > 0) {
        // the backward of the next step's mixed sum first: it completes this step's own gradient
        float4 G = ld4(N.gz + e);
        if (N.gz2 != nullptr) G = f4_add(G, ld4(N.gz2 + e));
        gv = f4_scale(G, wn[NP]);
        if (N.g_in != nullptr) gv = f4_add(gv, ld4(N.g_in + e));
        st4_wtg<2>(N.g_out + e, gv);
        part[NP] += f4_dot(G, ld4(N.s + e));
#pragma unroll
        for (int j = 0; j < NP; ++j) {                     // in order: destinations may alias each other
          part[j] += f4_dot(G, ld4(N.prev[j] + e));
          float* d = N.dprev[j];
          if (d == nullptr) continue;
          float4 rr = f4_scale(G, wn[j]);
          if (N.acc & (1u << j)) rr = f4_add(rr, ld4(d + e));
          st4_wtg<2>(d + e, rr);
        }
      } else {
        gv = ld4(g + e);
      }
      const float4 xv = ld4(x + e), yv = ld4(y + e), pv = ld4(p1 + e);
      const float4 m2 = drop_mult4(rglu, (uint64_t)e), m3 = drop_mult4(rfc, (uint64_t)e);
      float4 da, dg, df;
      mix_bwd4<kMixAll>(g2, g3, gv, f4_add(xv, yv), pv, ua, ug, uf, m2, m3, bn, dgam, da, dg, df, sw, sb);
      st4_wtg<2>(dV + ub, da);
      st4_wtg<2>(dV + ub + (int64_t)C * L, dg);
      st4_wtg<2>(dV + ub + (int64_t)2 * C * L, df);
      mix_dxy_store([](float* p, float4 v) { st4_wtg<2>(p, v); }, dx, dy, e, gv, g0, acc_mask);
    }
  }
  // per-channel batch sums -> BatchNorm affine gradients: reduce over the l4 lanes of a
  // channel row (shuffles), over the 4 sample lanes (LDS), then one atomic per channel
  float cs[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    cs[k] = row_sum(sw[k], l4n);
    cs[3 + k] = row_sum(sb[k], l4n);
  }
  if (sl > 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) csum[sl - 1][k][col] = cs[k];
  }
  // The four dgamma sums (and the next step's mixed-sum weight gradients) meet in LDS behind the SAME barrier as the
  // BatchNorm column sums: a block_sum_lead each after them was four more barriers (node_mix_lnp_bwd_k: 9.2 -> 8.4 us).
  // Every workgroup adds into the same few scalars: same-address atomics serialise (~25 ns each), so they are spread
  // over dg_shards copies (summed by the arch-softmax backward).
#pragma unroll
  for (int q = 0; q < 4; ++q) dgam[q] = wave_sum(dgam[q]);
  if (NP > 0) {
#pragma unroll
    for (int j = 0; j <= NP; ++j) part[j] = wave_sum(part[j]);
  }
  if (col == 0) {
#pragma unroll
    for (int q = 0; q < 4; ++q) red16[q * 4 + sl] = dgam[q];
    if (NP > 0) {
#pragma unroll
      for (int j = 0; j <= NP; ++j) redn[j * 4 + sl] = part[j];
    }
  }
  __syncthreads();
  if (sl == 0 && active && (r % l4n) == 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) cs[k] += csum[0][k][col] + csum[1][k][col] + csum[2][k][col];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      atomicAdd(bn_grad + k * C + c, cs[k]);
      atomicAdd(bn_grad + M + k * C + c, cs[3 + k]);
    }
  }
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x >= 64 && threadIdx.x < 68 && dgamma != nullptr) {      // (wave 1: wave 0's lanes are busy above)
    const int q = threadIdx.x - 64;
    atomicAdd(dgamma + (int64_t)(wg % dg_shards) * dg_stride + q,
              ((red16[q * 4] + red16[q * 4 + 1]) + red16[q * 4 + 2]) + red16[q * 4 + 3]);
  }
  if (NP > 0 && threadIdx.x >= 128 && (int)threadIdx.x <= 128 + NP) {
    const int j = threadIdx.x - 128;
    atomicAdd(N.dw + (int64_t)(wg % N.dw_shards) * N.dw_stride + j * N.ws,
              ((redn[j * 4] + redn[j * 4 + 1]) + redn[j * 4 + 2]) + redn[j * 4 + 3]);
  }
}


// K6 backward + K2 backward in ONE launch (node_multiplier == 1, small batches): the LayerNorm input
// gradient of the node output never makes a round trip of its own.  TWO workgroups per sample so that
// 128 samples still cover 256 CUs: both reduce the sample's two LayerNorm sums (the 24 KB of a sample's
// gy / pre-norm rows are read twice — against a 5 us launch), then each takes one half of the sample's
// channels through LayerNorm backward -> gamma-mix backward (the block of mix_bwd4, mix_terms.hpp).
// A thread's element k of the first phase (k < VPT2) IS its element of the second phase: half h
// starts its walk over the sample at its own half.  BatchNorm reductions: one atomic pair per
// channel per sample (as bn_relu_ln_bwd_k), which is why the launcher keeps this to b <= 128.
template <int VPT1, int VPT2, int BS>
__global__ __launch_bounds__(BS) void node_mix_ln_bwd_k(
    const float* __restrict__ gy, const float* __restrict__ pre, const float* __restrict__ ln_w,
    const float* __restrict__ stats, float* __restrict__ gbuf, float* dresid, int acc_resid,
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ p1,
    const float* __restrict__ U, const float* __restrict__ chan, const float* __restrict__ gamma,
    float* dgamma, int dg_shards, int64_t dg_stride, float* dx, float* dy, uint32_t acc_mask,
    float* __restrict__ dV, float* bn_grad, int b, int C, int L, DropCfg dglu, DropCfg dfc, int probe) {
  constexpr int NW = BS / 64;
  __shared__ float red2[NW * 2];
  __shared__ float red4[NW * 4];
  const int cl4 = C * L / 4, l4n = L / 4, M = 3 * C, h4 = cl4 / 2;
  const int smp = blockIdx.x >> 1, half = blockIdx.x & 1;
  const DropRt rglu = drop_begin(dglu), rfc = drop_begin(dfc);
  // second-phase operands first: they do not depend on the sums
  float4 ua[VPT2], ug[VPT2], uf[VPT2], xv[VPT2], yv[VPT2], pv[VPT2], oldr[VPT2], oldx[VPT2], oldy[VPT2];
  ChanBn<3> bn[VPT2];
#pragma unroll
  for (int k = 0; k < VPT2; ++k) {
    const int idx = threadIdx.x + k * BS;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    ua[k] = ug[k] = uf[k] = xv[k] = yv[k] = pv[k] = oldr[k] = oldx[k] = oldy[k] = zero;
    {                                                    // clamped addresses, no predicate around the loads
      const int r = half * h4 + (idx < h4 ? idx : h4 - 1);
      const int c = r / l4n;
      const int64_t e = ((int64_t)smp * cl4 + r) * 4;
      const int64_t ub = ((int64_t)smp * M) * L + (int64_t)r * 4;
      ua[k] = ld4(U + ub);
      ug[k] = ld4(U + ub + (int64_t)C * L);
      uf[k] = ld4(U + ub + (int64_t)2 * C * L);
      xv[k] = ld4(x + e);
      yv[k] = ld4(y + e);                                 // (x == y: an L1 hit — `same ? xv : load` was a wait + copy)
      pv[k] = ld4(p1 + e);
      if (acc_resid) oldr[k] = ld4(dresid + e);
      if (dx != nullptr && (acc_mask & 1u)) oldx[k] = ld4(dx + e);
      if (dy != nullptr && (acc_mask & 2u)) oldy[k] = ld4(dy + e);
      bn[k] = chan_load<3>(chan, M, C, c);
    }
  }
  const float g0 = gamma[0], g2 = gamma[2], g3 = gamma[3];
  const float mean = stats[2 * smp], rstd = stats[2 * smp + 1];
  // first phase: the whole sample's sum(gy w) and sum(gy w xhat)
  float4 xh[VPT1], dxh[VPT1];
  float s12[2] = {0.f, 0.f};
  // (all loads of the phase, then its arithmetic: interleaved per k, the first k's use of `mean` drained every
  // load in flight before the second k's loads were issued)
#pragma unroll
  for (int k = 0; k < VPT1; ++k) {
    const int idx = threadIdx.x + k * BS;
    int r = half * h4 + (idx < cl4 ? idx : cl4 - 1);
    r = r >= cl4 ? r - cl4 : r;
    const int64_t e = ((int64_t)smp * cl4 + r) * 4;
    xh[k] = ld4(pre + e);
    dxh[k] = f4_mul(ld4(gy + e), ld4(ln_w + (int64_t)r * 4));
  }
#pragma unroll
  for (int k = 0; k < VPT1; ++k) {
    const int idx = threadIdx.x + k * BS;
    const bool on = idx < cl4 && !((probe & 2) && idx >= h4);
    xh[k] = ln_xhat4(xh[k], mean, rstd);
    s12[0] += on ? f4_hsum(dxh[k]) : 0.f;
    s12[1] += on ? f4_dot(dxh[k], xh[k]) : 0.f;
  }
  block_sum_n<NW, 2>(s12, red2);
  const float inv_d = 1.f / (float)(cl4 * 4);
  const float m1 = s12[0] * inv_d, m2 = s12[1] * inv_d;
  // second phase
  float dgam[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < VPT2; ++k) {
    const int idx = threadIdx.x + k * BS;
    const bool act = idx < h4;
    const int r = half * h4 + (act ? idx : 0);
    const int c = r / l4n;
    float sw[3] = {0.f, 0.f, 0.f}, sb[3] = {0.f, 0.f, 0.f};
    if (act) {
      const int64_t e = ((int64_t)smp * cl4 + r) * 4;
      const int64_t ub = ((int64_t)smp * M) * L + (int64_t)r * 4;
      const float4 gv = ln_dx4(dxh[k], xh[k], m1, m2, rstd);
      if (gbuf != nullptr) st4_wtg<2>(gbuf + e, gv);
      if (dresid != nullptr) st4_wtg<2>(dresid + e, f4_add(gv, oldr[k]));
      const float4 m2d = drop_mult4(rglu, (uint64_t)e), m3d = drop_mult4(rfc, (uint64_t)e);
      const float gq[4] = {gv.x, gv.y, gv.z, gv.w};
      const float uaq[4] = {ua[k].x, ua[k].y, ua[k].z, ua[k].w}, ugq[4] = {ug[k].x, ug[k].y, ug[k].z, ug[k].w},
                  ufq[4] = {uf[k].x, uf[k].y, uf[k].z, uf[k].w};
      const float xq[4] = {xv[k].x + yv[k].x, xv[k].y + yv[k].y, xv[k].z + yv[k].z, xv[k].w + yv[k].w};
      const float pq[4] = {pv[k].x, pv[k].y, pv[k].z, pv[k].w};
      const float m2q[4] = {m2d.x, m2d.y, m2d.z, m2d.w}, m3q[4] = {m3d.x, m3d.y, m3d.z, m3d.w};
      float da[4], dg[4], df[4];
      // mix_bwd4<kMixAll> (mix_terms.hpp) written out: through the call <1,1,512> / <2,1,512> need 98 VGPRs, not 94 (occupancy 5 -> 4)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float va = fmaf(uaq[t], bn[k].sc[0], bn[k].sh[0]), vg = fmaf(ugq[t], bn[k].sc[1], bn[k].sh[1]),
                    vf = fmaf(ufq[t], bn[k].sc[2], bn[k].sh[2]);
        const float sg = sigmoidf(vg);
        dgam[0] += gq[t] * xq[t];
        dgam[1] += gq[t] * pq[t];
        dgam[2] += gq[t] * (va * sg * m2q[t]);
        dgam[3] += gq[t] * (fmaxf(vf, 0.f) * m3q[t]);
        const float gm2 = g2 * gq[t] * m2q[t];
        da[t] = gm2 * sg;
        dg[t] = gm2 * va * sg * (1.f - sg);
        df[t] = (vf > 0.f) ? g3 * gq[t] * m3q[t] : 0.f;
        sw[0] += da[t] * (uaq[t] - bn[k].mu[0]) * bn[k].rs[0];
        sw[1] += dg[t] * (ugq[t] - bn[k].mu[1]) * bn[k].rs[1];
        sw[2] += df[t] * (ufq[t] - bn[k].mu[2]) * bn[k].rs[2];
        sb[0] += da[t]; sb[1] += dg[t]; sb[2] += df[t];
      }
      st4_wtg<2>(dV + ub, make_float4(da[0], da[1], da[2], da[3]));
      st4_wtg<2>(dV + ub + (int64_t)C * L, make_float4(dg[0], dg[1], dg[2], dg[3]));
      st4_wtg<2>(dV + ub + (int64_t)2 * C * L, make_float4(df[0], df[1], df[2], df[3]));
      mix_dxy_store([](float* p, float4 v) { st4_wtg<2>(p, v); }, dx, dy, e, gv, g0, oldx[k], oldy[k]);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      sw[q] = row_sum(sw[q], l4n);
      sb[q] = row_sum(sb[q], l4n);
    }
    if (act && (r % l4n) == 0 && !(probe & 1)) {
#pragma unroll
      for (int q = 0; q < 3; ++q) {
        atomicAdd(bn_grad + q * C + c, sw[q]);
        atomicAdd(bn_grad + M + q * C + c, sb[q]);
      }
    }
  }
  block_sum_lead<NW, 4>(dgam, red4);
  if (threadIdx.x == 0 && dgamma != nullptr && !(probe & 4)) {
    float* p = dgamma + (int64_t)(blockIdx.x % dg_shards) * dg_stride;
#pragma unroll
    for (int q = 0; q < 4; ++q) atomicAdd(p + q, dgam[q]);
  }
}


// standalone LinearGLU tail: out = drop(va * sigmoid(vg)), U is (b, 2C, L) = [a | gate]
// (round 5: the BatchNorm statistics are finalised HERE when `fin` says so — as in bn_relu_fwd_k and every consumer of
// the search path — instead of by a bn_finalize launch in front: one launch less per LinearGLU of a found network)
__global__ __launch_bounds__(256) void bn_glu_fwd_k(const float* __restrict__ U,
                                                    float* __restrict__ chan, BnFin fin,
                                                    float* __restrict__ out, int b, int C, int L,
                                                    DropCfg d) {
  extern __shared__ float fin_lds[];
  const DropRt dr = drop_begin(d);
  const int cl4 = C * L / 4, l4n = L / 4, M = 2 * C;
  float* sc = fin_lds;
  float* sh = fin_lds + M;
  bn_fin_fill<256>(fin, chan, M, b * L, sc, sh, blockIdx.x == 0);
  const int64_t total = (int64_t)b * cl4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int s = (int)(i / cl4);
    const int r = (int)(i - (int64_t)s * cl4);
    const int c = r / l4n;
    const int64_t ub = ((int64_t)s * M) * L + (int64_t)r * 4;
    const float4 va = affine4(ld4(U + ub), sc[c], sh[c]);
    const float4 vg = affine4(ld4(U + ub + (int64_t)C * L), sc[C + c], sh[C + c]);
    const float4 m = drop_mult4(dr, (uint64_t)(i * 4));
    st4_wtg<2>(out + i * 4, make_float4(glu_term(va.x, sigmoidf(vg.x), m.x), glu_term(va.y, sigmoidf(vg.y), m.y),
                                        glu_term(va.z, sigmoidf(vg.z), m.z), glu_term(va.w, sigmoidf(vg.w), m.w)));
  }
}

__global__ __launch_bounds__(256) void bn_glu_bwd_k(const float* __restrict__ g,
                                                    const float* __restrict__ U,
                                                    const float* __restrict__ chan,
                                                    float* __restrict__ dV, float* bn_grad, int b,
                                                    int C, int L, int chunk, DropCfg d) {
  const DropRt dr = drop_begin(d);
  __shared__ float csum[3][4][64];
  const int cl4 = C * L / 4, l4n = L / 4, M = 2 * C;
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int r = blockIdx.x * 64 + col;
  const bool active = r < cl4;
  const int c = active ? r / l4n : 0;
  const ChanBn<2> bn = chan_load<2>(chan, M, C, c);
  float sw[2] = {0.f, 0.f}, sb[2] = {0.f, 0.f};
  const int s_beg = blockIdx.y * chunk;
  int s_end = s_beg + chunk;
  if (s_end > b) s_end = b;
  if (active) {
    for (int s = s_beg + sl; s < s_end; s += 4) {
      const int64_t e = ((int64_t)s * cl4 + r) * 4;
      const int64_t ub = ((int64_t)s * M) * L + (int64_t)r * 4;
      const float4 ua = ld4(U + ub), ug = ld4(U + ub + (int64_t)C * L), gv = ld4(g + e);
      const float4 m = drop_mult4(dr, (uint64_t)e);
      // the mix backward with LinearGLU alone and weight 1 (its dgamma sum has no reader and compiles to nothing)
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      float unused[4] = {0.f, 0.f, 0.f, 0.f};
      float4 da, dg, df;
      mix_bwd4<kGlu>(1.f, 0.f, gv, zero, zero, ua, ug, zero, m, zero, bn, unused, da, dg, df, sw, sb);
      st4_wtg<2>(dV + ub, da);
      st4_wtg<2>(dV + ub + (int64_t)C * L, dg);
    }
  }
  float cs[4];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    cs[k] = row_sum(sw[k], l4n);
    cs[2 + k] = row_sum(sb[k], l4n);
  }
  if (sl > 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) csum[sl - 1][k][col] = cs[k];
  }
  __syncthreads();
  if (sl == 0 && active && (r % l4n) == 0) {
#pragma unroll
    for (int k = 0; k < 4; ++k) cs[k] += csum[0][k][col] + csum[1][k][col] + csum[2][k][col];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      atomicAdd(bn_grad + k * C + c, cs[k]);
      atomicAdd(bn_grad + M + k * C + c, cs[2 + k]);
    }
  }
}

// standalone BatchNorm + activation + dropout tail: ACT = kActRelu (ConcatFC, out_conv, the reshape layers) |
// kActMish (CatConvMish, reference node_operations.py:58-82)
template <int ACT = kActRelu>
__device__ __forceinline__ void bn_relu_fwd_body(const float* __restrict__ U, float* __restrict__ chan,
                                                 const BnFin& fin, float* __restrict__ out, int b, int M, int L,
                                                 const DropCfg& d, const int bx, const int nbx, float* fin_lds) {
  const DropRt dr = drop_begin(d);
  float* sc = fin_lds;
  float* sh = fin_lds + M;
  bn_fin_fill<256>(fin, chan, M, b * L, sc, sh, bx == 0);
  const int ml4 = M * L / 4, l4n = L / 4;
  const int64_t total = (int64_t)b * ml4;
  for (int64_t i = (int64_t)bx * 256 + threadIdx.x; i < total; i += (int64_t)nbx * 256) {
    const int r = (int)(i % ml4);
    const int c = r / l4n;
    const float4 v = affine4(ld4(U + i * 4), sc[c], sh[c]);
    const float4 m = drop_mult4(dr, (uint64_t)(i * 4));
    if constexpr (ACT == kActMish) {
      const float4 a = act4(v, 1);
      st4_wtg<2>(out + i * 4, make_float4(a.x * m.x, a.y * m.y, a.z * m.z, a.w * m.w));
    } else {
      st4_wtg<2>(out + i * 4, make_float4(fmaxf(v.x, 0.f) * m.x, fmaxf(v.y, 0.f) * m.y,
                                    fmaxf(v.z, 0.f) * m.z, fmaxf(v.w, 0.f) * m.w));
    }
  }
}

__global__ __launch_bounds__(256) void bn_relu_fwd_k(const float* __restrict__ U,
                                                     float* __restrict__ chan, BnFin fin,
                                                     float* __restrict__ out, int b, int M, int L,
                                                     DropCfg d) {
  extern __shared__ float fin_lds[];
  bn_relu_fwd_body(U, chan, fin, out, b, M, L, d, blockIdx.x, gridDim.x, fin_lds);
}

__global__ __launch_bounds__(256) void bn_mish_fwd_k(const float* __restrict__ U,
                                                     float* __restrict__ chan, BnFin fin,
                                                     float* __restrict__ out, int b, int M, int L,
                                                     DropCfg d) {
  extern __shared__ float fin_lds[];
  bn_relu_fwd_body<kActMish>(U, chan, fin, out, b, M, L, d, blockIdx.x, gridDim.x, fin_lds);
}

// The same for up to kBnGroup convs of one shape in ONE launch (the N reshape layers in front of the fusion
// cell, aux_models.py:71-74 / 111-114): blockIdx.y = problem.
constexpr int kBnGroup = 8;
struct BnReluFwdGroup {
  const float* U[kBnGroup];
  float* chan[kBnGroup];
  float* out[kBnGroup];
  BnFin fin[kBnGroup];
  DropCfg drop[kBnGroup];
};
__global__ __launch_bounds__(256) void bn_relu_fwd_group_k(BnReluFwdGroup G, int b, int M, int L) {
  extern __shared__ float fin_lds[];
  // (chains over the compile-time-indexed elements, not G.x[p]: a run-time index sends the by-value argument
  // struct through scratch)
  const int p = blockIdx.y;
  BnFin fin = G.fin[0];
  DropCfg d = G.drop[0];
  const float* U = G.U[0];
  float* chan = G.chan[0];
  float* out = G.out[0];
#pragma unroll
  for (int q = 1; q < kBnGroup; ++q)
    if (p == q) { fin = G.fin[q]; d = G.drop[q]; U = G.U[q]; chan = G.chan[q]; out = G.out[q]; }
  bn_relu_fwd_body(U, chan, fin, out, b, M, L, d, blockIdx.x, gridDim.x, fin_lds);
}

template <int ACT = kActRelu>
__device__ __forceinline__ void bn_relu_bwd_body(const float* __restrict__ g, const float* __restrict__ U,
                                                 const float* __restrict__ chan, float* __restrict__ dV,
                                                 float* bn_grad, int b, int M, int L, int chunk, const DropCfg& d,
                                                 const int bx, const int by, float (*csum)[2][64]) {
  const DropRt dr = drop_begin(d);
  const int ml4 = M * L / 4, l4n = L / 4;
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;
  const int r = bx * 64 + col;
  const bool active = r < ml4;
  const int c = active ? r / l4n : 0;
  const float mu = chan[c], rs = chan[M + c], sc = chan[2 * M + c], sh = chan[3 * M + c];
  float sw = 0.f, sb = 0.f;
  const int s_beg = by * chunk;
  int s_end = s_beg + chunk;
  if (s_end > b) s_end = b;
  if (active) {
    for (int s = s_beg + sl; s < s_end; s += 4) {
      const int64_t e = ((int64_t)s * ml4 + r) * 4;
      const float4 u = ld4(U + e), gv = ld4(g + e);
      const float4 m = drop_mult4(dr, (uint64_t)e);
      const float uq[4] = {u.x, u.y, u.z, u.w}, gq[4] = {gv.x, gv.y, gv.z, gv.w},
                  mq[4] = {m.x, m.y, m.z, m.w};
      float dv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float v = fmaf(uq[t], sc, sh);
        if constexpr (ACT == kActMish) dv[t] = gq[t] * mq[t] * dact_f(v, 1);
        else dv[t] = (v > 0.f) ? gq[t] * mq[t] : 0.f;
        sw += dv[t] * (uq[t] - mu) * rs;
        sb += dv[t];
      }
      st4_wtg<2>(dV + e, make_float4(dv[0], dv[1], dv[2], dv[3]));
    }
  }
  float w = row_sum(sw, l4n), bb = row_sum(sb, l4n);
  if (sl > 0) {
    csum[sl - 1][0][col] = w;
    csum[sl - 1][1][col] = bb;
  }
  __syncthreads();
  if (sl == 0 && active && (r % l4n) == 0) {
    w += csum[0][0][col] + csum[1][0][col] + csum[2][0][col];
    bb += csum[0][1][col] + csum[1][1][col] + csum[2][1][col];
    atomicAdd(bn_grad + c, w);
    atomicAdd(bn_grad + M + c, bb);
  }
}

__global__ __launch_bounds__(256) void bn_relu_bwd_k(const float* __restrict__ g,
                                                     const float* __restrict__ U,
                                                     const float* __restrict__ chan,
                                                     float* __restrict__ dV, float* bn_grad, int b,
                                                     int M, int L, int chunk, DropCfg d) {
  __shared__ float csum[3][2][64];
  bn_relu_bwd_body(g, U, chan, dV, bn_grad, b, M, L, chunk, d, blockIdx.x, blockIdx.y, csum);
}

__global__ __launch_bounds__(256) void bn_mish_bwd_k(const float* __restrict__ g,
                                                     const float* __restrict__ U,
                                                     const float* __restrict__ chan,
                                                     float* __restrict__ dV, float* bn_grad, int b,
                                                     int M, int L, int chunk, DropCfg d) {
  __shared__ float csum[3][2][64];
  bn_relu_bwd_body<kActMish>(g, U, chan, dV, bn_grad, b, M, L, chunk, d, blockIdx.x, blockIdx.y, csum);
}

// ... and its backward for the whole group: blockIdx.z = problem
struct BnReluBwdGroup {
  const float* g[kBnGroup];
  const float* U[kBnGroup];
  const float* chan[kBnGroup];
  float* dV[kBnGroup];
  float* bn_grad[kBnGroup];
  DropCfg drop[kBnGroup];
};
__global__ __launch_bounds__(256) void bn_relu_bwd_group_k(BnReluBwdGroup G, int b, int M, int L, int chunk) {
  __shared__ float csum[3][2][64];
  const int p = blockIdx.z;
  DropCfg d = G.drop[0];
  const float* g = G.g[0];
  const float* U = G.U[0];
  const float* chan = G.chan[0];
  float* dV = G.dV[0];
  float* bn_grad = G.bn_grad[0];
#pragma unroll
  for (int q = 1; q < kBnGroup; ++q)
    if (p == q) { d = G.drop[q]; g = G.g[q]; U = G.U[q]; chan = G.chan[q]; dV = G.dV[q]; bn_grad = G.bn_grad[q]; }
  bn_relu_bwd_body(g, U, chan, dV, bn_grad, b, M, L, chunk, d, blockIdx.x, blockIdx.y, csum);
}

// NodeCell's tail with node_multiplier != 1 (node_search.py:64-69) as ONE launch per direction:
//   o = dropout(relu(bn(U)));  out = LayerNorm(o + resid)
// One workgroup per sample (the LayerNorm's two reductions stay in registers); the BatchNorm is
// finalised by every workgroup at its start (bn_fin.hpp).  o is written out as well: the batched
// LayerNorm-affine gradient of the backward epilogue reads the LayerNorm input from it.
// NP > 0 (small batches): the NEXT cell step's K1 pair sum rides along (FusionCell.forward, reference
// models/search/darts/model_search.py:58 + node_search.py:54 at t = 0): its inputs are NP earlier states plus
// the node output this workgroup has just normalised — per-sample, elementwise, and all of its loads go out
// with the kernel's first loads:   h = sum_{j < NP} w_j xs[j] + w_NP out,   z = (w2_0 + w2_1) h.
// One launch (~4.8 us at 6-8 samples per GPU) less per cell step after the first.
struct PairNextF {
  PtrsIn xs;
  const float* w;          // softmaxed edge weights, element j at w[j * ws]
  const float* w2;
  float* h;
  float* z;
  int ws, w2s;
};

template <int VPT, int BS, int NP = 0>
__global__ __launch_bounds__(BS) void bn_relu_ln_fwd_k(
    const float* __restrict__ U, float* __restrict__ chan, BnFin fin, const float* __restrict__ resid,
    const float* __restrict__ ln_w, const float* __restrict__ ln_b, float* __restrict__ o_out,
    float* __restrict__ out, float* __restrict__ stats, int b, int C, int L, DropCfg d,
    float* __restrict__ osum, PairNextF P) {
  const DropRt dr = drop_begin(d);
  __shared__ float red[8];
  __shared__ float red6[8 * 6];
  extern __shared__ float fin_lds[];
  const int cl4 = C * L / 4, l4n = L / 4;
  const int smp = blockIdx.x;
  float* sc = fin_lds;
  float* sh = fin_lds + C;
  float4 v[VPT], lw[VPT], lb[VPT], rv[VPT];
  float4 pn[VPT][NP > 0 ? NP : 1];
  float pw[NP + 1];
  float ps2 = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {                     // every global load first, then the finalisation
    const int r0 = threadIdx.x + k * BS;
    const int r = r0 < cl4 ? r0 : cl4 - 1;            // clamped, not predicated (see node_mix_ln_fwd_k)
    const int64_t e = ((int64_t)smp * cl4 + r) * 4;
    lw[k] = ld4(ln_w + (int64_t)r * 4);
    lb[k] = ld4(ln_b + (int64_t)r * 4);
    v[k] = ld4(U + e);
    rv[k] = ld4(resid + e);
    if (NP > 0) {
#pragma unroll
      for (int j = 0; j < NP; ++j) pn[k][j] = ld4(P.xs.p[j] + e);
    }
  }
  if (NP > 0) {
#pragma unroll
    for (int j = 0; j <= NP; ++j) pw[j] = P.w[j * P.ws];
    ps2 = P.w2[0] + P.w2[P.w2s];
  }
  bn_fin_fill<BS>(fin, chan, C, b * L, sc, sh, blockIdx.x == 0);
  float sum = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    if (r < cl4) {
      const int c = r / l4n;
      const int64_t e = ((int64_t)smp * cl4 + r) * 4;
      const float4 a = affine4(v[k], sc[c], sh[c]);
      const float4 m = drop_mult4(dr, (uint64_t)e);
      const float4 o = make_float4(fmaxf(a.x, 0.f) * m.x, fmaxf(a.y, 0.f) * m.y, fmaxf(a.z, 0.f) * m.z,
                                   fmaxf(a.w, 0.f) * m.w);
      st4_wtg<2>(o_out + e, o);
      v[k] = f4_add(o, rv[k]);
      sum += f4_hsum(v[k]);
    }
  }
  const float inv_d = 1.f / (float)(cl4 * 4);
  const float mean = block_sum_fresh<BS / 64>(sum, red) * inv_d;     // (first use of red: no barrier in front)
  float acc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // see node_mix_ln_fwd_k
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    if (r < cl4) {
      const float4 cdev = make_float4(v[k].x - mean, v[k].y - mean, v[k].z - mean, v[k].w - mean);
      acc[0] += f4_dot(cdev, cdev);
      if (osum != nullptr) {
        const float4 cw = f4_mul(cdev, lw[k]);
        acc[1] += f4_hsum(cw);
        acc[2] += f4_dot(cw, cw);
        acc[3] += f4_dot(cw, lb[k]);
        acc[4] += f4_hsum(lb[k]);
        acc[5] += f4_dot(lb[k], lb[k]);
      }
    }
  }
  if (osum != nullptr) {
    block_sum_lead_fresh<BS / 64, 6>(acc, red6);
  } else {
    acc[0] = block_sum_fresh<BS / 64>(acc[0], red6);        // (red6, not red: threads may still be reading the mean)
  }
  const float var = acc[0] * inv_d;
  const float rstd = 1.f / sqrtf(var + kLnEps);
  if (threadIdx.x == 0) {
    stats[2 * smp] = mean;
    stats[2 * smp + 1] = rstd;
    if (osum != nullptr) {
      osum[2 * smp] = rstd * acc[1] + acc[4];
      osum[2 * smp + 1] = rstd * rstd * acc[2] + 2.f * rstd * acc[3] + acc[5];
    }
  }
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    if (r < cl4) {
      const float4 y = ln_apply4(v[k], mean, rstd, lw[k], lb[k]);
      const int64_t e = ((int64_t)smp * cl4 + r) * 4;
      st4_wtg<2>(out + e, y);
      if (NP > 0) {
        // the arithmetic of mixsum_pair_fwd_k, in its order: inputs 0 .. NP-1, then this output
        float4 acc = f4_scale(pn[k][0], pw[0]);
#pragma unroll
        for (int j = 1; j < NP; ++j) {
          acc.x = fmaf(pw[j], pn[k][j].x, acc.x);
          acc.y = fmaf(pw[j], pn[k][j].y, acc.y);
          acc.z = fmaf(pw[j], pn[k][j].z, acc.z);
          acc.w = fmaf(pw[j], pn[k][j].w, acc.w);
        }
        acc.x = fmaf(pw[NP], y.x, acc.x);
        acc.y = fmaf(pw[NP], y.y, acc.y);
        acc.z = fmaf(pw[NP], y.z, acc.z);
        acc.w = fmaf(pw[NP], y.w, acc.w);
        st4_wtg<2>(P.h + e, acc);
        st4_wtg<2>(P.z + e, f4_scale(acc, ps2));
      }
    }
  }
}

// Backward of the same tail: LayerNorm input gradient dx (added to / written as the residual's
// gradient), then through dropout and ReLU to dV (the gradient w.r.t. the BatchNorm output) plus the
// BatchNorm reductions bn_grad = (sum dV * u_hat | sum dV) — one atomic pair per channel per sample.
// NP > 0 (one float4 per lane, small batches): the backward of the NEXT cell step's K1 pair sum runs first, in
// the same launch (bmnas_mixsum_pair_bwd, model_search.py:58 backwards).  That sum's last input is THIS node's
// output, so its backward is what completes the gradient the LayerNorm backward below starts from:
//   G = gh + (w2_0 + w2_1) (gz + gz2);   dxs[j] (=|+=) w_j G, dw_j += <G, xs[j]>  (j < NP);
//   gy = g + w_NP G  (g: what other consumers accumulated, nullable; gy is also written to g_full for the
//   deferred LayerNorm-affine reduction),  dw_NP += <G, out>,  dw2_0, dw2_1 += <gz + gz2, h>.
// Destinations must not alias each other (cell-level states never do).
struct PairPrevB {
  PtrsIn xs;
  PtrsOut dxs;
  const float* out;       // this node's forward output
  const float* w;
  const float* w2;
  const float* h;
  const float* gh;        // nullable
  const float* gz;
  const float* gz2;       // nullable
  float* dw;
  float* dw2;
  float* g_full;
  int64_t dw_stride;
  int ws, w2s, dw_shards;
  uint32_t acc;
};

template <int VPT, int BS, int NP = 0>
__global__ __launch_bounds__(BS) void bn_relu_ln_bwd_k(
    const float* __restrict__ g, const float* __restrict__ o, const float* __restrict__ resid,
    const float* __restrict__ ln_w, const float* __restrict__ stats, const float* __restrict__ U,
    const float* __restrict__ chan, float* __restrict__ dV, float* bn_grad, float* dresid, int acc_resid,
    int b, int C, int L, DropCfg d, PairPrevB P) {
  const DropRt dr = drop_begin(d);
  __shared__ float red[2 * (BS / 64)];
  __shared__ float redp[(BS / 64) * (NP + 2)];
  const int cl4 = C * L / 4, l4n = L / 4;
  const int smp = blockIdx.x;
  const float mean = stats[2 * smp], rstd = stats[2 * smp + 1];
  float4 xh[VPT], dxh[VPT], u[VPT], old[VPT];
  float s1 = 0.f, s2 = 0.f;
  float part[NP + 2];
#pragma unroll
  for (int j = 0; j < NP + 2; ++j) part[j] = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    xh[k] = dxh[k] = u[k] = old[k] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < cl4) {
      const int64_t e = ((int64_t)smp * cl4 + r) * 4;
      const float4 x = f4_add(ld4(o + e), ld4(resid + e));
      const float4 w = ld4(ln_w + (int64_t)r * 4);
      float4 gy = make_float4(0.f, 0.f, 0.f, 0.f);
      if (NP == 0 || g != nullptr) gy = ld4(g + e);
      u[k] = ld4(U + e);
      if (acc_resid) old[k] = ld4(dresid + e);
      if (NP > 0) {
        // every load of the pair backward with the loads above, arithmetic after
        const float4 za = ld4(P.gz + e), h4 = ld4(P.h + e), ov = ld4(P.out + e);
        float4 zb = make_float4(0.f, 0.f, 0.f, 0.f), gh4 = zb;
        if (P.gz2 != nullptr) zb = ld4(P.gz2 + e);
        if (P.gh != nullptr) gh4 = ld4(P.gh + e);
        float4 xv[NP > 0 ? NP : 1], od[NP > 0 ? NP : 1];
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          xv[j] = ld4(P.xs.p[j] + e);
          od[j] = make_float4(0.f, 0.f, 0.f, 0.f);
          if (P.dxs.p[j] != nullptr && (P.acc & (1u << j))) od[j] = ld4(P.dxs.p[j] + e);
        }
        const float sw2 = P.w2[0] + P.w2[P.w2s];
        const float4 z4 = f4_add(za, zb);
        const float4 G = f4_add(f4_scale(z4, sw2), gh4);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
          part[j] += f4_dot(G, xv[j]);
          if (P.dxs.p[j] != nullptr) st4_wtg<2>(P.dxs.p[j] + e, f4_add(f4_scale(G, P.w[j * P.ws]), od[j]));
        }
        part[NP] += f4_dot(G, ov);
        part[NP + 1] += f4_dot(z4, h4);
        gy = f4_add(gy, f4_scale(G, P.w[NP * P.ws]));
        st4_wtg<2>(P.g_full + e, gy);
      }
      xh[k] = ln_xhat4(x, mean, rstd);
      dxh[k] = f4_mul(gy, w);
      s1 += f4_hsum(dxh[k]);
      s2 += f4_dot(dxh[k], xh[k]);
    }
  }
  // the LayerNorm backward's two sums and (NP > 0) the mixed-sum weight gradients behind ONE barrier (three
  // reductions with two barriers each before); `red` / `redp` are written once per launch
  constexpr int NWV = BS / 64;
  ln_bwd_sums_put<NWV>(s1, s2, red);
  if (NP > 0) {
#pragma unroll
    for (int j = 0; j < NP + 2; ++j) part[j] = wave_sum(part[j]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int j = 0; j < NP + 2; ++j) redp[j * NWV + (threadIdx.x >> 6)] = part[j];
    }
  }
  __syncthreads();
  if (NP > 0 && (int)threadIdx.x <= NP + 2) {
    // dw / dw2: one sharded atomic per weight per workgroup, as bmnas_mixsum_pair_bwd (t = NP + 1, NP + 2: the two
    // dw2 adds of the same sum)
    const int t = threadIdx.x;
    const int q = t <= NP ? t : NP + 1;
    float val = redp[q * NWV];
#pragma unroll
    for (int w = 1; w < NWV; ++w) val += redp[q * NWV + w];
    const int64_t sh = (int64_t)(blockIdx.x % P.dw_shards) * P.dw_stride;
    if (t <= NP) atomicAdd(P.dw + sh + t * P.ws, val);
    else atomicAdd(P.dw2 + sh + (t - NP - 1) * P.w2s, val);
  }
  float m1, m2;
  ln_bwd_sums_get<NWV>(red, 1.f / (float)(cl4 * 4), m1, m2);
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int r = threadIdx.x + k * BS;
    const bool act = r < cl4;
    const int c = act ? r / l4n : 0;
    float sw = 0.f, sb = 0.f;
    if (act) {
      const int64_t e = ((int64_t)smp * cl4 + r) * 4;
      const float4 dx = ln_dx4(dxh[k], xh[k], m1, m2, rstd);
      if (dresid != nullptr) st4_wtg<2>(dresid + e, f4_add(dx, old[k]));
      const float mu = chan[c], rs = chan[C + c], scv = chan[2 * C + c], shv = chan[3 * C + c];
      const float4 m = drop_mult4(dr, (uint64_t)e);
      const float uq[4] = {u[k].x, u[k].y, u[k].z, u[k].w}, gq[4] = {dx.x, dx.y, dx.z, dx.w},
                  mq[4] = {m.x, m.y, m.z, m.w};
      float dv[4];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float a = fmaf(uq[t], scv, shv);
        dv[t] = (a > 0.f) ? gq[t] * mq[t] : 0.f;
        sw += dv[t] * (uq[t] - mu) * rs;
        sb += dv[t];
      }
      st4_wtg<2>(dV + e, make_float4(dv[0], dv[1], dv[2], dv[3]));
    }
    sw = row_sum(sw, l4n);
    sb = row_sum(sb, l4n);
    if (act && (r % l4n) == 0) {
      atomicAdd(bn_grad + c, sw);
      atomicAdd(bn_grad + C + c, sb);
    }
  }
}

// dU = scale * (dV - db/N - u_hat * dw/N)   (training);  dU = scale * dV  (eval)
__global__ __launch_bounds__(256) void bn_bwd_apply_k(float* __restrict__ dV,
                                                      const float* __restrict__ U,
                                                      const float* __restrict__ chan,
                                                      const float* __restrict__ bn_grad, int b,
                                                      int M, int L, int training) {
  const int ml4 = M * L / 4, l4n = L / 4;
  const int64_t total = (int64_t)b * ml4;
  const float invN = 1.f / (float)(b * L);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int r = (int)(i % ml4);
    const int c = r / l4n;
    const float sc = chan[2 * M + c];
    float4 d = ld4(dV + i * 4);
    if (training) {
      const float mu = chan[c], rs = chan[M + c];
      const float kw = bn_grad[c] * invN, kb = bn_grad[M + c] * invN;
      const float4 u = ld4(U + i * 4);
      d.x = sc * (d.x - kb - (u.x - mu) * rs * kw);
      d.y = sc * (d.y - kb - (u.y - mu) * rs * kw);
      d.z = sc * (d.z - kb - (u.z - mu) * rs * kw);
      d.w = sc * (d.w - kb - (u.w - mu) * rs * kw);
    } else {
      d = f4_scale(d, sc);
    }
    st4_wtg<2>(dV + i * 4, d);
  }
}

__global__ void arch_softmax_fwd_k(const float* __restrict__ a, float* __restrict__ w, int rows,
                                   int cols) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float mx = a[r * cols];
  for (int p = 1; p < cols; ++p) mx = fmaxf(mx, a[r * cols + p]);
  float den = 0.f;
  for (int p = 0; p < cols; ++p) den += expf(a[r * cols + p] - mx);
  for (int p = 0; p < cols; ++p) w[r * cols + p] = expf(a[r * cols + p] - mx) / den;
}

__global__ void arch_softmax_bwd_k(const float* __restrict__ w, const float* __restrict__ dw,
                                   float* __restrict__ da, int rows, int cols) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float dot = 0.f;
  for (int p = 0; p < cols; ++p) dot += w[r * cols + p] * dw[r * cols + p];
  for (int p = 0; p < cols; ++p) da[r * cols + p] = w[r * cols + p] * (dw[r * cols + p] - dot);
}

// backward of the row softmaxes with the shard sum spread over a wavefront: block = one row
__global__ __launch_bounds__(64) void arch_softmax_multi_bwd_k(ArchPack P) {
  arch_softmax_bwd_row(P, blockIdx.x, threadIdx.x);
}

// every row of every architecture tensor in ONE launch (<= 94 rows in total)
__global__ void arch_softmax_multi_k(ArchPack P, int backward) {
  int r = blockIdx.x * blockDim.x + threadIdx.x;
  for (int t = 0; t < P.n; ++t) {
    if (r < P.rows[t]) {
      const int cols = P.cols[t];
      const float* a = P.a[t] + r * cols;
      float* o = P.o[t] + r * cols;
      if (!backward) {
        float mx = a[0];
        for (int p = 1; p < cols; ++p) mx = fmaxf(mx, a[p]);
        float den = 0.f;
        for (int p = 0; p < cols; ++p) den += expf(a[p] - mx);
        for (int p = 0; p < cols; ++p) o[p] = expf(a[p] - mx) / den;
      } else {
        const float* dwp = P.b[t] + r * cols;
        float dw[4], dot = 0.f;
        for (int p = 0; p < cols; ++p) {
          float acc = 0.f;
          for (int sh = 0; sh < P.n_shards; ++sh) acc += dwp[(int64_t)sh * P.shard_stride + p];
          dw[p] = acc;
          dot += a[p] * acc;
        }
        for (int p = 0; p < cols; ++p) o[p] = a[p] * (dw[p] - dot);
      }
      return;
    }
    r -= P.rows[t];
  }
}

// ---- cell prologue: everything a FusionCell forward needs before its first data kernel, in
// ONE launch — the row softmax of every architecture tensor (alpha, betas, gammas) and the folded
// conv weights Weff = W[:, :C] + W[:, C:] of every NodeMixedOp (search mode feeds cat[z, z]).
// Three 4-us launches (2 folds + softmax at MM-IMDB) become one.
constexpr int kMaxFold = 8;
struct FoldPack {
  const float* W[kMaxFold];
  float* Weff[kMaxFold];
  int n, M, C, blocks_per;
};

// bid / nblocks: this workgroup's index among the prologue workgroups of the launch
__device__ __forceinline__ void cell_prologue_body(const ArchPack& P, const FoldPack& F,
                                                   unsigned long long* step_counter,
                                                   const unsigned long long* step_span,
                                                   float* __restrict__ scrub, int64_t scrub4, const int bid,
                                                   const int nblocks) {
  const int nfb = F.n * F.blocks_per;
  // side job: zero-fill the caller's forward accumulation buffers (BatchNorm batch sums that the GEMM
  // epilogues add into with atomics, the head's logits) — instead of a memset launch
  for (int64_t i = (int64_t)bid * 256 + threadIdx.x; i < scrub4; i += (int64_t)nblocks * 256)
    st4_wt(scrub + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
  // hipGraph replays: advance the dropout step counter once, here, before any kernel of this replay
  // reads it (one thread of the last workgroup; every later kernel is ordered after this launch)
  if (step_counter != nullptr && bid == nblocks - 1 && threadIdx.x == 0)
    step_counter[0] += step_span[0];
  if (bid < nfb) {
    const int q = bid / F.blocks_per, bi = bid - q * F.blocks_per;   // workgroup-uniform
    const float* __restrict__ W = F.W[q];
    float* __restrict__ We = F.Weff[q];
    const int c4n = F.C / 4;
    const int total = F.M * c4n;
    for (int i = bi * 256 + threadIdx.x; i < total; i += F.blocks_per * 256) {
      const int m = i / c4n, c4 = i - m * c4n;
      const float* r = W + (int64_t)m * 2 * F.C + 4 * c4;
      st4_wt(We + (int64_t)m * F.C + 4 * c4, f4_add(ld4(r), ld4(r + F.C)));
    }
    return;
  }
  int r = (bid - nfb) * 256 + threadIdx.x;
  for (int t = 0; t < P.n; ++t) {
    if (r < P.rows[t]) {
      const int cols = P.cols[t];
      const float* a = P.a[t] + r * cols;
      float* o = P.o[t] + r * cols;
      // the row's (at most four) logits in ONE batch, from clamped addresses: the three loops over `cols` below each
      // loaded a[p] again, one s_waitcnt vmcnt(0) per trip — up to eleven dependent round trips in the one workgroup
      // of the launch that every other one finishes ahead of
      float av[4];
#pragma unroll
      for (int p = 0; p < 4; ++p) av[p] = a[p < cols ? p : cols - 1];
      float mx = av[0];
#pragma unroll
      for (int p = 1; p < 4; ++p) mx = p < cols ? fmaxf(mx, av[p]) : mx;
      float ev[4], den = 0.f;
#pragma unroll
      for (int p = 0; p < 4; ++p) {
        ev[p] = expf(av[p] - mx);
        den = p < cols ? den + ev[p] : den;
      }
#pragma unroll
      for (int p = 0; p < 4; ++p)
        if (p < cols) o[p] = ev[p] / den;
      return;
    }
    r -= P.rows[t];
  }
}

__global__ __launch_bounds__(256) void cell_prologue_k(ArchPack P, FoldPack F, unsigned long long* step_counter,
                                                       const unsigned long long* step_span,
                                                       float* __restrict__ scrub, int64_t scrub4) {
  cell_prologue_body(P, F, step_counter, step_span, scrub, scrub4, (int)blockIdx.x, (int)gridDim.x);
}

// softmax(row)[1] of a two-column logits row, with the arithmetic of the prologue's row softmax (the
// backward kernels read the prologue's stored weights: both must be the same bits)
__device__ __forceinline__ float softmax2_col1(const float* a) {
  const float a0 = a[0], a1 = a[1];
  const float mx = fmaxf(a0, a1);
  const float e0 = expf(a0 - mx), e1 = expf(a1 - mx);
  return e1 / (e0 + e1);
}

// The prologue AND the first data kernel of the cell in one launch: workgroups [0, n_pro) do the
// prologue's independent jobs, the rest stream the first step's mixed-edge pair sum
//   h = sum_j softmax(alpha)[j, 1] x_j,   z = (softmax(beta)[0, 1] + softmax(beta)[1, 1]) h
// (bmnas_mixsum_pair_fwd) with the edge weights computed from the raw logits in registers — nothing
// of the prologue's output is needed before the NEXT launch.  One launch less per step.
struct PairArgs {
  PtrsIn xs;
  const float* alpha;      // logits of the step's first edge, rows of 2
  const float* beta;       // logits of the node's first two inner edges, rows of 2
  float* out;
  float* out2;
  int64_t n4;
};

template <int NIN>
__global__ __launch_bounds__(256) void cell_prologue_pair_k(ArchPack P, FoldPack F, unsigned long long* step_counter,
                                                            const unsigned long long* step_span,
                                                            float* __restrict__ scrub, int64_t scrub4, int n_pro,
                                                            PairArgs A) {
  if ((int)blockIdx.x < n_pro) {
    cell_prologue_body(P, F, step_counter, step_span, scrub, scrub4, (int)blockIdx.x, n_pro);
    return;
  }
  const int64_t stride = (int64_t)(gridDim.x - n_pro) * 256;
  int64_t i = (int64_t)(blockIdx.x - n_pro) * 256 + threadIdx.x;
  if (i >= A.n4) return;
  // the first trip's operands are requested BEFORE the edge weights: the logits sit behind pointers of the argument
  // block (a second scalar round trip) and their softmaxes are ~350 instructions — in front of the operand loads both
  // were part of the launch's one dependent chain, behind them they run while the operands travel
  float4 v[NIN];
#pragma unroll
  for (int j = 0; j < NIN; ++j) v[j] = reinterpret_cast<const float4*>(A.xs.p[j])[i];
  __builtin_amdgcn_sched_barrier(0);
  float wj[NIN];
#pragma unroll
  for (int j = 0; j < NIN; ++j) wj[j] = softmax2_col1(A.alpha + 2 * j);
  const float s2 = softmax2_col1(A.beta) + softmax2_col1(A.beta + 2);
  for (;;) {
    float4 acc = f4_scale(v[0], wj[0]);
#pragma unroll
    for (int j = 1; j < NIN; ++j) {
      acc.x = fmaf(wj[j], v[j].x, acc.x);
      acc.y = fmaf(wj[j], v[j].y, acc.y);
      acc.z = fmaf(wj[j], v[j].z, acc.z);
      acc.w = fmaf(wj[j], v[j].w, acc.w);
    }
    st4_w0<0>(A.out + 4 * i, acc);
    st4_w0<0>(A.out2 + 4 * i, f4_scale(acc, s2));
    i += stride;
    if (i >= A.n4) break;
#pragma unroll
    for (int j = 0; j < NIN; ++j) v[j] = reinterpret_cast<const float4*>(A.xs.p[j])[i];
  }
}

}  // namespace

extern "C" int bmnas_version(void) { return 100; }

extern "C" int bmnas_bn_finalize_ex(const float* part, int n_part, int b, int L, int M,
                                    const float* bn_w, const float* bn_b, float* running_mean,
                                    float* running_var, int64_t* num_batches_tracked, int n_nbt,
                                    int training, float momentum, int momentum_mode, float* chan, void* stream) {
  if (!bn_w || !bn_b || !chan || M < 1 || b < 1 || L < 1) return BMNAS_E_ARG;
  if (training && (!part || n_part < 1 || b * L < 2)) return BMNAS_E_ARG;
  if (!training && (!running_mean || !running_var)) return BMNAS_E_ARG;
  bmnas_bn_fin_t d{};                                      // (the momentum rules of the in-kernel finalisation)
  d.running_mean = running_mean; d.num_batches_tracked = num_batches_tracked; d.n_nbt = n_nbt;
  d.training = training; d.momentum = momentum; d.momentum_mode = momentum_mode;
  BnFin f{};
  f.on = 1;
  if (int e = fin_momentum(d, &f)) return e;
  const bool count_after = (f.on & kFinCum) && training && num_batches_tracked && n_nbt > 0;
  hipLaunchKernelGGL(bn_finalize_k, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, part,
                     n_part, b, L, M, bn_w, bn_b, running_mean, running_var, num_batches_tracked,
                     n_nbt, training, f.mom, count_after ? 1 : 0, chan);
  BMNAS_CHECK_LAUNCH();
  if (count_after) {
    hipLaunchKernelGGL(bn_count_k, dim3((n_nbt + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       num_batches_tracked, n_nbt);
    BMNAS_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int bmnas_bn_finalize(const float* part, int n_part, int b, int L, int M,
                                 const float* bn_w, const float* bn_b, float* running_mean,
                                 float* running_var, int64_t* num_batches_tracked, int n_nbt,
                                 int training, float* chan, void* stream) {
  return bmnas_bn_finalize_ex(part, n_part, b, L, M, bn_w, bn_b, running_mean, running_var, num_batches_tracked,
                              n_nbt, training, 0.f, BMNAS_BN_MOM_DEFAULT, chan, stream);
}

extern "C" int bmnas_node_mix_fwd_next(const float* x, const float* y, const float* p1, const float* U,
                                       float* chan, bmnas_bn_fin_t fin, const float* gamma, float* out,
                                       int b, int C, int L, bmnas_dropout_t drop_glu,
                                       bmnas_dropout_t drop_fc, const float* const* prev, int n_prev,
                                       const float* w, int w_stride, float* z_next, void* stream) {
  if (!x || !y || !p1 || !U || !chan || !gamma || !out || b < 0 || C < 1 || n_prev < 0) return BMNAS_E_ARG;
  if (!len_fwd_ok(L)) return BMNAS_E_SHAPE;
  if (n_prev > kMixPrev) return BMNAS_E_LIMIT;
  MixNextF N{};
  if (n_prev > 0) {
    if (!prev || !w || !z_next || w_stride < 1) return BMNAS_E_ARG;
    if (int e = fill_ptrs(N.prev, prev, n_prev)) return e;
    N.w = w; N.ws = w_stride; N.z = z_next; N.n = n_prev;
  }
  BnFin f;
  if (int e = fin_for(fin, b, L, &f)) return e;
  if (!fin_lds_ok(3, C)) return BMNAS_E_LIMIT;
  if (b == 0) return 0;
  const int64_t total = (int64_t)b * C * L / 4;
  if (int e = dispatch_range<0, kMixPrev>(n_prev, [&](auto NP) {
        hipLaunchKernelGGL(node_mix_fwd_k<decltype(NP)::value>, dim3(stream_grid(total)), dim3(256),
                           (size_t)6 * C * sizeof(float), (hipStream_t)stream, x, y, p1, U, chan, f, gamma, out, b, C,
                           L, to_cfg(drop_glu), to_cfg(drop_fc), N);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_node_mix_fwd(const float* x, const float* y, const float* p1, const float* U,
                                  float* chan, bmnas_bn_fin_t fin, const float* gamma, float* out,
                                  int b, int C, int L, bmnas_dropout_t drop_glu,
                                  bmnas_dropout_t drop_fc, void* stream) {
  return bmnas_node_mix_fwd_next(x, y, p1, U, chan, fin, gamma, out, b, C, L, drop_glu, drop_fc, nullptr, 0,
                                 nullptr, 0, nullptr, stream);
}


extern "C" int bmnas_node_mix_ln_fwd(const float* x, const float* y, const float* p1, const float* U,
                                     float* chan, bmnas_bn_fin_t fin, const float* gamma,
                                     const float* resid, const float* ln_w, const float* ln_b,
                                     float* pre, float* out, float* stats, int b, int C, int L,
                                     bmnas_dropout_t drop_glu, bmnas_dropout_t drop_fc, float* out_sums,
                                     void* stream) {
  if (!x || !y || !p1 || !U || !chan || !gamma || !resid || !ln_w || !ln_b || !pre || !out || !stats ||
      b < 0 || C < 1)
    return BMNAS_E_ARG;
  if (!len_fwd_ok(L)) return BMNAS_E_SHAPE;
  BnFin f;
  if (int e = fin_for(fin, b, L, &f)) return e;
  if (!fin_lds_ok(3, C)) return BMNAS_E_LIMIT;
  if (b == 0) return 0;
  const size_t fin_lds = (size_t)6 * C * sizeof(float);
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_ln<1, 2, 3, 4, 8>(ln_launch_shape(b, C * L / 4), [&](auto V, auto BS) {
        hipLaunchKernelGGL((node_mix_ln_fwd_k<decltype(V)::value, decltype(BS)::value>), dim3(b),
                           dim3(decltype(BS)::value), fin_lds, st, x, y, p1, U, chan, f, gamma, resid, ln_w, ln_b, pre,
                           out, stats, b, C, L, to_cfg(drop_glu), to_cfg(drop_fc), out_sums);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_node_mix_bwd_next(const float* g, const float* x, const float* y, const float* p1,
                                       const float* U, const float* chan, const float* gamma,
                                       float* dgamma, int dgamma_shards, int64_t dgamma_shard_stride,
                                       float* dx, float* dy, uint32_t accumulate_mask, float* dV,
                                       float* bn_grad, int b, int C, int L, bmnas_dropout_t drop_glu,
                                       bmnas_dropout_t drop_fc, const float* const* prev,
                                       float* const* dprev, int n_prev, uint32_t prev_accumulate_mask,
                                       const float* w, int w_stride, float* dw, int dw_shards,
                                       int64_t dw_shard_stride, const float* s, const float* gz,
                                       const float* gz2, float* g_out, void* stream) {
  if (!x || !y || !p1 || !U || !chan || !gamma || !dV || !bn_grad || b < 0 || C < 1 || dgamma_shards < 1 ||
      n_prev < 0)
    return BMNAS_E_ARG;
  if (!len_bwd_ok(L)) return BMNAS_E_SHAPE;
  if (n_prev > kMixPrev) return BMNAS_E_LIMIT;
  MixNextB N{};
  if (n_prev > 0) {
    // g (nullable here) is what other consumers of s accumulated; g_out receives the complete gradient
    if (!prev || !dprev || !w || !dw || !s || !gz || !g_out || w_stride < 1 || dw_shards < 1) return BMNAS_E_ARG;
    if (int e = fill_ptrs(N.prev, prev, n_prev)) return e;
    fill_ptrs_out(N.dprev, dprev, n_prev);
    N.w = w; N.ws = w_stride; N.dw = dw; N.dw_shards = dw_shards; N.dw_stride = dw_shard_stride;
    N.s = s; N.gz = gz; N.gz2 = gz2; N.g_in = g; N.g_out = g_out; N.n = n_prev; N.acc = prev_accumulate_mask;
  } else if (!g) {
    return BMNAS_E_ARG;
  }
  if (b == 0) return 0;
  const int cl4 = C * L / 4;
  const int chunk = pick_chunk(b, cl4);
  dim3 grid((cl4 + 63) / 64, (b + chunk - 1) / chunk);
  if (int e = dispatch_range<0, kMixPrev>(n_prev, [&](auto NP) {
        hipLaunchKernelGGL(node_mix_bwd_k<decltype(NP)::value>, grid, dim3(256), 0, (hipStream_t)stream, g, x, y, p1, U,
                           chan, gamma, dgamma, dgamma_shards, dgamma_shard_stride, dx, dy, accumulate_mask, dV,
                           bn_grad, b, C, L, chunk, to_cfg(drop_glu), to_cfg(drop_fc), N);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_node_mix_bwd(const float* g, const float* x, const float* y, const float* p1,
                                  const float* U, const float* chan, const float* gamma,
                                  float* dgamma, int dgamma_shards, int64_t dgamma_shard_stride,
                                  float* dx, float* dy, uint32_t accumulate_mask, float* dV,
                                  float* bn_grad, int b, int C, int L, bmnas_dropout_t drop_glu,
                                  bmnas_dropout_t drop_fc, void* stream) {
  return bmnas_node_mix_bwd_next(g, x, y, p1, U, chan, gamma, dgamma, dgamma_shards, dgamma_shard_stride, dx, dy,
                                 accumulate_mask, dV, bn_grad, b, C, L, drop_glu, drop_fc, nullptr, nullptr, 0,
                                 0, nullptr, 0, nullptr, 1, 0, nullptr, nullptr, nullptr, nullptr, stream);
}


extern "C" int bmnas_node_mix_ln_bwd_ok(int b, int C, int L) {
  return b >= 1 && b <= 128 && (L == 4 || L == 8 || L == 16) && C >= 2 && C % 2 == 0 && C * L / 4 <= 2048;
}

extern "C" int bmnas_node_mix_ln_bwd(const float* g, const float* pre, const float* ln_w, const float* stats,
                                     float* g_in, float* dresid, int accumulate_resid, const float* x,
                                     const float* y, const float* p1, const float* U, const float* chan,
                                     const float* gamma, float* dgamma, int dgamma_shards,
                                     int64_t dgamma_shard_stride, float* dx, float* dy,
                                     uint32_t accumulate_mask, float* dV, float* bn_grad, int b, int C, int L,
                                     bmnas_dropout_t drop_glu, bmnas_dropout_t drop_fc, void* stream) {
  if (!g || !pre || !ln_w || !stats || !x || !y || !p1 || !U || !chan || !gamma || !dV || !bn_grad || b < 0 ||
      C < 1 || dgamma_shards < 1)
    return BMNAS_E_ARG;
  if (accumulate_resid && !dresid) return BMNAS_E_ARG;
  if (!len_bwd_ok(L)) return BMNAS_E_SHAPE;
  if (b == 0) return 0;
  if (!bmnas_node_mix_ln_bwd_ok(b, C, L)) return BMNAS_E_LIMIT;
  const int cl4 = C * L / 4;
  hipStream_t st = (hipStream_t)stream;
  // BMNAS_MIXLN_PROBE: timing diagnostics only (1: no BatchNorm atomics, 2: half of the first phase,
  // 4: no dgamma atomics — results incomplete)
#if defined(BMNAS_BODY_PROBES) && BMNAS_BODY_PROBES
  static const int probe = []() { const char* e = getenv("BMNAS_MIXLN_PROBE"); return e ? atoi(e) : 0; }();
#else
  const int probe = 0;
#endif
  auto launch = [&](auto V1, auto V2) {
    hipLaunchKernelGGL((node_mix_ln_bwd_k<decltype(V1)::value, decltype(V2)::value, 512>), dim3(2 * b), dim3(512), 0,
                       st, g, pre, ln_w, stats, g_in, dresid, accumulate_resid, x, y, p1, U, chan, gamma, dgamma,
                       dgamma_shards, dgamma_shard_stride, dx, dy, accumulate_mask, dV, bn_grad, b, C, L,
                       to_cfg(drop_glu), to_cfg(drop_fc), probe);
  };
  if (cl4 <= 512) launch(int_c<1>{}, int_c<1>{});
  else if (cl4 <= 1024) launch(int_c<2>{}, int_c<1>{});
  else launch(int_c<4>{}, int_c<2>{});
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_glu_fwd(const float* U, float* chan, bmnas_bn_fin_t fin, float* out, int b, int C, int L,
                                bmnas_dropout_t drop, void* stream) {
  if (!U || !chan || !out || b < 0 || C < 1) return BMNAS_E_ARG;
  if (!len_fwd_ok(L)) return BMNAS_E_SHAPE;
  if (!fin_lds_ok(2, C)) return BMNAS_E_LIMIT;
  BnFin f;
  if (int e = fin_for(fin, b, L, &f)) return e;
  if (b == 0) return 0;
  const int64_t total = (int64_t)b * C * L / 4;
  hipLaunchKernelGGL(bn_glu_fwd_k, dim3(stream_grid(total)), dim3(256), (size_t)4 * C * sizeof(float),
                     (hipStream_t)stream, U, chan, f, out, b, C, L, to_cfg(drop));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_glu_bwd(const float* g, const float* U, const float* chan, float* dV,
                                float* bn_grad, int b, int C, int L, bmnas_dropout_t drop,
                                void* stream) {
  if (!g || !U || !chan || !dV || !bn_grad || b < 0 || C < 1) return BMNAS_E_ARG;
  if (!len_bwd_ok(L)) return BMNAS_E_SHAPE;
  if (b == 0) return 0;
  const int cl4 = C * L / 4;
  const int chunk = pick_chunk(b, cl4);
  dim3 grid((cl4 + 63) / 64, (b + chunk - 1) / chunk);
  hipLaunchKernelGGL(bn_glu_bwd_k, grid, dim3(256), 0, (hipStream_t)stream, g, U, chan, dV, bn_grad,
                     b, C, L, chunk, to_cfg(drop));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

template <typename Kern>
static int bn_act_fwd(Kern kern, const float* U, float* chan, bmnas_bn_fin_t fin, float* out, int b, int M, int L,
                      bmnas_dropout_t drop, void* stream) {
  if (!U || !chan || !out || b < 0 || M < 1) return BMNAS_E_ARG;
  if (!len_fwd_ok(L)) return BMNAS_E_SHAPE;
  if (!fin_lds_ok(1, M)) return BMNAS_E_LIMIT;
  BnFin f;
  if (int e = fin_for(fin, b, L, &f)) return e;
  if (b == 0) return 0;
  const int64_t total = (int64_t)b * M * L / 4;
  hipLaunchKernelGGL(kern, dim3(stream_grid(total)), dim3(256), (size_t)2 * M * sizeof(float),
                     (hipStream_t)stream, U, chan, f, out, b, M, L, to_cfg(drop));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_relu_fwd(const float* U, float* chan, bmnas_bn_fin_t fin, float* out, int b,
                                 int M, int L, bmnas_dropout_t drop, void* stream) {
  return bn_act_fwd(bn_relu_fwd_k, U, chan, fin, out, b, M, L, drop, stream);
}

extern "C" int bmnas_bn_mish_fwd(const float* U, float* chan, bmnas_bn_fin_t fin, float* out, int b,
                                 int M, int L, bmnas_dropout_t drop, void* stream) {
  return bn_act_fwd(bn_mish_fwd_k, U, chan, fin, out, b, M, L, drop, stream);
}

template <typename Kern>
static int bn_act_bwd(Kern kern, const float* g, const float* U, const float* chan, float* dV, float* bn_grad, int b,
                      int M, int L, bmnas_dropout_t drop, void* stream) {
  if (!g || !U || !chan || !dV || !bn_grad || b < 0 || M < 1) return BMNAS_E_ARG;
  if (!len_bwd_ok(L)) return BMNAS_E_SHAPE;
  if (b == 0) return 0;
  const int ml4 = M * L / 4;
  const int chunk = pick_chunk(b, ml4);
  dim3 grid((ml4 + 63) / 64, (b + chunk - 1) / chunk);
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, (hipStream_t)stream, g, U, chan, dV, bn_grad,
                     b, M, L, chunk, to_cfg(drop));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_relu_bwd(const float* g, const float* U, const float* chan, float* dV,
                                 float* bn_grad, int b, int M, int L, bmnas_dropout_t drop,
                                 void* stream) {
  return bn_act_bwd(bn_relu_bwd_k, g, U, chan, dV, bn_grad, b, M, L, drop, stream);
}

extern "C" int bmnas_bn_mish_bwd(const float* g, const float* U, const float* chan, float* dV,
                                 float* bn_grad, int b, int M, int L, bmnas_dropout_t drop,
                                 void* stream) {
  return bn_act_bwd(bn_mish_bwd_k, g, U, chan, dV, bn_grad, b, M, L, drop, stream);
}

extern "C" int bmnas_bn_relu_fwd_group(const bmnas_bn_relu_fwd_prob_t* probs, int n, int b, int M, int L,
                                       void* stream) {
  if (!probs || n < 1 || b < 0 || M < 1) return BMNAS_E_ARG;
  if (n > kBnGroup) return BMNAS_E_LIMIT;
  if (!len_fwd_ok(L)) return BMNAS_E_SHAPE;
  if (!fin_lds_ok(1, M)) return BMNAS_E_LIMIT;
  BnReluFwdGroup G{};
  for (int p = 0; p < n; ++p) {
    if (!probs[p].U || !probs[p].chan || !probs[p].out) return BMNAS_E_ARG;
    if (int e = fin_for(probs[p].fin, b, L, &G.fin[p])) return e;
    G.U[p] = probs[p].U; G.chan[p] = probs[p].chan; G.out[p] = probs[p].out; G.drop[p] = to_cfg(probs[p].drop);
  }
  if (b == 0) return 0;
  const int64_t total = (int64_t)b * M * L / 4;
  // every workgroup starts by finalising the BatchNorm statistics (bn_fin_fill): ~3 workgroups per CU over
  // the whole group, each walking several float4 rounds, not one workgroup per 256 float4
  int gx = stream_grid(total);
  const int cap = std::max(1, 768 / n);
  if (gx > cap) gx = cap;
  hipLaunchKernelGGL(bn_relu_fwd_group_k, dim3(gx, n), dim3(256), (size_t)2 * M * sizeof(float), (hipStream_t)stream,
                     G, b, M, L);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_relu_bwd_group(const bmnas_bn_relu_bwd_prob_t* probs, int n, int b, int M, int L,
                                       void* stream) {
  if (!probs || n < 1 || b < 0 || M < 1) return BMNAS_E_ARG;
  if (n > kBnGroup) return BMNAS_E_LIMIT;
  if (!len_bwd_ok(L)) return BMNAS_E_SHAPE;
  BnReluBwdGroup G{};
  for (int p = 0; p < n; ++p) {
    if (!probs[p].g || !probs[p].U || !probs[p].chan || !probs[p].dV || !probs[p].bn_grad) return BMNAS_E_ARG;
    G.g[p] = probs[p].g; G.U[p] = probs[p].U; G.chan[p] = probs[p].chan; G.dV[p] = probs[p].dV;
    G.bn_grad[p] = probs[p].bn_grad; G.drop[p] = to_cfg(probs[p].drop);
  }
  if (b == 0) return 0;
  const int ml4 = M * L / 4;
  const int chunk = pick_chunk(b, ml4 * n);
  dim3 grid((ml4 + 63) / 64, (b + chunk - 1) / chunk, n);
  hipLaunchKernelGGL(bn_relu_bwd_group_k, grid, dim3(256), 0, (hipStream_t)stream, G, b, M, L, chunk);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_relu_ln_fwd_pair_ok(int b, int C, int L, int n_prev) {
  return b >= 1 && b <= 128 && n_prev >= 1 && n_prev <= BMNAS_MAX_PTRS - 1 && C * L / 4 <= 256;
}

extern "C" int bmnas_bn_relu_ln_fwd_pair(const float* U, float* chan, bmnas_bn_fin_t fin, const float* resid,
                                         const float* ln_w, const float* ln_b, float* o, float* out,
                                         float* stats, int b, int C, int L, bmnas_dropout_t drop,
                                         float* out_sums, const float* const* xs, int n_prev, const float* w,
                                         int w_stride, const float* w2, int w2_stride, float* h, float* z,
                                         void* stream) {
  if (!U || !chan || !resid || !ln_w || !ln_b || !o || !out || !stats || b < 0 || C < 1) return BMNAS_E_ARG;
  PairNextF P{};
  if (n_prev > 0) {
    if (!xs || !w || !w2 || !h || !z || w_stride < 1 || w2_stride < 1) return BMNAS_E_ARG;
    if (!bmnas_bn_relu_ln_fwd_pair_ok(b > 0 ? b : 1, C, L, n_prev)) return BMNAS_E_LIMIT;
    if (int e = fill_ptrs(P.xs.p, xs, n_prev)) return e;
    P.w = w; P.w2 = w2; P.h = h; P.z = z; P.ws = w_stride; P.w2s = w2_stride;
  } else if (n_prev < 0) {
    return BMNAS_E_ARG;
  }
  if (!len_fwd_ok(L) || C % 4) return BMNAS_E_SHAPE;
  BnFin f;
  if (int e = fin_for(fin, b, L, &f)) return e;
  if (b == 0) return 0;
  const size_t fin_lds = (size_t)2 * C * sizeof(float);
  const LnShape sh = ln_launch_shape(b, C * L / 4);
  if (C > 4 * sh.bs) return BMNAS_E_LIMIT;                 // bn_fin_fill: one trip
  hipStream_t st = (hipStream_t)stream;
  const int e = n_prev > 0                                 // (host-checked: one float4 per lane, 256 lanes)
      ? dispatch_range<1, BMNAS_MAX_PTRS - 1>(n_prev, [&](auto NP) {
          hipLaunchKernelGGL((bn_relu_ln_fwd_k<1, 256, decltype(NP)::value>), dim3(b), dim3(256), fin_lds, st, U, chan,
                             f, resid, ln_w, ln_b, o, out, stats, b, C, L, to_cfg(drop), out_sums, P);
        })
      : dispatch_ln<1, 2, 3, 4, 8>(sh, [&](auto V, auto BS) {
          hipLaunchKernelGGL((bn_relu_ln_fwd_k<decltype(V)::value, decltype(BS)::value>), dim3(b),
                             dim3(decltype(BS)::value), fin_lds, st, U, chan, f, resid, ln_w, ln_b, o, out, stats, b,
                             C, L, to_cfg(drop), out_sums, P);
        });
  if (e) return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_relu_ln_fwd(const float* U, float* chan, bmnas_bn_fin_t fin, const float* resid,
                                    const float* ln_w, const float* ln_b, float* o, float* out, float* stats,
                                    int b, int C, int L, bmnas_dropout_t drop, float* out_sums,
                                    void* stream) {
  return bmnas_bn_relu_ln_fwd_pair(U, chan, fin, resid, ln_w, ln_b, o, out, stats, b, C, L, drop, out_sums,
                                   nullptr, 0, nullptr, 1, nullptr, 1, nullptr, nullptr, stream);
}

extern "C" int bmnas_bn_relu_ln_bwd_pair(
    const float* g, const float* o, const float* resid, const float* ln_w, const float* stats, const float* U,
    const float* chan, float* dV, float* bn_grad, float* dresid, int accumulate_resid, int b, int C, int L,
    bmnas_dropout_t drop, const float* const* xs, float* const* dxs, int n_prev, uint32_t accumulate_mask,
    const float* out, const float* w, int w_stride, const float* w2, int w2_stride, const float* h,
    const float* gh, const float* gz, const float* gz2, float* dw, float* dw2, int dw_shards,
    int64_t dw_shard_stride, float* g_full, void* stream) {
  if ((n_prev == 0 && !g) || !o || !resid || !ln_w || !stats || !U || !chan || !dV || !bn_grad || b < 0 || C < 1)
    return BMNAS_E_ARG;
  PairPrevB P{};
  if (n_prev > 0) {
    if (!xs || !dxs || !out || !w || !w2 || !h || !gz || !dw || !dw2 || !g_full || w_stride < 1 || w2_stride < 1 ||
        dw_shards < 1)
      return BMNAS_E_ARG;
    if (!bmnas_bn_relu_ln_fwd_pair_ok(b > 0 ? b : 1, C, L, n_prev)) return BMNAS_E_LIMIT;
    if (int e = fill_ptrs(P.xs.p, xs, n_prev)) return e;
    fill_ptrs_out(P.dxs.p, dxs, n_prev);
    for (int j = 0; j < n_prev; ++j)
      for (int k = 0; k < j; ++k)
        if (dxs[j] != nullptr && dxs[j] == dxs[k]) return BMNAS_E_ARG;     // old values are fetched up front
    P.out = out; P.w = w; P.w2 = w2; P.h = h; P.gh = gh; P.gz = gz; P.gz2 = gz2; P.dw = dw; P.dw2 = dw2;
    P.g_full = g_full; P.dw_stride = dw_shard_stride; P.ws = w_stride; P.w2s = w2_stride;
    P.dw_shards = dw_shards; P.acc = accumulate_mask;
  } else if (n_prev < 0) {
    return BMNAS_E_ARG;
  }
  if (!len_bwd_ok(L)) return BMNAS_E_SHAPE;
  if (accumulate_resid && !dresid) return BMNAS_E_ARG;
  if (b == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const int e = n_prev > 0                                 // (host-checked: one float4 per lane, 256 lanes)
      ? dispatch_range<1, BMNAS_MAX_PTRS - 1>(n_prev, [&](auto NP) {
          hipLaunchKernelGGL((bn_relu_ln_bwd_k<1, 256, decltype(NP)::value>), dim3(b), dim3(256), 0, st, g, o, resid,
                             ln_w, stats, U, chan, dV, bn_grad, dresid, accumulate_resid, b, C, L, to_cfg(drop), P);
        })
      : dispatch_ln<1, 2, 3, 4, 8>(ln_launch_shape(b, C * L / 4), [&](auto V, auto BS) {
          hipLaunchKernelGGL((bn_relu_ln_bwd_k<decltype(V)::value, decltype(BS)::value>), dim3(b),
                             dim3(decltype(BS)::value), 0, st, g, o, resid, ln_w, stats, U, chan, dV, bn_grad, dresid,
                             accumulate_resid, b, C, L, to_cfg(drop), P);
        });
  if (e) return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_bn_relu_ln_bwd(const float* g, const float* o, const float* resid, const float* ln_w,
                                    const float* stats, const float* U, const float* chan, float* dV,
                                    float* bn_grad, float* dresid, int accumulate_resid, int b, int C,
                                    int L, bmnas_dropout_t drop, void* stream) {
  return bmnas_bn_relu_ln_bwd_pair(g, o, resid, ln_w, stats, U, chan, dV, bn_grad, dresid, accumulate_resid, b, C,
                                   L, drop, nullptr, nullptr, 0, 0, nullptr, nullptr, 1, nullptr, 1, nullptr,
                                   nullptr, nullptr, nullptr, nullptr, nullptr, 1, 0, nullptr, stream);
}

extern "C" int bmnas_bn_bwd_apply(float* dV, const float* U, const float* chan,
                                  const float* bn_grad, int b, int M, int L, int training,
                                  void* stream) {
  if (!dV || !U || !chan || !bn_grad || b < 0 || M < 1) return BMNAS_E_ARG;
  if (!len_fwd_ok(L)) return BMNAS_E_SHAPE;
  if (b == 0) return 0;
  const int64_t total = (int64_t)b * M * L / 4;
  hipLaunchKernelGGL(bn_bwd_apply_k, dim3(stream_grid(total)), dim3(256), 0, (hipStream_t)stream, dV,
                     U, chan, bn_grad, b, M, L, training);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_arch_softmax_fwd(const float* logits, float* w, int rows, int cols,
                                      void* stream) {
  if (!logits || !w || rows < 1 || cols < 1) return BMNAS_E_ARG;
  hipLaunchKernelGGL(arch_softmax_fwd_k, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream,
                     logits, w, rows, cols);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_arch_softmax_bwd(const float* w, const float* dw, float* dlogits, int rows,
                                      int cols, void* stream) {
  if (!w || !dw || !dlogits || rows < 1 || cols < 1) return BMNAS_E_ARG;
  hipLaunchKernelGGL(arch_softmax_bwd_k, dim3((rows + 63) / 64), dim3(64), 0, (hipStream_t)stream, w,
                     dw, dlogits, rows, cols);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_arch_softmax_multi(const float* const* a, const float* const* dw,
                                        float* const* out, const int* rows, const int* cols, int n,
                                        int backward, int n_shards, int64_t shard_stride,
                                        void* stream) {
  ArchPack P{};
  const int total = fill_arch_pack(P, a, dw, out, rows, cols, n, backward, n_shards, shard_stride);
  if (total < 0) return total;
  if (backward) {
    hipLaunchKernelGGL(arch_softmax_multi_bwd_k, dim3(total), dim3(64), 0, (hipStream_t)stream, P);
    BMNAS_CHECK_LAUNCH();
    return 0;
  }
  hipLaunchKernelGGL(arch_softmax_multi_k, dim3((total + 63) / 64), dim3(64), 0, (hipStream_t)stream, P,
                     backward);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

namespace {
struct PrologueLaunch {
  ArchPack P;
  FoldPack F;
  int blocks;
};

int fill_prologue(PrologueLaunch& L, const float* const* a, float* const* out, const int* rows, const int* cols,
                  int n_arch, const float* const* W, float* const* Weff, int n_fold, int M, int C,
                  const uint64_t* step_counter, const uint64_t* step_span, const float* scrub, int64_t scrub_n) {
  if ((step_counter == nullptr) != (step_span == nullptr)) return BMNAS_E_ARG;
  if (scrub_n < 0 || (scrub_n > 0 && !scrub) || scrub_n % 4) return BMNAS_E_ARG;
  if (n_arch < 0 || n_fold < 0 || (n_arch > 0 && (!a || !out || !rows || !cols)) ||
      (n_fold > 0 && (!W || !Weff || M < 1 || C < 1)))
    return BMNAS_E_ARG;
  if (n_arch > BMNAS_MAX_PTRS || n_fold > kMaxFold) return BMNAS_E_LIMIT;
  if (n_fold > 0 && C % 4) return BMNAS_E_SHAPE;
  L.P = ArchPack{};
  int total = 0;
  for (int t = 0; t < n_arch; ++t) {
    if (!a[t] || !out[t] || rows[t] < 1 || cols[t] < 1 || cols[t] > 4) return BMNAS_E_ARG;
    L.P.a[t] = a[t];
    L.P.o[t] = out[t];
    L.P.rows[t] = rows[t];
    L.P.cols[t] = cols[t];
    total += rows[t];
  }
  L.P.n = n_arch;
  L.P.n_shards = 1;
  L.F = FoldPack{};
  for (int q = 0; q < n_fold; ++q) {
    if (!W[q] || !Weff[q]) return BMNAS_E_ARG;
    L.F.W[q] = W[q];
    L.F.Weff[q] = Weff[q];
  }
  L.F.n = n_fold; L.F.M = M; L.F.C = C;
  int per = n_fold > 0 ? (int)(((int64_t)M * (C / 4) + 255) / 256) : 0;
  if (per > 128) per = 128;
  L.F.blocks_per = per;
  L.blocks = n_fold * per + (total + 255) / 256;
  if (L.blocks == 0 && (step_counter != nullptr || scrub_n > 0)) L.blocks = 1;
  return 0;
}
}  // namespace

extern "C" int bmnas_cell_prologue(const float* const* a, float* const* out, const int* rows,
                                   const int* cols, int n_arch, const float* const* W,
                                   float* const* Weff, int n_fold, int M, int C,
                                   uint64_t* step_counter, const uint64_t* step_span, float* scrub,
                                   int64_t scrub_n, void* stream) {
  PrologueLaunch L;
  if (int e = fill_prologue(L, a, out, rows, cols, n_arch, W, Weff, n_fold, M, C, step_counter, step_span, scrub,
                            scrub_n))
    return e;
  if (L.blocks == 0) return 0;
  // a large zero-fill (the reshape group's accumulation buffers: ~2 MB) wants more than the few softmax / fold
  // workgroups: one per 4 KB, at most two per CU
  if (scrub_n > 0) L.blocks = std::max(L.blocks, (int)std::min<int64_t>(512, (scrub_n / 4 + 255) / 256));
  hipLaunchKernelGGL(cell_prologue_k, dim3(L.blocks), dim3(256), 0, (hipStream_t)stream, L.P, L.F,
                     (unsigned long long*)step_counter, (const unsigned long long*)step_span, scrub,
                     scrub_n / 4);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_cell_prologue_pair(const float* const* a, float* const* out, const int* rows,
                                        const int* cols, int n_arch, const float* const* W,
                                        float* const* Weff, int n_fold, int M, int C,
                                        uint64_t* step_counter, const uint64_t* step_span, float* scrub,
                                        int64_t scrub_n, const float* const* xs, int n_in,
                                        const float* alpha_logits, const float* beta_logits, float* h,
                                        float* z, int64_t n_elem, void* stream) {
  PrologueLaunch L;
  if (int e = fill_prologue(L, a, out, rows, cols, n_arch, W, Weff, n_fold, M, C, step_counter, step_span, scrub,
                            scrub_n))
    return e;
  if (!xs || !alpha_logits || !beta_logits || !h || !z || n_in < 1 || n_elem < 0) return BMNAS_E_ARG;
  if (n_in > BMNAS_MAX_PTRS - 1) return BMNAS_E_LIMIT;
  if (n_elem % 4) return BMNAS_E_SHAPE;
  PairArgs A{};
  if (int e = fill_ptrs(A.xs.p, xs, n_in)) return e;
  A.alpha = alpha_logits; A.beta = beta_logits; A.out = h; A.out2 = z; A.n4 = n_elem / 4;
  // one float4 per lane and input: the pair sum is a latency-floor kernel at the reference batches
  int64_t pair_blocks = (A.n4 + 255) / 256;                   // (0 at n_elem == 0: the prologue alone)
  if (pair_blocks > 2048) pair_blocks = 2048;                 // as bmnas_mixsum_pair_fwd
  if (L.blocks + pair_blocks == 0) return 0;
  dim3 grid((unsigned)(L.blocks + pair_blocks));
  hipStream_t st = (hipStream_t)stream;
  if (int e = dispatch_range<1, BMNAS_MAX_PTRS - 1>(n_in, [&](auto N) {
        hipLaunchKernelGGL(cell_prologue_pair_k<decltype(N)::value>, grid, dim3(256), 0, st, L.P, L.F,
                           (unsigned long long*)step_counter, (const unsigned long long*)step_span, scrub,
                           scrub_n / 4, L.blocks, A);
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}
