// The gamma-weighted NodeMixedOp combine for an EDITED STEP_STEP_PRIMITIVES list: any non-empty subset of
// {Sum, ScaleDotAttn, LinearGLU, ConcatFC}, in any order (reference models/search/darts/node_operations.py:110-120,
// `sum(w * op(x, y) for w, op in zip(weights, self._ops))`).
//
//   s = sum_{p present} gamma[col(p)] * term_p,   term_Sum = x + y,  term_Attn = p1,
//       term_GLU = drop(glu(BN(U[:, glu rows]))),  term_FC = drop(relu(BN(U[:, fc rows])))
//
// The arithmetic is mix_fwd4 / mix_bwd4 of mix_terms.hpp, which node_mix_fwd_k / node_mix_bwd_k (bnmix.hip) compile for
// the default list (mask 15); here the kernels are specialised at compile time on the presence mask (bit 0 Sum,
// 1 ScaleDotAttn, 2 LinearGLU, 3 ConcatFC), so that an
// absent term costs no load, no store, no reduction and no LDS, and U holds only the present conv rows
// (M = 2C [GLU] + C [FC], GLU rows first).  Which gamma column belongs to which kind comes with the launch (Sel).
//
// CatConvMish (reference node_operations.py:58-82: cat -> Conv1d(2C, C, 1) -> BatchNorm1d -> Mish -> Dropout) is ConcatFC
// with another activation: it takes ConcatFC's slot (bit 3, the C rows behind the GLU rows, col[3], drop_fc) and the
// kernels' second template parameter ACT = kActMish, instantiated for the 8 masks that hold bit 3.
#include "common.hpp"
#include "../../include/bmnas_hip.h"
#include "bn_fin.hpp"
#include "mix_common.hpp"

namespace {

struct Sel {
  int col[4];      // gamma column of Sum | ScaleDotAttn | LinearGLU | ConcatFC (unused where absent)
};

template <int MASK, int ACT>
__global__ __launch_bounds__(256) void node_mix_sel_fwd_k(
    const float* __restrict__ x, const float* __restrict__ y, const float* __restrict__ p1,
    const float* __restrict__ U, float* __restrict__ chan, BnFin fin, const float* __restrict__ gamma, Sel sel,
    float* __restrict__ out, int b, int C, int L, DropCfg dglu, DropCfg dfc) {
  constexpr bool hS = MASK & kSum, hA = MASK & kAttn, hG = MASK & kGlu, hF = MASK & kFc;
  constexpr int MC = MixRows<MASK>::kMc, FO = MixRows<MASK>::kFo;      // U rows / C; first ConcatFC row / C
  extern __shared__ float fin_lds[];
  const int cl4 = C * L / 4, l4n = L / 4, M = MC * C;
  float* sc = fin_lds;
  float* sh = fin_lds + M;
  DropRt rglu{}, rfc{};
  if constexpr (hG) rglu = drop_begin(dglu);
  if constexpr (hF) rfc = drop_begin(dfc);
  if constexpr (MC > 0) bn_fin_fill<256>(fin, chan, M, b * L, sc, sh, blockIdx.x == 0);
  float gS = 0.f, gA = 0.f, gG = 0.f, gF = 0.f;
  if constexpr (hS) gS = gamma[sel.col[0]];
  if constexpr (hA) gA = gamma[sel.col[1]];
  if constexpr (hG) gG = gamma[sel.col[2]];
  if constexpr (hF) gF = gamma[sel.col[3]];
  const int64_t total = (int64_t)b * cl4;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int s = (int)(i / cl4);
    const int r = (int)(i - (int64_t)s * cl4);
    const int c = r / l4n;
    const int64_t e = i * 4;
    const int64_t ub = ((int64_t)s * M) * L + (int64_t)r * 4;      // (s, c, l) inside U's first C block
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 xy = zero, pv = zero, va = zero, vg = zero, vf = zero, m2 = zero, m3 = zero;
    if constexpr (hS) xy = f4_add(ld4(x + e), ld4(y + e));
    if constexpr (hA) pv = ld4(p1 + e);
    if constexpr (hG) {
      va = affine4(ld4(U + ub), sc[c], sh[c]);
      vg = affine4(ld4(U + ub + (int64_t)C * L), sc[C + c], sh[C + c]);
      m2 = drop_mult4(rglu, (uint64_t)e);
    }
    if constexpr (hF) {
      vf = affine4(ld4(U + ub + (int64_t)FO * C * L), sc[FO * C + c], sh[FO * C + c]);
      m3 = drop_mult4(rfc, (uint64_t)e);
    }
    st4_wtg<2>(out + e, mix_fwd4<MASK, ACT>(gS, gA, gG, gF, xy, pv, va, vg, vf, m2, m3));
  }
}


// Phase A of the backward, as node_mix_bwd_k: a thread owns one float4 slot of a sample's (C, L) tile and walks a chunk
// of samples (4 sample lanes per slot), so the per-channel BatchNorm sums and the dgamma sums stay in registers.
template <int MASK, int ACT>
__global__ __launch_bounds__(256) void node_mix_sel_bwd_k(
    const float* __restrict__ g, const float* __restrict__ x, const float* __restrict__ y,
    const float* __restrict__ p1, const float* __restrict__ U, const float* __restrict__ chan,
    const float* __restrict__ gamma, Sel sel, float* dgamma, int dg_shards, int64_t dg_stride, float* dx, float* dy,
    uint32_t acc_mask, float* __restrict__ dV, float* bn_grad, int b, int C, int L, int chunk, DropCfg dglu,
    DropCfg dfc) {
  constexpr bool hS = MASK & kSum, hA = MASK & kAttn, hG = MASK & kGlu, hF = MASK & kFc;
  constexpr int MC = MixRows<MASK>::kMc, FO = MixRows<MASK>::kFo;
  constexpr int NB = MixRows<MASK>::kNb;               // (array extents; nothing of them is touched when MC == 0)
  __shared__ float red16[16];
  __shared__ float csum[3][2 * NB][64];
  const int cl4 = C * L / 4, l4n = L / 4, M = MC * C;
  const int col = threadIdx.x & 63, sl = threadIdx.x >> 6;   // 64 slots x 4 sample lanes
  const int r = blockIdx.x * 64 + col;               // float4 slot inside one sample's (C, L) tile
  const bool active = r < cl4;
  const int c = active ? r / l4n : 0;
  float gS = 0.f, gG = 0.f, gF = 0.f;
  if constexpr (hS) gS = gamma[sel.col[0]];
  if constexpr (hG) gG = gamma[sel.col[2]];
  if constexpr (hF) gF = gamma[sel.col[3]];
  DropRt rglu{}, rfc{};
  if constexpr (hG) rglu = drop_begin(dglu);
  if constexpr (hF) rfc = drop_begin(dfc);
  ChanBn<NB> bn{};
  if constexpr (MC > 0) bn = chan_load<NB>(chan, M, C, c);
  float sw[NB] = {}, sb[NB] = {};
  float dgam[4] = {0.f, 0.f, 0.f, 0.f};
  const int s_beg = blockIdx.y * chunk;
  int s_end = s_beg + chunk;
  if (s_end > b) s_end = b;
  if (active) {
    for (int s = s_beg + sl; s < s_end; s += 4) {
      const int64_t e = ((int64_t)s * cl4 + r) * 4;
      const int64_t ub = ((int64_t)s * M) * L + (int64_t)r * 4;
      const float4 gv = ld4(g + e);
      const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
      float4 xy = zero, pv = zero, ua = zero, ug = zero, uf = zero, m2 = zero, m3 = zero;
      if constexpr (hS) xy = f4_add(ld4(x + e), ld4(y + e));
      if constexpr (hA) pv = ld4(p1 + e);
      if constexpr (hG) {
        ua = ld4(U + ub);
        ug = ld4(U + ub + (int64_t)C * L);
        m2 = drop_mult4(rglu, (uint64_t)e);
      }
      if constexpr (hF) {
        uf = ld4(U + ub + (int64_t)FO * C * L);
        m3 = drop_mult4(rfc, (uint64_t)e);
      }
      float4 da, dg, df;
      mix_bwd4<MASK, ACT>(gG, gF, gv, xy, pv, ua, ug, uf, m2, m3, bn, dgam, da, dg, df, sw, sb);
      if constexpr (hG) {
        st4_wtg<2>(dV + ub, da);
        st4_wtg<2>(dV + ub + (int64_t)C * L, dg);
      }
      if constexpr (hF) st4_wtg<2>(dV + ub + (int64_t)FO * C * L, df);
      if constexpr (hS) {
        mix_dxy_store([](float* p, float4 v) { st4_wtg<2>(p, v); }, dx, dy, e, gv, gS, acc_mask);
      } else {
        // no Sum term: this launch contributes nothing to dx / dy — a destination that nobody wrote yet is
        // cleared, so that the conv / attention gradients behind it can accumulate
        if (dx != nullptr && !(acc_mask & 1u)) st4_wtg<2>(dx + e, zero);
        if (dy != nullptr && !(acc_mask & 2u)) st4_wtg<2>(dy + e, zero);
      }
    }
  }
  // per-channel batch sums -> BatchNorm affine gradients: over the l4 lanes of a channel row (shuffles), over the
  // 4 sample lanes (LDS, behind the same barrier as the dgamma sums), then one atomic per channel
  float cs[2 * NB];
  if constexpr (MC > 0) {
#pragma unroll
    for (int k = 0; k < MC; ++k) {
      cs[k] = row_sum(sw[k], l4n);
      cs[MC + k] = row_sum(sb[k], l4n);
    }
    if (sl > 0) {
#pragma unroll
      for (int k = 0; k < 2 * MC; ++k) csum[sl - 1][k][col] = cs[k];
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (MASK & (1 << q)) {
      dgam[q] = wave_sum(dgam[q]);
      if (col == 0) red16[q * 4 + sl] = dgam[q];
    }
  }
  __syncthreads();
  if constexpr (MC > 0) {
    if (sl == 0 && active && (r % l4n) == 0) {
#pragma unroll
      for (int k = 0; k < 2 * MC; ++k) cs[k] += csum[0][k][col] + csum[1][k][col] + csum[2][k][col];
#pragma unroll
      for (int k = 0; k < MC; ++k) {
        atomicAdd(bn_grad + k * C + c, cs[k]);
        atomicAdd(bn_grad + M + k * C + c, cs[MC + k]);
      }
    }
  }
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (threadIdx.x >= 64 && threadIdx.x < 68 && dgamma != nullptr) {      // (wave 1: wave 0's lanes are busy above)
    const int q = threadIdx.x - 64;
    if (MASK & (1 << q))
      atomicAdd(dgamma + (int64_t)(wg % dg_shards) * dg_stride + sel.col[q],
                ((red16[q * 4] + red16[q * 4 + 1]) + red16[q * 4 + 2]) + red16[q * 4 + 3]);
  }
}

// -> presence mask, or < 0: every present kind has its own column in [0, n), n = number of present kinds
int sel_mask(const bmnas_node_sel_t& s, Sel* out) {
  if (s.n < 1 || s.n > 4) return BMNAS_E_ARG;
  int mask = 0, cols = 0, cnt = 0;
  for (int k = 0; k < 4; ++k) {
    out->col[k] = 0;
    const int c = s.col[k];
    if (c < 0) continue;
    if (c >= s.n || (cols & (1 << c))) return BMNAS_E_ARG;
    cols |= 1 << c;
    mask |= 1 << k;
    out->col[k] = c;
    ++cnt;
  }
  if (cnt != s.n) return BMNAS_E_ARG;
  return mask;
}

inline int sel_rows(int mask) { return ((mask & kGlu) ? 2 : 0) + ((mask & kFc) ? 1 : 0); }

}  // namespace

extern "C" int bmnas_node_mix_sel_ok(int mask, int b, int C, int L) {
  if (mask < 1 || mask > 15 || b < 1 || C < 1 || L < 4 || L % 4) return 0;
  const bool attn = mask & kAttn, conv = mask & (kGlu | kFc);
  // the attention kernels and the conv GEMMs tile 16 (sample, l) columns and 16 channels; the BatchNorm row
  // reductions of the backward walk L / 4 in {1, 2, 4} adjacent lanes
  if ((attn || conv) && !len_bwd_ok(L)) return 0;
  if ((attn || conv) && C % 16) return 0;
  if (attn && C > 512) return 0;
  if (conv && sel_rows(mask) * C > 4096) return 0;        // scale | shift of every conv row sit in LDS
  return 1;
}

// f(int_c<mask>, int_c<fc_act>) for the 23 instantiated pairs — ReLU: all 15 masks; Mish: the 8 masks with the FC slot
template <class F>
static int dispatch_sel(int mask, int fc_act, F&& f) {
  const int e = fc_act != kActMish ? dispatch_range<1, 15>(mask, [&](auto M) { f(M, int_c<kActRelu>{}); })
                                   : dispatch_range<8, 15>(mask, [&](auto M) { f(M, int_c<kActMish>{}); });
  return e ? BMNAS_E_ARG : 0;
}

extern "C" int bmnas_node_mix_sel_act_fwd(const float* x, const float* y, const float* p1, const float* U,
                                          float* chan, bmnas_bn_fin_t fin, const float* gamma, bmnas_node_sel_t sel,
                                          float* out, int b, int C, int L, bmnas_dropout_t drop_glu,
                                          bmnas_dropout_t drop_fc, int fc_act, void* stream) {
  Sel s;
  const int mask = sel_mask(sel, &s);
  if (mask < 0) return mask;
  if (fc_act != kActRelu && fc_act != kActMish) return BMNAS_E_ARG;
  if (!(mask & kFc)) fc_act = kActRelu;                   // no FC slot: nothing to activate
  if (!gamma || !out || b < 0 || C < 1) return BMNAS_E_ARG;
  if (!bmnas_node_mix_sel_ok(mask, b > 0 ? b : 1, C, L)) return BMNAS_E_LIMIT;
  const int M = sel_rows(mask) * C;
  if ((mask & kSum) && (!x || !y)) return BMNAS_E_ARG;
  if ((mask & kAttn) && !p1) return BMNAS_E_ARG;
  if (M > 0 && (!U || !chan)) return BMNAS_E_ARG;
  BnFin f{};
  if (M > 0) {
    if (int e = fin_for(fin, b, L, &f)) return e;
  }
  if (b == 0) return 0;
  const int64_t total = (int64_t)b * C * L / 4;
  if (int e = dispatch_sel(mask, fc_act, [&](auto Mk, auto Act) {
        hipLaunchKernelGGL((node_mix_sel_fwd_k<decltype(Mk)::value, decltype(Act)::value>), dim3(stream_grid(total)),
                           dim3(256), (size_t)2 * M * sizeof(float), (hipStream_t)stream, x, y, p1, U, chan, f, gamma,
                           s, out, b, C, L, to_cfg(drop_glu), to_cfg(drop_fc));
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_node_mix_sel_fwd(const float* x, const float* y, const float* p1, const float* U, float* chan,
                                      bmnas_bn_fin_t fin, const float* gamma, bmnas_node_sel_t sel, float* out,
                                      int b, int C, int L, bmnas_dropout_t drop_glu, bmnas_dropout_t drop_fc,
                                      void* stream) {
  return bmnas_node_mix_sel_act_fwd(x, y, p1, U, chan, fin, gamma, sel, out, b, C, L, drop_glu, drop_fc, kActRelu,
                                    stream);
}

extern "C" int bmnas_node_mix_sel_act_bwd(const float* g, const float* x, const float* y, const float* p1,
                                          const float* U, const float* chan, const float* gamma,
                                          bmnas_node_sel_t sel, float* dgamma, int dgamma_shards,
                                          int64_t dgamma_shard_stride, float* dx, float* dy,
                                          uint32_t accumulate_mask, float* dV, float* bn_grad, int b, int C, int L,
                                          bmnas_dropout_t drop_glu, bmnas_dropout_t drop_fc, int fc_act,
                                          void* stream) {
  Sel s;
  const int mask = sel_mask(sel, &s);
  if (mask < 0) return mask;
  if (fc_act != kActRelu && fc_act != kActMish) return BMNAS_E_ARG;
  if (!(mask & kFc)) fc_act = kActRelu;
  if (!g || !gamma || b < 0 || C < 1 || dgamma_shards < 1) return BMNAS_E_ARG;
  if (!bmnas_node_mix_sel_ok(mask, b > 0 ? b : 1, C, L)) return BMNAS_E_LIMIT;
  const int M = sel_rows(mask) * C;
  if ((mask & kSum) && (!x || !y)) return BMNAS_E_ARG;
  if ((mask & kAttn) && !p1) return BMNAS_E_ARG;
  if (M > 0 && (!U || !chan || !dV || !bn_grad)) return BMNAS_E_ARG;
  if (b == 0) return 0;
  const int cl4 = C * L / 4;
  const int chunk = pick_chunk(b, cl4);
  dim3 grid((cl4 + 63) / 64, (b + chunk - 1) / chunk);
  if (int e = dispatch_sel(mask, fc_act, [&](auto Mk, auto Act) {
        hipLaunchKernelGGL((node_mix_sel_bwd_k<decltype(Mk)::value, decltype(Act)::value>), grid, dim3(256), 0,
                           (hipStream_t)stream, g, x, y, p1, U, chan, gamma, s, dgamma, dgamma_shards,
                           dgamma_shard_stride, dx, dy, accumulate_mask, dV, bn_grad, b, C, L, chunk, to_cfg(drop_glu),
                           to_cfg(drop_fc));
      }))
    return e;
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_node_mix_sel_bwd(const float* g, const float* x, const float* y, const float* p1,
                                      const float* U, const float* chan, const float* gamma, bmnas_node_sel_t sel,
                                      float* dgamma, int dgamma_shards, int64_t dgamma_shard_stride, float* dx,
                                      float* dy, uint32_t accumulate_mask, float* dV, float* bn_grad, int b, int C,
                                      int L, bmnas_dropout_t drop_glu, bmnas_dropout_t drop_fc, void* stream) {
  return bmnas_node_mix_sel_act_bwd(g, x, y, p1, U, chan, gamma, sel, dgamma, dgamma_shards, dgamma_shard_stride, dx,
                                    dy, accumulate_mask, dV, bn_grad, b, C, L, drop_glu, drop_fc, kActRelu, stream);
}
