// Multi-head attention core (the part of nn.MultiheadAttention between its in_proj and out_proj GEMMs), forward
// and backward, for the Attention / MultiHeadAttn fusion primitive (reference models/search/darts/operations.py:67-86).
// The projections themselves are bmnas_conv1x1_* launches; this file only sees projected (b, C, L) operands, given
// by pointer + sample stride, so that q / k / v may be row ranges of one stacked GEMM output.
//
// Decomposition.  A (sample, head) problem is an L x L score matrix over a contraction of d = C / heads channels,
// L <= 16: far too small for a workgroup, and with b * heads of them a launch is latency bound (d = 96 at
// MM-IMDB is 24 MFMA k-steps).  16 / L problems are packed on the 16-wide MFMA dimension of one "tile" (a
// block-diagonal mask keeps them apart), so that at L = 4 every lane still loads a useful operand element: the packed
// tile of attn_tile.hpp, whose per-lane arithmetic (contraction over channels, masked softmax and its backward, product
// over positions) this file shares with the ScaleDotAttn bodies of sdpa_body.hpp.  Unlike there, ONE WAVE owns a tile
// end to end (the channel contraction is d, not C: splitting it over four waves would buy 6 k-steps per wave at the
// price of an LDS reduction and two barriers) and a 256-thread workgroup carries four independent tiles.  Problem
// p = s * heads + a lives at channel offset a * d of sample s; row r of a tile is (problem tile * spw + (r >> Lb),
// position r & (L - 1)).
//   S^T[j][i] = sum_c K[c][j] Q[c][i]     contract_channels: dword operand loads straight from global
//   P = softmax_j(S / sqrt(d))            tile_softmax: a lane holds S[i = lane & 15][j = 4 (lane >> 4) + r]
//   O[c][i] = sum_j P'[i][j] V[c][j]      tile_apply per 16-channel chunk: V as float4 along l, O leaves as float4 along l
// The backward runs the same two shapes of product: dP like S (over channels), dV / dQ / dK like O (over positions),
// with P' and dS transposed through a wave-private 16 x 17 LDS image.  No atomics, no cross-wave reduction: every
// output element has one writer and one summation order, so the results are bit-stable from run to run.
#include "attn_tile.hpp"
#include "drop_cfg.hpp"

namespace {

constexpr int kMhaWaves = 4;                                   // tiles per workgroup

struct MhaGeom {
  int b, C, L, Lb, spw, heads, d;
  int np;                 // problems = b * heads
  int tiles;              // ceil(np / spw)
  float inv;              // 1 / sqrt(d)
};

struct MhaOperand {       // a projected (b, C, L) tensor: sample s at p + s * ss
  const float* p;
  int64_t ss;
};
struct MhaResult {
  float* p;
  int64_t ss;
};

// float offset of channel 0 / position 0 of problem p inside an operand
__device__ __forceinline__ int64_t prob_off(const MhaGeom& G, int p, int64_t ss) {
  const int s = p / G.heads, a = p - s * G.heads;
  return (int64_t)s * ss + (int64_t)a * G.d * G.L;
}

// What a lane is, in a tile
struct MhaLane {
  int lo, h;
  int p_lo, pos_lo;       // row lo: problem (clamped) and position
  int p_h, l0;            // rows 4h .. 4h + 3: problem (clamped) and first position
  bool v_lo, v_h;         // ... is a real problem
  bool same;              // rows lo and 4h.. belong to one problem
  int64_t pe;             // flat element of P[p_lo][pos_lo][l0] (4 consecutive j)
};

__device__ __forceinline__ MhaLane mha_lane(const MhaGeom& G, int tile, int lane) {
  MhaLane m;
  m.lo = lane & 15; m.h = lane >> 4;
  const int last = G.np - 1;
  // rows of padded problems (the ragged last tile, a workgroup's spare waves) read the last real problem — clamped
  // addresses, no predicated loads — and store nothing
  const int p_lo = tile * G.spw + (m.lo >> G.Lb);
  const int p_h = tile * G.spw + ((4 * m.h) >> G.Lb);
  m.v_lo = p_lo <= last; m.v_h = p_h <= last;
  m.p_lo = m.v_lo ? p_lo : last;
  m.p_h = m.v_h ? p_h : last;
  m.pos_lo = m.lo & (G.L - 1);
  m.l0 = (4 * m.h) & (G.L - 1);
  m.same = p_lo == p_h;
  m.pe = ((int64_t)m.p_lo * G.L + m.pos_lo) * G.L + m.l0;
  return m;
}

__global__ __launch_bounds__(64 * kMhaWaves) void mha_core_fwd_k(MhaOperand q, MhaOperand k, MhaOperand v,
                                                                 float* __restrict__ O, float* __restrict__ P,
                                                                 MhaGeom G, DropCfg drop) {
  const DropRt drop_rt = drop_begin(drop);          // the step counter's load goes out first
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int tile = blockIdx.x * kMhaWaves + wave;
  if (tile >= G.tiles) return;                      // (no barrier in this kernel: a spare wave may leave)
  const MhaLane m = mha_lane(G, tile, lane);

  float raw[4], p[4];
  contract_channels(k.p + prob_off(G, m.p_lo, k.ss) + m.pos_lo, q.p + prob_off(G, m.p_lo, q.ss) + m.pos_lo, 0,
                    G.d >> 2, G.L, m.h, raw);
  // lane holds S[i = lo][j = 4h + r]; keep only the j of the problem of row i
  tile_softmax(raw, G.inv, m.same, p);
  if (m.same && m.v_lo) {
    st4(P + m.pe, make_float4(p[0], p[1], p[2], p[3]));                    // saved BEFORE dropout
    const float4 dm = drop_mult4(drop_rt, (uint64_t)m.pe);
    p[0] *= dm.x; p[1] *= dm.y; p[2] *= dm.z; p[3] *= dm.w;
  }

  // O[c][i] = sum_j P'[i][j] V[c][j], 16 channels of the head at a time (lane lo = channel, regs = positions i)
  const float* vb = v.p + prob_off(G, m.p_h, v.ss) + m.l0;
  float* ob = O + prob_off(G, m.p_h, (int64_t)G.C * G.L) + m.l0;
  const int nch = (G.d + 15) >> 4;
#pragma unroll 2
  for (int ch = 0; ch < nch; ++ch) {
    const int c = ch * 16 + m.lo;
    const bool vc = c < G.d;
    const int cc = vc ? c : G.d - 1;
    const float4 vv = ld4(vb + (int64_t)cc * G.L);
    const f32x4 o = tile_apply(p, vv, f32x4{0.f, 0.f, 0.f, 0.f});
    if (vc && m.v_h) st4(ob + (int64_t)c * G.L, make_float4(o[0], o[1], o[2], o[3]));
  }
}

__global__ __launch_bounds__(64 * kMhaWaves) void mha_core_bwd_k(const float* __restrict__ dO, MhaOperand q,
                                                                 MhaOperand k, MhaOperand v,
                                                                 const float* __restrict__ P, MhaResult dq,
                                                                 MhaResult dk, MhaResult dv, MhaGeom G,
                                                                 DropCfg drop) {
  const DropRt drop_rt = drop_begin(drop);          // the step counter's load goes out first
  __shared__ float tr[kMhaWaves][2][16 * 17];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  // a spare wave (tile >= G.tiles) walks through on clamped addresses — the barrier below is for all four — and
  // stores nothing
  const int tile = blockIdx.x * kMhaWaves + wave;
  const MhaLane m = mha_lane(G, tile, lane);
  const int64_t oss = (int64_t)G.C * G.L;           // dO is contiguous

  // P and its dropout multipliers
  float p[4] = {0.f, 0.f, 0.f, 0.f}, pm[4] = {0.f, 0.f, 0.f, 0.f};
  if (m.same) {                                     // (clamped p_lo: a padded row loads a real row, stores nothing)
    const float4 pv = ld4(P + m.pe);
    const float4 dm = drop_mult4(drop_rt, (uint64_t)m.pe);
    p[0] = pv.x; p[1] = pv.y; p[2] = pv.z; p[3] = pv.w;
    pm[0] = dm.x; pm[1] = dm.y; pm[2] = dm.z; pm[3] = dm.w;
  }
  // dP[i = lo][j = 4h + r] = mask * sum_c dO[c][i] V[c][j]
  float dP[4];
  contract_channels(v.p + prob_off(G, m.p_lo, v.ss) + m.pos_lo, dO + prob_off(G, m.p_lo, oss) + m.pos_lo, 0,
                    G.d >> 2, G.L, m.h, dP);
  float ds[4], pd[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    dP[r] *= pm[r];
    pd[r] = p[r] * pm[r];                           // P'
  }
  tile_softmax_bwd(p, dP, G.inv, ds);               // dS / sqrt(d): what dQ and dK contract with
  // (the transposes stay written out, as in sdpa_bwd_body: see the note there)
  float* tP = tr[wave][0];
  float* tS = tr[wave][1];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    tP[m.lo * 17 + 4 * m.h + r] = pd[r];
    tS[m.lo * 17 + 4 * m.h + r] = ds[r];
  }
  __syncthreads();
  float pw[4], dsw[4];                              // P'[i = 4h + r][j = lo], dS[i = 4h + r][j = lo]
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    pw[r] = tP[(4 * m.h + r) * 17 + m.lo];
    dsw[r] = tS[(4 * m.h + r) * 17 + m.lo];
  }

  const int64_t qo = prob_off(G, m.p_h, q.ss) + m.l0, ko = prob_off(G, m.p_h, k.ss) + m.l0;
  const int64_t vo = prob_off(G, m.p_h, dv.ss) + m.l0, go = prob_off(G, m.p_h, oss) + m.l0;
  const int64_t dqo = prob_off(G, m.p_h, dq.ss) + m.l0, dko = prob_off(G, m.p_h, dk.ss) + m.l0;
  const bool live = m.v_h && tile < G.tiles;
  const int nch = (G.d + 15) >> 4;
#pragma unroll 2
  for (int ch = 0; ch < nch; ++ch) {
    const int c = ch * 16 + m.lo;
    const bool vc = c < G.d;
    const int64_t co = (int64_t)(vc ? c : G.d - 1) * G.L;
    const float4 gv = ld4(dO + go + co), kv = ld4(k.p + ko + co), qv = ld4(q.p + qo + co);
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    const f32x4 av = tile_apply(pw, gv, zero);      // dV[c][j] = sum_i P'[i][j] dO[c][i]
    const f32x4 aq = tile_apply(ds, kv, zero);      // dQ[c][i] = sum_j dS[i][j] K[c][j]
    const f32x4 ak = tile_apply(dsw, qv, zero);     // dK[c][j] = sum_i dS[i][j] Q[c][i]
    if (vc && live) {
      st4(dv.p + vo + co, make_float4(av[0], av[1], av[2], av[3]));
      st4(dq.p + dqo + co, make_float4(aq[0], aq[1], aq[2], aq[3]));
      st4(dk.p + dko + co, make_float4(ak[0], ak[1], ak[2], ak[3]));
    }
  }
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

inline int mha_geom(int b, int C, int L, int heads, MhaGeom* G) {
  if (!bmnas_mha_ok(b, C, L, heads)) return BMNAS_E_LIMIT;
  G->b = b; G->C = C; G->L = L; G->Lb = ilog2_exact(L); G->spw = 16 / L; G->heads = heads; G->d = C / heads;
  G->np = b * heads;
  G->tiles = (G->np + G->spw - 1) / G->spw;
  G->inv = 1.f / sqrtf((float)G->d);
  return 0;
}

}  // namespace

extern "C" int bmnas_mha_ok(int b, int C, int L, int heads) {
  if (b < 1 || heads < 1 || !(L == 4 || L == 8 || L == 16)) return 0;
  if (C < 16 || C > 512 || C % 16 != 0 || C % heads != 0 || (C / heads) % 4 != 0) return 0;
  if ((int64_t)b * heads > (int64_t)1 << 24) return 0;          // problem and tile counts stay far inside an int
  return 1;
}

extern "C" int bmnas_mha_core_fwd(const float* q, const float* k, const float* v, int64_t q_ss, int64_t k_ss,
                                  int64_t v_ss, float* O, float* P, int b, int C, int L, int heads,
                                  bmnas_dropout_t drop, void* stream) {
  if (!q || !k || !v || !O || !P) return BMNAS_E_ARG;
  MhaGeom G;
  if (int e = mha_geom(b, C, L, heads, &G)) return e;
  const int64_t row = (int64_t)C * L;
  if (q_ss < row || k_ss < row || v_ss < row || (q_ss | k_ss | v_ss) % 4 != 0) return BMNAS_E_ARG;
  if (!aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(O) || !aligned16(P)) return BMNAS_E_ARG;
  const int groups = (G.tiles + kMhaWaves - 1) / kMhaWaves;
  hipLaunchKernelGGL(mha_core_fwd_k, dim3(groups), dim3(64 * kMhaWaves), 0, (hipStream_t)stream, MhaOperand{q, q_ss},
                     MhaOperand{k, k_ss}, MhaOperand{v, v_ss}, O, P, G, to_cfg(drop));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_mha_core_bwd(const float* dO, const float* q, const float* k, const float* v, int64_t q_ss,
                                  int64_t k_ss, int64_t v_ss, const float* P, float* dq, float* dk, float* dv,
                                  int64_t dq_ss, int64_t dk_ss, int64_t dv_ss, int b, int C, int L, int heads,
                                  bmnas_dropout_t drop, void* stream) {
  if (!dO || !q || !k || !v || !P || !dq || !dk || !dv) return BMNAS_E_ARG;
  MhaGeom G;
  if (int e = mha_geom(b, C, L, heads, &G)) return e;
  const int64_t row = (int64_t)C * L;
  if (q_ss < row || k_ss < row || v_ss < row || dq_ss < row || dk_ss < row || dv_ss < row ||
      (q_ss | k_ss | v_ss | dq_ss | dk_ss | dv_ss) % 4 != 0)
    return BMNAS_E_ARG;
  if (!aligned16(dO) || !aligned16(q) || !aligned16(k) || !aligned16(v) || !aligned16(P) || !aligned16(dq) ||
      !aligned16(dk) || !aligned16(dv))
    return BMNAS_E_ARG;
  const int groups = (G.tiles + kMhaWaves - 1) / kMhaWaves;
  hipLaunchKernelGGL(mha_core_bwd_k, dim3(groups), dim3(64 * kMhaWaves), 0, (hipStream_t)stream, dO,
                     MhaOperand{q, q_ss}, MhaOperand{k, k_ss}, MhaOperand{v, v_ss}, P, MhaResult{dq, dq_ss},
                     MhaResult{dk, dk_ss}, MhaResult{dv, dv_ss}, G, to_cfg(drop));
  BMNAS_CHECK_LAUNCH();
  return 0;
}
