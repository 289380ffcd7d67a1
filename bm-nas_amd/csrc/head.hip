// The head of a search step in two launches (forward, backward) instead of seven:
//
//   K7   out = relu(LayerNorm_[M*C, L](cat(states[-M:])))          model_search.py:63-67
//        logits = out.view(b, -1) @ Wcls^T + bcls                  mmimdb_darts_searchable.py:82-83, 114
//        loss = criterion(logits, labels)                          mmimdb_darts_searchable.py:22,
//                                                                  ntu_darts_searchable.py:25, ego_...:24
//   and their backward down to the gradients of the M states.
//
// What makes one launch each possible:
//  * the LayerNorm statistics of a sample are not reduced here: every state that K7 concatenates is
//    the output of a step node, whose kernel (node_mix_ln_fwd / cat_ln_fwd) already holds the whole
//    sample in registers and hands over (sum, sum of squares) per sample; mean and rstd of the
//    concatenation follow from M such pairs.  K7 thereby becomes elementwise and moves into the
//    operand fetch of the classifier GEMM — `out` (b x 6144 floats) is never written or read;
//  * the two per-sample reductions of the LayerNorm BACKWARD (mean of dxh, mean of dxh * xhat) are
//    linear in dlogits:   m1[s] = sum_o dl[s,o] A[s,o] / D,   m2[s] = sum_o dl[s,o] B[s,o] / D   with
//        A[s,o] = sum_k mask[s,k] lnw[k] W[o,k],    B[s,o] = sum_k mask[s,k] lnw[k] xhat[s,k] W[o,k],
//    two more accumulator sets of the SAME forward GEMM (same W operand).  The backward is then
//    elementwise per (sample, k) too, and tiles freely over the chip (a per-sample workgroup would
//    read the whole 565 KB of Wcls per sample);
//  * batch reductions (dWcls, dbcls, dlnw, dlnb) leave as per-16-sample-chunk partials with plain
//    stores and are summed by the launch that ends the backward pass (bmnas_backward_epilogue):
//    8 x fewer bytes than fp32 atomics would serialise at the memory side.
//
// Matrix products on v_mfma_f32_16x16x4_f32 (exact fp32).  Bound: latency / L2 (the whole head moves
// ~15 MB at MM-IMDB batch 128); algorithmic FLOPs fwd 6 b O D (three accumulator sets), bwd 4 b O D.
#include "common.hpp"
#include "../../include/bmnas_hip.h"
#include "lazy_ln.hpp"
#include "ln_sample.hpp"
#include <algorithm>
#include <cstdlib>

namespace {

constexpr int kHeadSrc = 4;
constexpr int kMaxO = 128;

struct HeadSrc {
  const float* p[kHeadSrc];      // M states (b, C, L)
  const float* sums[kHeadSrc];   // per state: (b, 2) = (sum, sum of squares) of each sample
};

// Step-node outputs whose LayerNorm is applied HERE instead of by their producer (lazyln.hip, lazy_ln.hpp).
// Forward: source `lq` is given un-normalised (src.p[lq] = pre) with its moment records; it is normalised in the
// operand fetch, its (mean, rstd) are written to nstats[lq] and its per-sample sums follow from the records.
// Backward: EVERY source is given as `pre` + nstats + the node LayerNorm's affine, and the launch also leaves,
// per (sample, 64-k group), the partials of S(gy w), S(gy w xhat) of the node LayerNorm backward in lnpart[q].
struct HeadLazy {
  const float* rec;              // forward: (b, P, 8) of source lq
  const float* prm;              //          (P, 8)
  const float* nw[kHeadSrc];     // node LayerNorm affine (C, L); forward: entry 0 describes source lq
  const float* nb[kHeadSrc];
  float* nstats[kHeadSrc];       // (b, 2) mean | rstd of the node LayerNorm (forward: entry 0, written; backward: read)
  float* lnpart[kHeadSrc];       // backward: (b, CL / 64, 2), nullable
  int lq, P;
};

__device__ __forceinline__ void sample_stats(const HeadSrc& src, int n_src, int s, int D, float* mean, float* rstd) {
  float S = 0.f, Q = 0.f;
  float2 sv[kHeadSrc];
#pragma unroll
  for (int q = 0; q < kHeadSrc; ++q)                          // (every load first, clamped source index: no load in a loop)
    sv[q] = reinterpret_cast<const float2*>(pick_ptr(src.sums, q < n_src ? q : 0))[s];
#pragma unroll
  for (int q = 0; q < kHeadSrc; ++q) {
    S += q < n_src ? sv[q].x : 0.f;
    Q += q < n_src ? sv[q].y : 0.f;
  }
  const float inv = 1.f / (float)D;
  const float m = S * inv;
  const float var = fmaxf(Q * inv - m * m, 0.f);
  *mean = m;
  *rstd = 1.f / sqrtf(var + kLnEps);
}

// ------------------------------------------------------------------------------ forward
struct HeadFwdArgs {
  HeadSrc src;
  const float* ln_w;
  const float* ln_b;
  const float* W;        // (O, D)
  const float* bias;     // (O)
  float* hb;             // [3][b][O], zero-filled: logits | A | B (atomic adds)
  float* hb_part;        // deterministic mode: [KS][hb_stride] — every k-slice STORES its partial tile (no atomics; the
  long long hb_stride;   // launcher sums the slices in order, bmnas_sum_chunks); NULL: atomics into hb
  float* stats;          // (b, 2): mean, rstd of the K7 LayerNorm (written by k-slice 0)
  int b, O, D, CL, n_src, KS;
};

// grid = (KS k-slices, ceil(b / 16) sample tiles); 4 waves; wave w of slice ks takes the 16-k blocks
// kb = (j * KS + ks) * 4 + w, j < J.  All operand loads of a wave are issued before its first MFMA.
template <int J, int TJ, bool LZ>
__global__ __launch_bounds__(256) void head_fwd_k(HeadFwdArgs a, HeadLazy z) {
  __shared__ float red[4][3][16][16 * TJ + 1];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lo = lane & 15, h = lane >> 4;
  const int ks = blockIdx.x, st = blockIdx.y;
  STAMP(4, blockIdx.y * gridDim.x + blockIdx.x, 0);
  const int s = st * 16 + lo;
  const int sc = s < a.b ? s : a.b - 1;                       // clamped rows are never stored
  const int nkb = a.D / 16;
  int oc[TJ];
#pragma unroll
  for (int t = 0; t < TJ; ++t) {
    const int o = 16 * t + lo;
    oc[t] = o < a.O ? o : a.O - 1;
  }
  float4 xv[J], lw[J], lb[J], wv[J][TJ], nwv[LZ ? J : 1], nbv[LZ ? J : 1];
  bool valid[J], lzq[J];
#pragma unroll
  for (int j = 0; j < J; ++j) {
    const int kb = (j * a.KS + ks) * 4 + wave;
    valid[j] = kb < nkb;                                      // wave-uniform
    const int kbc = valid[j] ? kb : nkb - 1;
    const int k = kbc * 16 + 4 * h;
    const int q = (kbc * 16) / a.CL;
    // (a select chain over the pointers, not a.src.p[q]: a run-time index into the argument block is a MEMORY load of
    // the pointer with a wait in front of the operand load it feeds — common.hpp pick_ptr)
    xv[j] = ld4(pick_ptr(a.src.p, q) + (int64_t)sc * a.CL + (k - q * a.CL));
    lw[j] = ld4(a.ln_w + k);
    lb[j] = ld4(a.ln_b + k);
    lzq[j] = LZ && q == z.lq;                                 // wave-uniform
    if (LZ) {                                                 // unconditional loads: an always-valid address otherwise
      nwv[j] = ld4(lzq[j] ? z.nw[0] + (k - q * a.CL) : a.ln_w + k);
      nbv[j] = ld4(lzq[j] ? z.nb[0] + (k - q * a.CL) : a.ln_b + k);
    }
#pragma unroll
    for (int t = 0; t < TJ; ++t) wv[j][t] = ld4(a.W + (int64_t)oc[t] * a.D + k);
  }
  // the statistics AFTER the operand loads have been issued: their own loads (moment records, per-sample sums) are a
  // dependent round trip that the operands do not wait for — in front of them it was one (two with a lazy source)
  // full memory latency before the first operand load went out
  __builtin_amdgcn_sched_barrier(0);
  float mean, rstd, nmean = 0.f, nrstd = 1.f;
  if (LZ) {
    // (all kHeadSrc per-sample sums fetched unconditionally, from a valid slot where there is no such source or it is
    // the lazy one: no load inside a run-time loop, where each would be waited for on its own)
    float2 sv[kHeadSrc];
#pragma unroll
    for (int q = 0; q < kHeadSrc; ++q) {
      const bool use = q < a.n_src && q != z.lq;
      const int qq = use ? q : (z.lq == 0 ? (a.n_src > 1 ? 1 : 0) : 0);
      const float* sp = pick_ptr(a.src.sums, qq);
      sv[q] = reinterpret_cast<const float2*>(sp != nullptr ? sp : z.rec)[sc];
    }
    const LazyStats ls = lazy_combine(z.rec, z.prm, z.P, sc);
    float S = ls.osum, Q = ls.osq;
#pragma unroll
    for (int q = 0; q < kHeadSrc; ++q) {
      const bool use = q < a.n_src && q != z.lq;
      S += use ? sv[q].x : 0.f;
      Q += use ? sv[q].y : 0.f;
    }
    const float inv = 1.f / (float)a.D;
    mean = S * inv;
    rstd = 1.f / sqrtf(fmaxf(Q * inv - mean * mean, 0.f) + kLnEps);
    nmean = ls.mean;
    nrstd = ls.rstd;
  } else {
    sample_stats(a.src, a.n_src, sc, a.D, &mean, &rstd);
  }
  if (ks == 0 && wave == 0 && h == 0 && s < a.b) {
    a.stats[2 * s] = mean;
    a.stats[2 * s + 1] = rstd;
    if (LZ) {
      z.nstats[0][2 * s] = nmean;
      z.nstats[0][2 * s + 1] = nrstd;
    }
  }
  STAMP(4, blockIdx.y * gridDim.x + blockIdx.x, 1);
  __builtin_amdgcn_sched_barrier(0);
  f32x4 acc[3][TJ];
#pragma unroll
  for (int v = 0; v < 3; ++v)
#pragma unroll
    for (int t = 0; t < TJ; ++t) acc[v][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < J; ++j) {
    if (!valid[j]) continue;
    float x4[4] = {xv[j].x, xv[j].y, xv[j].z, xv[j].w};
    const float w4[4] = {lw[j].x, lw[j].y, lw[j].z, lw[j].w};
    const float b4[4] = {lb[j].x, lb[j].y, lb[j].z, lb[j].w};
    if (LZ && lzq[j]) {                                       // the node's own LayerNorm first (node_search.py:68)
      const float n4[4] = {nwv[j].x, nwv[j].y, nwv[j].z, nwv[j].w};
      const float c4[4] = {nbv[j].x, nbv[j].y, nbv[j].z, nbv[j].w};
#pragma unroll
      for (int r = 0; r < 4; ++r) x4[r] = ln_apply(x4[r], nmean, nrstd, n4[r], c4[r]);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float xh = ln_xhat(x4[r], mean, rstd);
      const float pre = xh * w4[r] + b4[r];
      const bool on = pre > 0.f;
      const float f = on ? pre : 0.f;                         // relu(LayerNorm(.))
      const float a2 = on ? w4[r] : 0.f;                      // mask * lnw
      const float a3 = a2 * xh;                               // mask * lnw * xhat
#pragma unroll
      for (int t = 0; t < TJ; ++t) {
        const float wr = r == 0 ? wv[j][t].x : r == 1 ? wv[j][t].y : r == 2 ? wv[j][t].z : wv[j][t].w;
        acc[0][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(f, wr, acc[0][t], 0, 0, 0);
        acc[1][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, wr, acc[1][t], 0, 0, 0);
        acc[2][t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, wr, acc[2][t], 0, 0, 0);
      }
    }
  }
  // acc[v][t][r] = OUT_v[sample st*16 + 4h + r][class 16 t + lo].  All four waves lay their tiles out
  // in LDS as [v][sample][class]; the workgroup then adds the four partials and issues the atomics in
  // memory order — hb is [v][b][O] row-major, so a 16-sample tile is ONE contiguous run of 16 * O
  // floats per v: full 256-byte wave-instructions instead of four 64-byte pieces each
#pragma unroll
  for (int v = 0; v < 3; ++v)
#pragma unroll
    for (int t = 0; t < TJ; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][v][4 * h + r][16 * t + lo] = acc[v][t][r];
  STAMP(4, blockIdx.y * gridDim.x + blockIdx.x, 2);
  __syncthreads();
  const int rows = (a.b - st * 16) < 16 ? (a.b - st * 16) : 16;
  const int per_v = rows * a.O;
  for (int i = threadIdx.x; i < 3 * per_v; i += 256) {
    const int v = i / per_v, e = i - v * per_v;
    const int sr = e / a.O, o = e - sr * a.O;
    float val = (red[0][v][sr][o] + red[1][v][sr][o]) + (red[2][v][sr][o] + red[3][v][sr][o]);
    if (v == 0 && ks == 0) val += a.bias[o];
    if (a.hb_part != nullptr) a.hb_part[(int64_t)ks * a.hb_stride + ((int64_t)v * a.b + st * 16) * a.O + e] = val;
    else atomicAdd(a.hb + ((int64_t)v * a.b + st * 16) * a.O + e, val);
  }
  STAMP(4, blockIdx.y * gridDim.x + blockIdx.x, 3);
}

// ----------------------------------------------------------------------------- backward
struct HeadBwdArgs {
  HeadSrc src;
  float* dsrc[kHeadSrc];     // gradients of the M states (nullable)
  uint32_t acc_mask;         // bit q: accumulate into dsrc[q]
  const float* ln_w;
  const float* ln_b;
  const float* W;
  const float* hb;           // [3][b][O] from the forward
  const float* stats;        // (b, 2)
  const float* g;            // mode 0: dlogits (b, O)
  const float* gscale;       // nullable device scalar multiplying dlogits (all modes)
  const float* labels_f;     // mode 1: (b, O) multi-hot floats
  const long long* labels_i; // mode 2: (b) class ids
  float* loss;               // modes 1, 2: += mean loss (zero-filled by the caller)
  float* loss_part;          // deterministic mode: [n_chunk] — each sample chunk STORES its share (summed by the host in
                             // a fixed order); NULL: atomic adds into loss
  float* part;               // [n_chunk][O + 3][D] partials of each sample chunk (bmnas_head_chunks): rows 0..O-1 dW,
                             // O dln_w, O+1 dln_b, O+2 dbias (first O entries)
  float* scrub;              // side job: zero-fill (the caller's backward accumulation arena)
  long long scrub4;
  int b, O, D, CL, n_src, mode;
  int probe;                 // BMNAS_HEAD_PROBE: timing diagnostics only (results incomplete)
  // the weighted / smoothed criteria (CR != 0 instantiations only; bmnas_criterion_t): a NULL pointer means ones
  const float* cw;           // (O) class weights
  const float* cpw;          // (O) BCE positive weights
  long long ignore;          // CE: rows with this label count for nothing
  float eps;                 // CE: label smoothing
  int red;                   // 0 mean, 1 sum
};

__device__ __forceinline__ float sigmoidf_(float v) { return 1.f / (1.f + __expf(-v)); }

// grid = (D / 64 k-groups, sample chunks of 16 * SG); wave w of k-group x owns the (16 SG samples x
// 16 k) tile kt = 4 x + w.  Every global load of the kernel is issued first — the tile's operands do
// not depend on the criterion — then the prologue (dl[16 SG][O] = criterion gradient or the given
// one, m1 / m2 / mean / rstd of the chunk's samples, into LDS; thread = (row, 16-class stripe),
// reductions over a row = shuffles inside a 16-lane group), then the tile:  per group of 16 samples
// dfeat^T = W^T dl^T on the matrix cores with k on the accumulator rows (float4 along k per sample:
// LayerNorm backward and the state-gradient store are coalesced), and dW = dl^T feat accumulated
// over the SG groups, with feat handed from the first product's lanes to the second's through a per-wave LDS image
// (never stored to memory, the states fetched once).  Each product requests all its LDS operands, then runs its MFMAs
// without a wait or a branch between them (profiles/r22_head_bwd_batches.txt).
// OT = class tiles of 16 the kernel is built for (O <= 16 OT).
// CR = 0: modes 0 - 2 as above.  CR = 1: BCEWithLogits with per-class weight / pos_weight, CR = 2: CrossEntropy with
// class weights, label smoothing and ignore_index, both with reduction mean or sum (the formulas: bmnas_hip.h,
// bmnas_criterion_t).  A compile-time parameter: the CR = 0 instantiations carry none of the extra registers.  The
// per-class values join the prologue loads (a thread owns the class stripes lo + 16 u); the denominator of the
// weighted CE mean, sum of w[label] over the rows that count, is formed by every workgroup over all b labels in a
// fixed order (thread-strided partial sums, wave butterflies, four LDS slots): no host read, no launch in front.
__device__ __forceinline__ float group16_sum(float v) { return row16_sum(v); }
__device__ __forceinline__ float group16_max(float v) { return row16_max(v); }

template <int OT, int SG, bool LZ, int CR = 0>
__global__ __launch_bounds__(256) void head_bwd_k(HeadBwdArgs a, HeadLazy z) {
  constexpr int kSteps = 4 * OT, kRows = 16 * SG;
  // dl in the two layouts its products read it in, so that one lane's operands of a product are contiguous and leave as
  // ds_read_b128, every one of them requested before the product's first MFMA (one wait per product instead of one per MFMA):
  //   dl_a[row][(o & 3) kSteps + (o >> 2)]   GEMM 1: lane (lo, h) takes dl[row = lo][o = 4 t + h], t = 0 .. kSteps - 1;
  //                                          row stride = 4 (mod 32) floats: the 16 rows of a k-slot h cover all 64 banks
  //   dl_b[row >> 2][o][row & 3]             GEMM 2: lane (lo, h) takes dl[row = 4 h + r][o = 16 t + lo], r = 0 .. 3;
  //                                          lanes lo are 16 bytes apart
  // Both hold zeros past O and in rows past b: the products run all OT class tiles without a range test.
  constexpr int kDlA = 4 * kSteps + 4, kMs = LZ ? 8 : 4;
  __shared__ __attribute__((aligned(16))) float dl_a[kRows][kDlA];
  __shared__ __attribute__((aligned(16))) float dl_b[kRows / 4][16 * OT][4];
  __shared__ __attribute__((aligned(16))) float ms[kRows][kMs];  // per row: m1, m2, mean, rstd (, node mean, node rstd, -, -)
  // feat of a wave's (16 samples x 16 k) block per sample group: written as GEMM 1's lanes hold it (sample lo, k 4h + r:
  // one float4), read as GEMM 2 takes it (sample 4h + r, k lo).  Row stride 20: a read's four k-slots are 16 banks apart.
  __shared__ __attribute__((aligned(16))) float ft_s[4][SG][16][20];
  __shared__ float lnp_s[LZ ? 4 : 1][LZ ? kRows : 1][2];
  __shared__ float loss_s[4];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int lo = lane & 15, h = lane >> 4;
  const int chunk = blockIdx.y, s0 = chunk * kRows;
  STAMP(5, blockIdx.y * gridDim.x + blockIdx.x, 0);
  const float gs = (a.gscale != nullptr) ? a.gscale[0] : 1.f;
  const float invD = 1.f / (float)a.D;
  // ---- the tile's operand loads (independent of everything the prologue computes)
  const int nkt = a.D / 16;
  const int kt = blockIdx.x * 4 + wave;
  const bool vt = kt < nkt;                                     // wave-uniform
  const int k0 = (vt ? kt : nkt - 1) * 16;
  const int q = k0 / a.CL;                                      // a tile never straddles two states
  const int kin = k0 - q * a.CL;
  float wv[kSteps];
#pragma unroll
  for (int t = 0; t < kSteps; ++t) {
    const int o = 4 * t + h;
    wv[t] = a.W[(int64_t)(o < a.O ? o : a.O - 1) * a.D + k0 + lo];     // clamped address, selected below
  }
  const float4 lw = ld4(a.ln_w + k0 + 4 * h), lb = ld4(a.ln_b + k0 + 4 * h);
  // the workgroup's source q through select chains (common.hpp pick_ptr), never a.src.p[q]: a run-time index into the
  // argument block is a memory load of the POINTER and a wait in front of every operand load it feeds
  const float* const srcq = pick_ptr(a.src.p, q);
  float4 nw4 = make_float4(1.f, 1.f, 1.f, 1.f), nb4 = make_float4(0.f, 0.f, 0.f, 0.f);
  const float* nstq = nullptr;
  if (LZ) {                                                     // (q: uniform over the workgroup, CL % 64 == 0)
    const float* const nwq_p = pick_ptr(z.nw, q);
    const float* const nbq_p = pick_ptr(z.nb, q);
    nstq = pick_ptr(z.nstats, q);
    nw4 = ld4(nwq_p + kin + 4 * h);
    nb4 = ld4(nbq_p + kin + 4 * h);
  }
  // (the states are fetched ONCE, in GEMM 1's layout; GEMM 2 takes the same block through ft_s)
  float4 x[SG];
#pragma unroll
  for (int g = 0; g < SG; ++g) {
    const int s = s0 + 16 * g + lo;
    x[g] = ld4(srcq + (int64_t)(s < a.b ? s : a.b - 1) * a.CL + kin + 4 * h);
  }
  // ---- prologue: thread = (row tid / 16 of sample group g, class stripe lo + 16 u)
  {
    float zz[SG][OT], aa[SG][OT], bb[SG][OT], yy[SG][OT], st_mean[SG], st_rstd[SG], nd_mean[SG], nd_rstd[SG];
    int lab[SG];
    float cwv[CR != 0 ? OT : 1], cpv[CR == 1 ? OT : 1];
    if constexpr (CR != 0) {
      // (unconditional loads, from an always-valid address where there is no such vector: hb holds >= 3 O floats)
      const float* const cwp = a.cw != nullptr ? a.cw : a.hb;
      const float* const cpp = a.cpw != nullptr ? a.cpw : a.hb;
#pragma unroll
      for (int u = 0; u < OT; ++u) {
        const int o = lo + 16 * u;
        const int oc = o < a.O ? o : a.O - 1;
        const float wv_ = cwp[oc];
        cwv[u] = a.cw != nullptr ? wv_ : 1.f;
        if constexpr (CR == 1) {
          const float pv_ = cpp[oc];
          cpv[u] = a.cpw != nullptr ? pv_ : 1.f;
        }
      }
    }
#pragma unroll
    for (int g = 0; g < SG; ++g) {
      const int sp = s0 + 16 * g + (threadIdx.x >> 4);
      const int spc = sp < a.b ? sp : a.b - 1;
#pragma unroll
      for (int u = 0; u < OT; ++u) {
        const int o = lo + 16 * u;
        const int oc = o < a.O ? o : a.O - 1;
        zz[g][u] = (a.mode == 0) ? a.g[(int64_t)spc * a.O + oc] : a.hb[(int64_t)spc * a.O + oc];
        aa[g][u] = a.hb[((int64_t)a.b + spc) * a.O + oc];
        bb[g][u] = a.hb[((int64_t)2 * a.b + spc) * a.O + oc];
        yy[g][u] = (a.mode == 1) ? a.labels_f[(int64_t)spc * a.O + oc] : 0.f;
      }
      if constexpr (CR == 2) {                                  // -1: the row counts for nothing (never an index)
        const long long l = a.labels_i[spc];
        lab[g] = (l != a.ignore && l >= 0 && l < (long long)a.O) ? (int)l : -1;
      } else {
        lab[g] = (a.mode == 2) ? (int)a.labels_i[spc] : 0;
      }
      st_mean[g] = a.stats[2 * spc];
      st_rstd[g] = a.stats[2 * spc + 1];
      nd_mean[g] = LZ ? nstq[2 * spc] : 0.f;
      nd_rstd[g] = LZ ? nstq[2 * spc + 1] : 1.f;
    }
    // the side job (zero-fill of the caller's accumulation arena) AFTER every load of the kernel has been issued: at
    // the top it stood — with an argument-block fetch and a dependent scalar load of its own — in front of them
    __builtin_amdgcn_sched_barrier(0);
    for (long long i = ((long long)blockIdx.y * gridDim.x + blockIdx.x) * 256 + threadIdx.x; i < a.scrub4;
         i += (long long)gridDim.x * gridDim.y * 256)
      st4_wt(a.scrub + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
    __builtin_amdgcn_sched_barrier(0);
    float loss_acc = 0.f;
    float cden = 1.f, cwsum = 0.f;
    if constexpr (CR == 2) {
      if (a.red == 0) {                                         // uniform
        __shared__ float den_s[4];
        float t = 0.f;
        for (int i = threadIdx.x; i < a.b; i += 256) {
          const long long l = a.labels_i[i];
          const bool k = l != a.ignore && l >= 0 && l < (long long)a.O;
          const float wl = a.cw != nullptr ? a.cw[k ? l : 0] : 1.f;
          t += k ? wl : 0.f;
        }
        t = wave_sum(t);
        if (lane == 0) den_s[wave] = t;
        __syncthreads();
        cden = (den_s[0] + den_s[1]) + (den_s[2] + den_s[3]);
      }
#pragma unroll
      for (int u = 0; u < OT; ++u) cwsum += (lo + 16 * u < a.O) ? cwv[u] : 0.f;
      cwsum = group16_sum(cwsum);
    }
#pragma unroll
    for (int g = 0; g < SG; ++g) {
      const int rr = 16 * g + (threadIdx.x >> 4);
      const bool vsp = s0 + rr < a.b;
      float dl[OT];
      float row_loss = 0.f;
      if constexpr (CR == 1) {                                  // BCEWithLogits, weight / pos_weight, mean | sum
        const float sc_ = a.red == 0 ? gs / ((float)a.b * (float)a.O) : gs;
#pragma unroll
        for (int u = 0; u < OT; ++u) {
          const bool vo = lo + 16 * u < a.O;
          const float z = zz[g][u], y = yy[g][u];
          const float c = 1.f + (cpv[u] - 1.f) * y;
          dl[u] = vo ? cwv[u] * ((1.f - y) - c * sigmoidf_(-z)) * sc_ : 0.f;
          if (vo) row_loss += cwv[u] * ((1.f - y) * z + c * (log1pf(__expf(-fabsf(z))) + fmaxf(-z, 0.f)));
        }
      } else if constexpr (CR == 2) {                           // CrossEntropy, weight / smoothing / ignore, mean | sum
        const bool keep = lab[g] >= 0;
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < OT; ++u)
          if (lo + 16 * u < a.O) mx = fmaxf(mx, zz[g][u]);
        mx = group16_max(mx);
        float e[OT], den = 0.f;
#pragma unroll
        for (int u = 0; u < OT; ++u) {
          e[u] = (lo + 16 * u < a.O) ? __expf(zz[g][u] - mx) : 0.f;
          den += e[u];
        }
        den = group16_sum(den);
        const float lse = mx + __logf(den);
        float sm = 0.f, wy = 0.f, ny = 0.f;                     // sum_c w_c (-log p_c), w[label], -log p[label]
#pragma unroll
        for (int u = 0; u < OT; ++u) {
          const int o = lo + 16 * u;
          const float nl = lse - zz[g][u];
          if (o < a.O) sm += cwv[u] * nl;
          if (o < a.O && o == lab[g]) {
            wy = cwv[u];
            ny = nl;
          }
        }
        sm = group16_sum(sm);
        wy = group16_sum(wy);
        ny = group16_sum(ny);
        const float a1 = (1.f - a.eps) * wy, a2 = a.eps / (float)a.O;
        const float sc_ = gs / cden;
#pragma unroll
        for (int u = 0; u < OT; ++u) {
          const int o = lo + 16 * u;
          const float p = e[u] / den;
          dl[u] = (o < a.O && keep) ? (a1 * (p - (o == lab[g] ? 1.f : 0.f)) + a2 * (cwsum * p - cwv[u])) * sc_ : 0.f;
        }
        if (lo == 0 && keep) row_loss = a1 * ny + a2 * sm;
      } else if (a.mode == 0) {
#pragma unroll
        for (int u = 0; u < OT; ++u) dl[u] = (lo + 16 * u < a.O) ? zz[g][u] * gs : 0.f;
      } else if (a.mode == 1) {                                 // BCEWithLogits, reduction = mean
        const float sc_ = gs / ((float)a.b * (float)a.O);
#pragma unroll
        for (int u = 0; u < OT; ++u) {
          const bool vo = lo + 16 * u < a.O;
          const float z = zz[g][u], y = yy[g][u];
          dl[u] = vo ? (sigmoidf_(z) - y) * sc_ : 0.f;
          if (vo) row_loss += fmaxf(z, 0.f) - z * y + log1pf(__expf(-fabsf(z)));
        }
      } else {                                                  // CrossEntropy, reduction = mean
        float mx = -INFINITY;
#pragma unroll
        for (int u = 0; u < OT; ++u)
          if (lo + 16 * u < a.O) mx = fmaxf(mx, zz[g][u]);
        mx = group16_max(mx);
        float e[OT], den = 0.f;
#pragma unroll
        for (int u = 0; u < OT; ++u) {
          e[u] = (lo + 16 * u < a.O) ? __expf(zz[g][u] - mx) : 0.f;
          den += e[u];
        }
        den = group16_sum(den);
        const float sc_ = gs / (float)a.b;
#pragma unroll
        for (int u = 0; u < OT; ++u) {
          const int o = lo + 16 * u;
          dl[u] = (o < a.O) ? (e[u] / den - (o == lab[g] ? 1.f : 0.f)) * sc_ : 0.f;
          if (o < a.O && o == lab[g]) row_loss += (mx + __logf(den)) - zz[g][u];
        }
      }
      float p1 = 0.f, p2 = 0.f;
#pragma unroll
      for (int u = 0; u < OT; ++u) {
        if (!vsp) dl[u] = 0.f;
        const int o = lo + 16 * u;                              // (dl[u] is zero past O in every mode)
        dl_a[rr][(o & 3) * kSteps + (o >> 2)] = dl[u];
        dl_b[rr >> 2][o][rr & 3] = dl[u];
        p1 += dl[u] * aa[g][u];
        p2 += dl[u] * bb[g][u];
      }
      p1 = group16_sum(p1);
      p2 = group16_sum(p2);
      if (lo == 0) {
        *reinterpret_cast<float4*>(&ms[rr][0]) = make_float4(p1 * invD, p2 * invD, st_mean[g], st_rstd[g]);
        if (LZ) *reinterpret_cast<float4*>(&ms[rr][kMs - 4]) = make_float4(nd_mean[g], nd_rstd[g], 0.f, 0.f);
      }
      loss_acc += vsp ? row_loss : 0.f;
    }
    if (a.mode != 0 && blockIdx.x == 0) {
      loss_acc = wave_sum(loss_acc);
      // (the chunk's 16 SG rows are spread over the workgroup's four waves: wave partials meet in LDS first when the
      // chunk's share has to be ONE number)
      float share;
      if constexpr (CR == 1) share = a.red == 0 ? loss_acc / ((float)a.b * (float)a.O) : loss_acc;
      else if constexpr (CR == 2) share = loss_acc / cden;     // (mean over no row that counts: 0 / 0 = NaN, as torch)
      else share = loss_acc / (a.mode == 1 ? (float)a.b * (float)a.O : (float)a.b);
      if (a.loss_part != nullptr) {
        if (lane == 0) loss_s[wave] = share;
      } else if (lane == 0) {
        atomicAdd(a.loss, share);
      }
    }
  }
  __syncthreads();
  if (a.loss_part != nullptr && a.mode != 0 && blockIdx.x == 0 && threadIdx.x == 0)
    a.loss_part[chunk] = (loss_s[0] + loss_s[1]) + (loss_s[2] + loss_s[3]);
  if (a.part != nullptr && blockIdx.x == 0 && (int)threadIdx.x < a.O) {   // dbias partial of this chunk
    float t = 0.f;
#pragma unroll
    for (int rr = 0; rr < kRows; ++rr) t += dl_a[rr][(threadIdx.x & 3) * kSteps + (threadIdx.x >> 2)];
    a.part[((int64_t)chunk * (a.O + 3) + a.O + 2) * a.D + threadIdx.x] = t;
  }
  STAMP(5, blockIdx.y * gridDim.x + blockIdx.x, 1);
  if (!vt || (a.probe & 8)) return;
  // ---- the tile
  float* const part = a.part + (int64_t)chunk * (a.O + 3) * a.D;
  const float wq[4] = {lw.x, lw.y, lw.z, lw.w}, bq[4] = {lb.x, lb.y, lb.z, lb.w};
  const float nwq[4] = {nw4.x, nw4.y, nw4.z, nw4.w}, nbq[4] = {nb4.x, nb4.y, nb4.z, nb4.w};
  float gw[4] = {0.f, 0.f, 0.f, 0.f}, gb[4] = {0.f, 0.f, 0.f, 0.f};
  // GEMM 1: D[k = 4h + r][s = lo] = sum_o W[o][k0 + 4h + r] dl[s][o].  Every LDS operand of the product — dl of all class
  // steps and the per-sample values, of all sample groups — is requested first (float4 reads, one wait); the steps then run
  // without a range test (W is selected to zero past O, dl IS zero there: the steps past O add zeros) with the sample
  // groups' accumulators taking turns, each in its own order t = 0, 1, ...
  float wz[kSteps];
#pragma unroll
  for (int t = 0; t < kSteps; ++t) wz[t] = (4 * t + h < a.O) ? wv[t] : 0.f;
  float4 mv[SG], nv[SG], da[SG][OT];
#pragma unroll
  for (int g = 0; g < SG; ++g) {
    const int rl = 16 * g + lo;
    mv[g] = *reinterpret_cast<const float4*>(&ms[rl][0]);
    nv[g] = *reinterpret_cast<const float4*>(&ms[rl][kMs - 4]);
#pragma unroll
    for (int j = 0; j < OT; ++j) da[g][j] = *reinterpret_cast<const float4*>(&dl_a[rl][h * kSteps + 4 * j]);
  }
#pragma unroll
  for (int g = 0; g < SG; ++g) {                                  // (common.hpp pin4: the batch stays in front of the MFMAs)
#pragma unroll
    for (int j = 0; j < OT; ++j) pin4(da[g][j]);
    pin4(mv[g]);
    if (LZ) pin4(nv[g]);
  }
  f32x4 acc1[SG];
#pragma unroll
  for (int g = 0; g < SG; ++g) acc1[g] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int j = 0; j < OT; ++j) {
#pragma unroll
    for (int g = 0; g < SG; ++g) acc1[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[4 * j], da[g][j].x, acc1[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < SG; ++g) acc1[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[4 * j + 1], da[g][j].y, acc1[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < SG; ++g) acc1[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[4 * j + 2], da[g][j].z, acc1[g], 0, 0, 0);
#pragma unroll
    for (int g = 0; g < SG; ++g) acc1[g] = __builtin_amdgcn_mfma_f32_16x16x4f32(wz[4 * j + 3], da[g][j].w, acc1[g], 0, 0, 0);
  }
  float* const d = pick_ptr(a.dsrc, q);
  const bool dst = d != nullptr && !(a.probe & 2), dacc = (a.acc_mask & (1u << q)) != 0;      // uniform
  float4 dx4[SG];
#pragma unroll
  for (int g = 0; g < SG; ++g) {
    const int rl = 16 * g + lo;
    const bool vs = s0 + rl < a.b;
    const f32x4 acc = acc1[g];
    const float m1 = mv[g].x, m2 = mv[g].y, mean = mv[g].z, rstd = mv[g].w;
    float xq[4] = {x[g].x, x[g].y, x[g].z, x[g].w};
    float xhn[4] = {0.f, 0.f, 0.f, 0.f};
    if (LZ) {                                                   // the state itself: LayerNorm_node(pre)
      const float nmean = nv[g].x, nrstd = nv[g].y;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        xhn[r] = ln_xhat(xq[r], nmean, nrstd);
        xq[r] = xhn[r] * nwq[r] + nbq[r];
      }
    }
    float dx[4], ff[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float xh = ln_xhat(xq[r], mean, rstd);
      const float pre = xh * wq[r] + bq[r];
      const bool on = pre > 0.f;
      const float gy = (on && vs) ? acc[r] : 0.f;               // gradient at the LayerNorm output
      dx[r] = ln_dx(gy * wq[r], xh, m1, m2, rstd);
      gw[r] += gy * xh;
      gb[r] += gy;
      ff[r] = vs ? fmaxf(pre, 0.f) : 0.f;                       // feat = relu(LayerNorm(.)), zero in rows past b
    }
    // feat for GEMM 2, from what this lane holds: (sample lo, k 4h + r) here, (sample 4h + r, k lo) there
    *reinterpret_cast<float4*>(&ft_s[wave][g][lo][4 * h]) = make_float4(ff[0], ff[1], ff[2], ff[3]);
    dx4[g] = make_float4(dx[0], dx[1], dx[2], dx[3]);
    if (LZ) {
      // this wave's 16 k of the node LayerNorm backward's two sums, per sample: S(gy w), S(gy w xhat)
      float q1 = 0.f, q2 = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float t = vs ? dx[r] * nwq[r] : 0.f;
        q1 += t;
        q2 += t * xhn[r];
      }
      q1 = xor16_sum(q1); q1 = xor32_sum(q1);
      q2 = xor16_sum(q2); q2 = xor32_sum(q2);
      if (h == 0) {
        lnp_s[wave][rl][0] = q1;
        lnp_s[wave][rl][1] = q2;
      }
    }
  }
  // the state gradients, behind both groups' arithmetic.  (The old value of an accumulating call is loaded INSIDE the
  // store's condition: a load that some path leaves unwaited makes the compiler wait for every outstanding memory
  // operation at the next barrier — these write-through stores included.)
#pragma unroll
  for (int g = 0; g < SG; ++g) {
    const int s = s0 + 16 * g + lo;
    if (dst && s < a.b) {
      float* pp = d + (int64_t)s * a.CL + kin + 4 * h;
      float4 o4 = dx4[g];
      if (dacc) o4 = f4_add(o4, ld4(pp));
      st4_w0<5>(pp, o4);
    }
  }
  STAMP(5, blockIdx.y * gridDim.x + blockIdx.x, 2);
  if (LZ) {                                                     // (every wave is here: CL % 64 == 0 -> vt)
    __syncthreads();
    float* lp = pick_ptr(z.lnpart, q);
    if (lp != nullptr && (int)threadIdx.x < 2 * kRows) {
      const int rl = threadIdx.x >> 1, cpt = threadIdx.x & 1;
      if (s0 + rl < a.b) {
        const int nkg = a.CL / 64, kg = blockIdx.x - q * nkg;
        lp[((int64_t)(s0 + rl) * nkg + kg) * 2 + cpt] =
            (lnp_s[0][rl][cpt] + lnp_s[1][rl][cpt]) + (lnp_s[2][rl][cpt] + lnp_s[3][rl][cpt]);
      }
    }
  }
  // LayerNorm affine partials of this chunk: sum over the samples (lanes lo, groups) per k
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    gw[r] = group16_sum(gw[r]);
    gb[r] = group16_sum(gb[r]);
  }
  // (part == NULL: nobody wants the classifier / K7-affine gradients — the architecture step of the search loop
  // differentiates alpha / beta / gamma only — so the affine partials and GEMM 2 are skipped)
  STAMP(5, blockIdx.y * gridDim.x + blockIdx.x, 3);
  if (a.part == nullptr) return;
  if (lo == 0) {
    st4_wt(part + (int64_t)a.O * a.D + k0 + 4 * h, make_float4(gw[0], gw[1], gw[2], gw[3]));
    st4_wt(part + (int64_t)(a.O + 1) * a.D + k0 + 4 * h, make_float4(gb[0], gb[1], gb[2], gb[3]));
  }
  // GEMM 2: dW[o = 16 t + lo][k0 + 4h + r] = sum_s feat[s][k0 + 4h + r] dl[s][o] — feat on the row operand, dl on the
  // column operand: an accumulator holds four consecutive k of one class and leaves as one 16-byte store (a plain one:
  // written through, the epilogue and the launch after this one each ran 0.3 us longer and the step did not move).
  // Both operands of all class tiles are requested first (feat back from this wave's ft_s, dl as float4 over r); the class
  // tiles' accumulators then take turns, each summing its samples in the order g, r.
  if (!(a.probe & 1)) {                                           // uniform (timing builds)
    __builtin_amdgcn_wave_barrier();                              // ft_s: this wave's own writes, in program order
    float fr[SG][4];
    float4 db[SG][OT];
#pragma unroll
    for (int g = 0; g < SG; ++g) {
#pragma unroll
      for (int r = 0; r < 4; ++r) fr[g][r] = ft_s[wave][g][4 * h + r][lo];
#pragma unroll
      for (int t = 0; t < OT; ++t) db[g][t] = *reinterpret_cast<const float4*>(&dl_b[4 * g + h][16 * t + lo][0]);
    }
#pragma unroll
    for (int g = 0; g < SG; ++g) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pin1(fr[g][r]);
#pragma unroll
      for (int t = 0; t < OT; ++t) pin4(db[g][t]);
    }
    f32x4 acc2[OT];
#pragma unroll
    for (int t = 0; t < OT; ++t) acc2[t] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int g = 0; g < SG; ++g) {
#pragma unroll
      for (int t = 0; t < OT; ++t) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[g][0], db[g][t].x, acc2[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < OT; ++t) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[g][1], db[g][t].y, acc2[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < OT; ++t) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[g][2], db[g][t].z, acc2[t], 0, 0, 0);
#pragma unroll
      for (int t = 0; t < OT; ++t) acc2[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(fr[g][3], db[g][t].w, acc2[t], 0, 0, 0);
    }
#pragma unroll
    for (int t = 0; t < OT; ++t) {
      const int o = 16 * t + lo;
      // (probe bit 4, timing builds: one store per address — the volume of a design without per-chunk partials)
      if (o < a.O && (!(a.probe & 4) || chunk == 0))
        st4(part + (int64_t)o * a.D + k0 + 4 * h, make_float4(acc2[t][0], acc2[t][1], acc2[t][2], acc2[t][3]));
    }
  }
  STAMP(5, blockIdx.y * gridDim.x + blockIdx.x, 4);
}

// Sum of per-chunk partials: out[e] = sum_c part[c][e]  (float4 stream).  Runs as a slice of the
// backward epilogue launch; also callable on its own.
__global__ __launch_bounds__(256) void sum_chunks_k(const float* __restrict__ part, float* __restrict__ out,
                                                    int n_chunk, long long n4) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 t = ld4(part + 4 * i);
    for (int c = 1; c < n_chunk; ++c) t = f4_add(t, ld4(part + 4 * (i + (long long)c * n4)));
    st4_wt(out + 4 * i, t);
  }
}

// out[e] = sum_c part[c * stride + e] in the order c = 0, 1, ... (deterministic head forward): n4 float4 + a scalar tail
__global__ __launch_bounds__(256) void sum_chunks_strided_k(const float* __restrict__ part, float* __restrict__ out,
                                                            int n_chunk, long long n4, long long stride, long long tail) {
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
    float4 t = ld4(part + 4 * i);
    for (int c = 1; c < n_chunk; ++c) t = f4_add(t, ld4(part + (long long)c * stride + 4 * i));
    st4_wt(out + 4 * i, t);
  }
  if (blockIdx.x == 0 && (long long)threadIdx.x < tail) {
    const long long e = 4 * n4 + threadIdx.x;
    float t = part[e];
    for (int c = 1; c < n_chunk; ++c) t += part[(long long)c * stride + e];
    out[e] = t;
  }
}

}  // namespace

// tools/stamp_probe.py (timing builds): slot 4 head_fwd_k, 5 head_bwd_k
BMNAS_DEFINE_STAMP_SETTER(bmnas_debug_stamps_head)

// samples per partial-sum chunk of the backward: 32 (two MFMA sample groups per workgroup: the W
// operand and the partial stores are shared) once the batch fills the chip that way, else 16
static inline int head_sg(int b) { return b >= 64 ? 2 : 1; }

extern "C" int bmnas_head_chunks(int b) {
  if (b < 1) return BMNAS_E_ARG;
  const int rows = 16 * head_sg(b);
  return (b + rows - 1) / rows;
}

static int head_fwd_impl(const float* const* srcs, const float* const* sums, int n_src, const float* ln_w,
                         const float* ln_b, const float* W, const float* bias, float* hb, float* stats, int b, int C,
                         int L, int O, const HeadLazy* lazy, float* hb_part, void* stream) {
  if (!ln_w || !ln_b || !W || !bias || !hb || !stats || b < 0 || C < 1 || L < 1 || O < 1) return BMNAS_E_ARG;
  if (O > kMaxO) return BMNAS_E_LIMIT;
  if ((C * L) % 16) return BMNAS_E_SHAPE;
  HeadFwdArgs a{};
  if (!srcs || !sums || n_src < 1) return BMNAS_E_ARG;
  if (n_src > kHeadSrc) return BMNAS_E_LIMIT;
  for (int q = 0; q < n_src; ++q) {
    if (!srcs[q] || (!sums[q] && !(lazy && q == lazy->lq))) return BMNAS_E_ARG;
    a.src.p[q] = srcs[q];
    a.src.sums[q] = sums[q];
  }
  if (b == 0) return 0;
  a.ln_w = ln_w; a.ln_b = ln_b; a.W = W; a.bias = bias; a.hb = hb; a.stats = stats;
  a.b = b; a.O = O; a.CL = C * L; a.D = n_src * C * L; a.n_src = n_src;
  const int nkb = a.D / 16;
  // three 16-k blocks per wave when the grid still fills the chip, else one or two
  const int tiles = (b + 15) / 16;
  int J = 3;
  if ((nkb + 11) / 12 * tiles < 128) J = (nkb + 7) / 8 * tiles < 128 ? 1 : 2;
  a.KS = (nkb + 4 * J - 1) / (4 * J);
  a.hb_part = hb_part;
  a.hb_stride = ((long long)3 * b * O + 3) / 4 * 4;             // (bmnas_head_fwd_part_floats)
  dim3 grid((unsigned)a.KS, (unsigned)tiles);
  const int TJ = (O + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
  HeadLazy z{};
  if (lazy) z = *lazy;
#define HF(Jv, Tv)                                                                              \
  do {                                                                                          \
    if (lazy) hipLaunchKernelGGL((head_fwd_k<Jv, Tv, true>), grid, dim3(256), 0, st, a, z);     \
    else hipLaunchKernelGGL((head_fwd_k<Jv, Tv, false>), grid, dim3(256), 0, st, a, z);         \
  } while (0)
#define HF_T(Jv)                                                                      \
  do {                                                                                \
    if (TJ <= 2) HF(Jv, 2); else if (TJ <= 4) HF(Jv, 4); else if (TJ <= 6) HF(Jv, 6); \
    else HF(Jv, 8);                                                                   \
  } while (0)
  if (J == 3) HF_T(3); else if (J == 2) HF_T(2); else HF_T(1);
#undef HF_T
#undef HF
  BMNAS_CHECK_LAUNCH();
  if (hb_part != nullptr) {
    // the k-slices in order (padding floats of a slice are never written: sum exactly 3 b O, rounded down to a
    // multiple of four, and the tail by hand)
    // (n = 3: b = 1, O = 1 — no float4 at all, the tail alone; workgroup 0 sums it, so there is always one)
    const long long n = (long long)3 * b * O, n4 = n / 4 * 4;
    hipLaunchKernelGGL(sum_chunks_strided_k, dim3((unsigned)std::max<long long>(1, std::min<long long>((n4 / 4 + 255) / 256, 2048))),
                       dim3(256), 0, st, hb_part, hb, a.KS, n4 / 4, a.hb_stride, n - n4);
    BMNAS_CHECK_LAUNCH();
  }
  return 0;
}

extern "C" int bmnas_head_fwd_part_floats(int b, int C, int L, int n_src, int O) {
  // an upper bound of what bmnas_head_fwd_lazy's hb_part needs: one slice per 64 k at most
  if (b < 1 || C < 1 || L < 1 || n_src < 1 || O < 1) return BMNAS_E_ARG;
  const long long slices = ((long long)n_src * C * L / 16 + 3) / 4;
  const long long n = slices * (((long long)3 * b * O + 3) / 4 * 4);
  return n < (1LL << 31) ? (int)n : BMNAS_E_LIMIT;
}

extern "C" int bmnas_head_fwd(const float* const* srcs, const float* const* sums, int n_src,
                              const float* ln_w, const float* ln_b, const float* W, const float* bias,
                              float* hb, float* stats, int b, int C, int L, int O, void* stream) {
  return head_fwd_impl(srcs, sums, n_src, ln_w, ln_b, W, bias, hb, stats, b, C, L, O, nullptr, nullptr, stream);
}

extern "C" int bmnas_head_fwd_lazy(const float* const* srcs, const float* const* sums, int n_src, int lazy_q,
                                   const bmnas_lazy_ln_t* lazy, const float* ln_w, const float* ln_b,
                                   const float* W, const float* bias, float* hb, float* stats, int b, int C, int L,
                                   int O, float* hb_part, void* stream) {
  if (!lazy || lazy_q < 0 || lazy_q >= n_src) return BMNAS_E_ARG;
  if (!lazy->pre || !lazy->rec || !lazy->prm || !lazy->ln_w || !lazy->ln_b || !lazy->stats) return BMNAS_E_ARG;
  if (!bmnas_lazy_ln_ok(C, L)) return BMNAS_E_LIMIT;
  if (!srcs || srcs[lazy_q] != lazy->pre) return BMNAS_E_ARG;      // the lazy source IS given un-normalised
  HeadLazy z{};
  z.rec = lazy->rec; z.prm = lazy->prm; z.nw[0] = lazy->ln_w; z.nb[0] = lazy->ln_b; z.nstats[0] = lazy->stats;
  z.lq = lazy_q; z.P = bmnas_lazy_ln_parts(C, L);
  return head_fwd_impl(srcs, sums, n_src, ln_w, ln_b, W, bias, hb, stats, b, C, L, O, &z, hb_part, stream);
}

// The options of a descriptor form, judged before every shape and limit rule of either entry point: kind 1 (BCE) | 2 (CE)
static int crit_arg_check(int kind, const bmnas_criterion_t& crit) {
  if (kind != BMNAS_CRIT_BCE && kind != BMNAS_CRIT_CE) return BMNAS_E_ARG;
  if (!(crit.label_smoothing >= 0.f && crit.label_smoothing < 1.f)) return BMNAS_E_ARG;
  if (crit.reduction != BMNAS_REDUCE_MEAN && crit.reduction != BMNAS_REDUCE_SUM) return BMNAS_E_ARG;
  if (kind == BMNAS_CRIT_CE && crit.pos_weight) return BMNAS_E_ARG;
  if (kind == BMNAS_CRIT_BCE && crit.label_smoothing != 0.f) return BMNAS_E_ARG;
  return 0;
}

static int head_bwd_impl(const float* const* srcs, const float* const* sums, float* const* dsrcs, int n_src,
                         uint32_t accumulate_mask, const float* ln_w, const float* ln_b, const float* W,
                         const float* hb, const float* stats, int mode, const float* g, const float* gscale,
                         const void* labels, float* loss, float* part, int b, int C, int L, int O, float* scrub,
                         int64_t scrub_n, const HeadLazy* lazy, float* loss_part, const bmnas_criterion_t* crit,
                         void* stream) {
  if (!dsrcs || !ln_w || !ln_b || !W || !hb || !stats || b < 0 || C < 1 || L < 1 || O < 1)
    return BMNAS_E_ARG;                          // (part may be NULL: no classifier / K7-affine gradients wanted)
  if (mode < 0 || mode > 2 || (mode == 0 && !g) || (mode != 0 && (!labels || !loss))) return BMNAS_E_ARG;
  if (crit) {                                    // (the *_crit entry points have judged it already: crit_arg_check)
    if (const int rc = crit_arg_check(mode, *crit)) return rc;
  }
  if (scrub_n < 0 || (scrub_n > 0 && !scrub) || scrub_n % 4) return BMNAS_E_ARG;
  if (O > kMaxO) return BMNAS_E_LIMIT;
  if ((C * L) % 16) return BMNAS_E_SHAPE;
  if (lazy && (C * L) % 64) return BMNAS_E_SHAPE;
  HeadBwdArgs a{};
  if (!srcs || n_src < 1) return BMNAS_E_ARG;
  if (n_src > kHeadSrc) return BMNAS_E_LIMIT;
  if (part && O > n_src * C * L) return BMNAS_E_SHAPE;          // dbias lives in ONE row of part (D floats): O <= D
  for (int q = 0; q < n_src; ++q) {
    if (!srcs[q] || (!lazy && (!sums || !sums[q]))) return BMNAS_E_ARG;
    a.src.p[q] = srcs[q];
    a.src.sums[q] = sums ? sums[q] : nullptr;
  }
  if (b == 0) return 0;
  for (int q = 0; q < n_src; ++q) a.dsrc[q] = dsrcs[q];
  a.acc_mask = accumulate_mask; a.ln_w = ln_w; a.ln_b = ln_b; a.W = W; a.hb = hb; a.stats = stats;
  a.g = g; a.gscale = gscale; a.mode = mode;
  a.labels_f = mode == 1 ? (const float*)labels : nullptr;
  a.labels_i = mode == 2 ? (const long long*)labels : nullptr;
  a.loss = loss; a.loss_part = loss_part; a.part = part; a.scrub = scrub; a.scrub4 = scrub_n / 4;
  a.b = b; a.O = O; a.CL = C * L; a.D = n_src * C * L; a.n_src = n_src;
  if (crit) {
    a.cw = crit->weight; a.cpw = crit->pos_weight; a.ignore = crit->ignore_index; a.eps = crit->label_smoothing;
    a.red = crit->reduction;
  }
#if (defined(BMNAS_BODY_PROBES) && BMNAS_BODY_PROBES) || defined(BMNAS_CLASS_PROBE)
  static const int probe = []() { const char* e = getenv("BMNAS_HEAD_PROBE"); return e ? atoi(e) : 0; }();
  a.probe = probe;
#else
  a.probe = 0;    // timing diagnostics exist in -DBMNAS_BODY_PROBES=1 builds only
#endif
  const int nkt = a.D / 16, sg = head_sg(b), chunks = bmnas_head_chunks(b);
  dim3 grid((unsigned)((nkt + 3) / 4), (unsigned)chunks);
  const int OT = (O + 15) / 16;
  hipStream_t st = (hipStream_t)stream;
  HeadLazy z{};
  if (lazy) z = *lazy;
#define HB3(OTv, SGv, LZv)                                                                              \
  do {                                                                                                  \
    if (!crit) hipLaunchKernelGGL((head_bwd_k<OTv, SGv, LZv>), grid, dim3(256), 0, st, a, z);           \
    else if (mode == 1) hipLaunchKernelGGL((head_bwd_k<OTv, SGv, LZv, 1>), grid, dim3(256), 0, st, a, z); \
    else hipLaunchKernelGGL((head_bwd_k<OTv, SGv, LZv, 2>), grid, dim3(256), 0, st, a, z);              \
  } while (0)
#define HB2(OTv, SGv)              \
  do {                             \
    if (lazy) HB3(OTv, SGv, true); \
    else HB3(OTv, SGv, false);     \
  } while (0)
#define HB(OTv)               \
  do {                        \
    if (sg == 2) HB2(OTv, 2); \
    else HB2(OTv, 1);         \
  } while (0)
  if (OT <= 2) HB(2); else if (OT <= 4) HB(4); else if (OT <= 6) HB(6); else HB(8);
#undef HB
#undef HB2
#undef HB3
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_head_bwd(const float* const* srcs, const float* const* sums, float* const* dsrcs,
                              int n_src, uint32_t accumulate_mask, const float* ln_w, const float* ln_b,
                              const float* W, const float* hb, const float* stats, int mode, const float* g,
                              const float* gscale, const void* labels, float* loss, float* part,
                              int b, int C, int L, int O, float* scrub, int64_t scrub_n, void* stream) {
  return head_bwd_impl(srcs, sums, dsrcs, n_src, accumulate_mask, ln_w, ln_b, W, hb, stats, mode, g, gscale, labels,
                       loss, part, b, C, L, O, scrub, scrub_n, nullptr, nullptr, nullptr, stream);
}

extern "C" int bmnas_head_bwd_crit(const float* const* srcs, const float* const* sums, float* const* dsrcs,
                                   int n_src, uint32_t accumulate_mask, const float* ln_w, const float* ln_b,
                                   const float* W, const float* hb, const float* stats, int kind,
                                   const float* gscale, const void* labels, float* loss, float* part, int b, int C,
                                   int L, int O, float* scrub, int64_t scrub_n, bmnas_criterion_t crit,
                                   void* stream) {
  if (const int rc = crit_arg_check(kind, crit)) return rc;
  return head_bwd_impl(srcs, sums, dsrcs, n_src, accumulate_mask, ln_w, ln_b, W, hb, stats, kind, nullptr, gscale,
                       labels, loss, part, b, C, L, O, scrub, scrub_n, nullptr, nullptr, &crit, stream);
}

static int head_bwd_lazy_impl(const bmnas_lazy_ln_t* lazy, float* const* lnpart, float* const* dsrcs, int n_src,
                              uint32_t accumulate_mask, const float* ln_w, const float* ln_b, const float* W,
                              const float* hb, const float* stats, int mode, const float* g, const float* gscale,
                              const void* labels, float* loss, float* part, int b, int C, int L, int O, float* scrub,
                              int64_t scrub_n, float* loss_part, const bmnas_criterion_t* crit, void* stream) {
  if (!lazy || !lnpart || n_src < 1) return BMNAS_E_ARG;
  if (n_src > kHeadSrc) return BMNAS_E_LIMIT;
  if (!bmnas_lazy_ln_ok(C, L)) return BMNAS_E_LIMIT;             // (as the forward half: the sources are its family's)
  HeadLazy z{};
  const float* srcs[kHeadSrc] = {nullptr, nullptr, nullptr, nullptr};
  for (int q = 0; q < n_src; ++q) {
    if (!lazy[q].pre || !lazy[q].ln_w || !lazy[q].ln_b || !lazy[q].stats) return BMNAS_E_ARG;
    srcs[q] = lazy[q].pre;
    z.nw[q] = lazy[q].ln_w; z.nb[q] = lazy[q].ln_b; z.nstats[q] = lazy[q].stats; z.lnpart[q] = lnpart[q];
  }
  z.lq = -1; z.P = 0;
  return head_bwd_impl(srcs, nullptr, dsrcs, n_src, accumulate_mask, ln_w, ln_b, W, hb, stats, mode, g, gscale,
                       labels, loss, part, b, C, L, O, scrub, scrub_n, &z, loss_part, crit, stream);
}

extern "C" int bmnas_head_bwd_lazy(const bmnas_lazy_ln_t* lazy, float* const* lnpart, float* const* dsrcs,
                                   int n_src, uint32_t accumulate_mask, const float* ln_w, const float* ln_b,
                                   const float* W, const float* hb, const float* stats, int mode, const float* g,
                                   const float* gscale, const void* labels, float* loss, float* part, int b, int C,
                                   int L, int O, float* scrub, int64_t scrub_n, float* loss_part, void* stream) {
  return head_bwd_lazy_impl(lazy, lnpart, dsrcs, n_src, accumulate_mask, ln_w, ln_b, W, hb, stats, mode, g, gscale,
                            labels, loss, part, b, C, L, O, scrub, scrub_n, loss_part, nullptr, stream);
}

extern "C" int bmnas_head_bwd_lazy_crit(const bmnas_lazy_ln_t* lazy, float* const* lnpart, float* const* dsrcs,
                                        int n_src, uint32_t accumulate_mask, const float* ln_w, const float* ln_b,
                                        const float* W, const float* hb, const float* stats, int kind,
                                        const float* gscale, const void* labels, float* loss, float* part, int b,
                                        int C, int L, int O, float* scrub, int64_t scrub_n, float* loss_part,
                                        bmnas_criterion_t crit, void* stream) {
  if (const int rc = crit_arg_check(kind, crit)) return rc;
  return head_bwd_lazy_impl(lazy, lnpart, dsrcs, n_src, accumulate_mask, ln_w, ln_b, W, hb, stats, kind, nullptr,
                            gscale, labels, loss, part, b, C, L, O, scrub, scrub_n, loss_part, &crit, stream);
}

extern "C" int bmnas_sum_chunks(const float* part, float* out, int n_chunk, int64_t n, void* stream) {
  if (!part || !out || n_chunk < 1 || n < 0 || n % 4) return BMNAS_E_ARG;
  if (n == 0) return 0;
  int blocks = (int)((n / 4 + 255) / 256);
  if (blocks > 2048) blocks = 2048;
  hipLaunchKernelGGL(sum_chunks_k, dim3(blocks), dim3(256), 0, (hipStream_t)stream, part, out, n_chunk,
                     (long long)(n / 4));
  BMNAS_CHECK_LAUNCH();
  return 0;
}
