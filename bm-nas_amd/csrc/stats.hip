// Phase statistics of the trainer loop — loss sum, accuracy, per-class F1 counts — tallied by ONE launch per batch into a
// persistent accumulator of 64-bit words (layout: include/bmnas_hip.h, bmnas_phase_stats_words).  Replaces the aten
// launches the loop issued behind every replay (`loss_sum += loss.double() * n`, `argmax == labels`, `sigmoid > th` plus
// the phase-long list of predictions): stream work only, so the launch can sit at the end of a captured forward.
//
// Exactness.  Counts are summed per lane, then per workgroup (wave reductions of common.hpp / LDS integer adds), then
// added with at most one 64-bit integer global atomic per counter and workgroup: integer sums do not depend on the order
// of arrival, so every word is independent of the grid shape and bit-identical from run to run.  Words 0-2 have ONE
// writer per launch (thread 0 of workgroup 0, plain read-modify-write; launches on a stream are ordered): word 0 holds
// the bits of the double  sum + (double)loss * (double)n  with the product and the sum rounded on their own.  There is no
// floating-point atomic.
//
// Loads.  The (n, O) logits are walked as ONE flat array in 16-byte quads laid on the tensor's own 16-byte grid (the
// real class counts, 23 / 60 / 83, give rows that start anywhere on it): a quad that lies inside the tensor is one
// global_load_dwordx4, the at most two that hang over its ends are read element by element — no access leaves the
// tensors, whatever 4-byte alignment the pointers have.
#include "common.hpp"
#include "../../include/bmnas_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kRowLanes = 16;                        // the lanes of one DPP row share a sample (accuracy tally)
constexpr int kRowsPerPass = kThreads / kRowLanes;
constexpr int kMaxBlocks = 256;
constexpr int kNoIndex = 1 << 20;                    // above every class index, exact as a float

typedef unsigned long long u64;

// how many floats p lies behind the 16-byte grid (0 .. 3)
__host__ __device__ __forceinline__ int quad_phase(const void* p) { return (int)(((uintptr_t)p >> 2) & 3); }

// The four elements e0 .. e0 + 3 of p (total elements; e0 may start up to 3 before 0 and the quad may end behind
// total): one 16-byte load where the quad is inside the tensor and on the grid, guarded scalar loads otherwise.
// Elements outside [0, total) come back as 0 and are masked by the caller.
__device__ __forceinline__ void load_quad(const float* __restrict__ p, int phase, int64_t e0, int64_t total,
                                          float (&v)[4]) {
  if (e0 >= 0 && e0 + 4 <= total && ((e0 + phase) & 3) == 0) {
    const float4 q = ld4(p + e0);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t e = e0 + k;
      v[k] = (e >= 0 && e < total) ? p[e] : 0.f;
    }
  }
}

// words 0 - 2: the loss term, the launch count, the sample count (one thread of the launch)
struct Head {
  bool mine;
  float loss;
  u64 w0, w1, w2;
};
__device__ __forceinline__ Head head_begin(const float* __restrict__ loss, const u64* __restrict__ acc) {
  Head h{blockIdx.x == 0 && threadIdx.x == 0, 0.f, 0ull, 0ull, 0ull};
  if (h.mine) {                                      // (issued in front of the tally: the loads travel with its own)
    h.w0 = acc[0];
    h.w1 = acc[1];
    h.w2 = acc[2];
    if (loss != nullptr) h.loss = loss[0];
  }
  return h;
}
__device__ __forceinline__ void head_end(const Head& h, bool has_loss, int n, u64* __restrict__ acc) {
#pragma clang fp contract(off)
  if (!h.mine) return;
  if (has_loss) {
    const double term = (double)h.loss * (double)n;
    const double sum = __longlong_as_double((long long)h.w0) + term;
    acc[0] = (u64)__double_as_longlong(sum);
  }
  acc[1] = h.w1 + 1ull;
  acc[2] = h.w2 + (u64)n;
}

// ---- accuracy: argmax with torch's rule (first maximum; NaN is a maximum, the first NaN wins) == label --------------
__global__ __launch_bounds__(kThreads) void phase_stats_acc_k(const float* __restrict__ logits,
                                                              const int64_t* __restrict__ labels,
                                                              const float* __restrict__ loss, int n, int O,
                                                              u64* __restrict__ acc) {
  __shared__ float red[kThreads / BMNAS_WAVE];
  const Head head = head_begin(loss, acc);
  const int sub = threadIdx.x & (kRowLanes - 1), grp = threadIdx.x / kRowLanes;
  const int phase = quad_phase(logits);
  const int64_t total = (int64_t)n * O;
  float hits = 0.f;                                  // (<= rows of this workgroup's passes per lane: exact)
  // the trip count is the same for every lane of the workgroup: the DPP reductions below see 64 active lanes
  for (int64_t r0 = (int64_t)blockIdx.x * kRowsPerPass; r0 < n; r0 += (int64_t)gridDim.x * kRowsPerPass) {
    const int64_t r = r0 + grp;
    const bool live = r < n;
    const int64_t label = live ? labels[r] : -1;
    const int64_t lo = live ? r * O : 0, hi = live ? lo + O : 0;
    // quads of the 16-byte grid that touch [lo, hi): at most 33 for O <= 128, lane `sub` takes every 16th
    const int64_t q0 = (lo + phase) >> 2, q1 = live ? ((hi + phase - 1) >> 2) : q0 - 1;
    float lmax = -INFINITY;
    int imax = kNoIndex, inan = kNoIndex;
    for (int64_t q = q0 + sub; q <= q1; q += kRowLanes) {
      const int64_t e0 = 4 * q - phase;
      float v[4];
      load_quad(logits, phase, e0, total, v);
#pragma unroll
      for (int k = 0; k < 4; ++k) {                  // ascending class index inside a lane: `>` keeps the first
        const int64_t e = e0 + k;
        if (e < lo || e >= hi) continue;
        const int idx = (int)(e - lo);
        if (v[k] != v[k]) {
          inan = min(inan, idx);
        } else if (imax == kNoIndex || v[k] > lmax) {
          lmax = v[k];
          imax = idx;
        }
      }
    }
    const float m = row16_max(lmax);
    const bool any_nan = row16_max(inan != kNoIndex ? 1.f : 0.f) > 0.f;
    const int cand = any_nan ? inan : ((imax != kNoIndex && lmax == m) ? imax : kNoIndex);
    const int win = (int)(-row16_max(-(float)cand));           // the smallest candidate index of the row
    // (a label outside [0, O) is never equal to a class index: nothing is indexed by it)
    if (live && sub == 0 && (int64_t)win == label) hits += 1.f;
  }
  const float total_hits = block_sum_fresh<kThreads / BMNAS_WAVE>(hits, red);
  if (threadIdx.x == 0 && total_hits > 0.f) atomicAdd(acc + 3, (u64)total_hits);
  head_end(head, loss != nullptr, n, acc);
}

// ---- F1: per-class tp / fp / fn of (logit > logit_threshold) against (target > 0.5) ------------------------------------
__global__ __launch_bounds__(kThreads) void phase_stats_f1_k(const float* __restrict__ logits,
                                                             const float* __restrict__ targets,
                                                             const float* __restrict__ loss, float thr, int n, int O,
                                                             u64* __restrict__ acc) {
  __shared__ unsigned cnt[3 * BMNAS_STATS_MAX_CLASSES];
  const Head head = head_begin(loss, acc);
  for (int i = threadIdx.x; i < 3 * O; i += kThreads) cnt[i] = 0u;
  __syncthreads();
  const int phase = quad_phase(logits), phase_t = quad_phase(targets);
  const int64_t total = (int64_t)n * O;
  const int64_t quads = (total + phase + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (int64_t)gridDim.x * kThreads) {
    const int64_t e0 = 4 * q - phase;
    float x[4], t[4];
    load_quad(logits, phase, e0, total, x);
    load_quad(targets, phase_t, e0, total, t);       // (16-byte loads too when both tensors sit alike on the grid)
    int cls = (int)((e0 + 4 * (int64_t)O) % O);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t e = e0 + k;
      if (e >= 0 && e < total) {
        const bool pred = x[k] > thr, truth = t[k] > 0.5f;     // (NaN: neither, as torch's `>`)
        if (pred && truth) atomicAdd(&cnt[3 * cls], 1u);
        else if (pred) atomicAdd(&cnt[3 * cls + 1], 1u);
        else if (truth) atomicAdd(&cnt[3 * cls + 2], 1u);
      }
      cls = (cls + 1 == O) ? 0 : cls + 1;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < 3 * O; i += kThreads) {
    const unsigned c = cnt[i];
    if (c != 0u) atomicAdd(acc + 4 + i, (u64)c);
  }
  head_end(head, loss != nullptr, n, acc);
}

bool stats_args_ok(const void* logits, const void* second, int second_align, const void* loss, int n, int O,
                   const void* acc) {
  if (!logits || !second || !acc || n < 1 || O < 1 || O > BMNAS_STATS_MAX_CLASSES) return false;
  if (((uintptr_t)logits & 3) || ((uintptr_t)second & (uintptr_t)(second_align - 1)) || ((uintptr_t)acc & 7) ||
      ((uintptr_t)loss & 3))
    return false;
  return true;
}

}  // namespace

extern "C" int bmnas_phase_stats_words(int O) {
  if (O < 1) return BMNAS_E_ARG;
  return 4 + 3 * O;
}

extern "C" int bmnas_phase_stats_acc(const float* logits, const int64_t* labels, const float* loss, int n, int O,
                                     uint64_t* acc, void* stream) {
  if (!stats_args_ok(logits, labels, 8, loss, n, O, acc)) return BMNAS_E_ARG;
  const int64_t passes = ((int64_t)n + kRowsPerPass - 1) / kRowsPerPass;
  const int blocks = (int)(passes < kMaxBlocks ? passes : kMaxBlocks);
  hipLaunchKernelGGL(phase_stats_acc_k, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, logits, labels, loss, n, O,
                     reinterpret_cast<u64*>(acc));
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_phase_stats_f1(const float* logits, const float* targets, const float* loss,
                                    float logit_threshold, int n, int O, uint64_t* acc, void* stream) {
  if (!stats_args_ok(logits, targets, 4, loss, n, O, acc)) return BMNAS_E_ARG;
  const int64_t quads = ((int64_t)n * O + quad_phase(logits) + 3) >> 2;
  const int64_t want = (quads + kThreads - 1) / kThreads;
  const int blocks = (int)(want < kMaxBlocks ? want : kMaxBlocks);
  hipLaunchKernelGGL(phase_stats_f1_k, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, logits, targets, loss,
                     logit_threshold, n, O, reinterpret_cast<u64*>(acc));
  BMNAS_CHECK_LAUNCH();
  return 0;
}
