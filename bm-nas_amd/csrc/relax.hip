// Temperature / Gumbel-softmax relaxation of the architecture tensors (alphas_edges, every step node's betas and gammas):
//   z = a / tau                      (gumbel == 0: an annealed temperature)
//   z = (a + G) / tau                (gumbel != 0: SNAS / GDAS-style stochastic relaxation, fresh noise per step)
// over up to BMNAS_MAX_PTRS tensors as ONE launch in FRONT of the cell prologue, which then softmaxes z where it
// softmaxed the raw logits.  Backward: da = dz / tau.  Nothing of the softmax / prologue / epilogue kernels changes.
//
// State.  tau, the noise seed and the step counter live in a DEVICE block (bmnas_arch_relax_state_t) that the kernels
// read by address: a captured launch honours a tau edited between replays and draws the noise of the counter as the
// replay finds it — no host value is frozen into a hipGraph and the graph needs no H2D node.
//
// Noise.  The tensors form one flat element sequence (tensor order, row-major) that starts at flat index e0; element e
// draws word e & 3 of philox4x32_10(ctr = (step << 32) + (e >> 2), key = seed ^ 0x6A09E667F3BCC908) — the dropout
// stream's generator (common.hpp) under a salted key, so the two streams of one seed never coincide —,
//   u = ((w >> 9) + 0.5f) * 2^-23,   G = -logf(-logf(u)).
// 23 bits, not 24: k + 0.5 with k < 2^23 is exact in fp32 and u lies in [2^-24, 1 - 2^-24], so both logarithms are
// finite (G in [-2.82, 16.64]); a 24-bit mantissa of w rounds to u = 1 for the top words and gives G = inf.
// Every operation is rounded on its own: a plain add, a correctly rounded division, the accurate logf.
//
// Counter.  The launch is ONE workgroup (the work is a few hundred elements: launch-floor bound whatever the grid):
// every thread has consumed the counter it loaded when it arrives at the barrier behind the element loop, and thread 0
// then stores step + 1 with an ordinary store — no atomic, no race between workgroups, bit-identical from run to run.
//
// Tensor walk.  Neighbouring lanes straddle tensor boundaries, so the tensor index is per lane (unlike the
// one-wavefront-per-row walk of arch_body.hpp, where it is wave-uniform and the pointers follow as scalar loads): the
// element counts come out of the argument block as scalars, the index is found by selects and the pointers are picked
// by pick_ptr's select chains over SGPR pairs — no pointer is loaded from the kernarg segment by a per-lane index, so
// the only dependent round trip of the launch is state + logits -> results.
#include "common.hpp"
#include "../../include/bmnas_hip.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxElems = 65536;
constexpr uint64_t kKeySalt = 0x6A09E667F3BCC908ull;

struct RelaxPack {
  const float* a[BMNAS_MAX_PTRS];     // fwd: logits      bwd: dz
  float* z[BMNAS_MAX_PTRS];           // fwd: z           bwd: da
  float* noise[BMNAS_MAX_PTRS];       // fwd: G export (entries nullable)
  int cnt[BMNAS_MAX_PTRS];            // rows * cols of every tensor
  int n, total;
};

// flat index i of the launch (0 <= i < total) -> its tensor t and the index `at` inside it
__device__ __forceinline__ void relax_locate(const RelaxPack& P, int i, int& t, int& at) {
  t = -1;
  at = 0;
#pragma unroll
  for (int q = 0; q < BMNAS_MAX_PTRS; ++q) {
    const bool open = t < 0 && q < P.n;
    const bool here = open && i < P.cnt[q];
    t = here ? q : t;
    at = here ? i : at;
    i -= (open && !here) ? P.cnt[q] : 0;
  }
}

__device__ __forceinline__ float gumbel_of(uint32_t w) {
#pragma clang fp contract(off)
  const float u = ((float)(w >> 9) + 0.5f) * 1.1920928955078125e-07f;      // 2^-23: every step exact
  return -logf(-logf(u));
}

__global__ __launch_bounds__(kThreads) void arch_relax_fwd_k(RelaxPack P, int64_t e0, bmnas_arch_relax_state_t* state,
                                                             int gumbel, int advance) {
#pragma clang fp contract(off)
  const float tau = state->tau;
  uint64_t seed = 0ull, step = 0ull;
  if (gumbel != 0 || advance != 0) step = state->step;          // (uniform: kernel arguments)
  if (gumbel != 0) seed = state->seed ^ kKeySalt;
  for (int i = threadIdx.x; i < P.total; i += kThreads) {
    int t, at;
    relax_locate(P, i, t, at);
    if (t < 0) continue;                                        // (cannot happen: total is the sum of cnt)
    const float* ap = pick_ptr(P.a, t);
    float* zp = pick_ptr(P.z, t);
    float* np = pick_ptr(P.noise, t);
    const float a = ap[at];
    float v = a;
    if (gumbel != 0) {
      const uint64_t e = (uint64_t)(e0 + i);
      const uint4 r = philox4x32_10((step << 32) + (e >> 2), seed);
      const uint32_t k = (uint32_t)(e & 3ull);
      const uint32_t w = k == 0u ? r.x : (k == 1u ? r.y : (k == 2u ? r.z : r.w));
      const float G = gumbel_of(w);
      if (np != nullptr) np[at] = G;
      v = a + G;
    }
    zp[at] = v / tau;
  }
  // every thread that drew noise has used the counter it loaded: its results are issued in front of this barrier
  __syncthreads();
  if (advance != 0 && threadIdx.x == 0) state->step = step + 1ull;
}

__global__ __launch_bounds__(kThreads) void arch_relax_bwd_k(RelaxPack P, const bmnas_arch_relax_state_t* state) {
#pragma clang fp contract(off)
  const float tau = state->tau;
  for (int i = threadIdx.x; i < P.total; i += kThreads) {
    int t, at;
    relax_locate(P, i, t, at);
    if (t < 0) continue;
    const float* gp = pick_ptr(P.a, t);
    float* op = pick_ptr(P.z, t);
    op[at] = gp[at] / tau;
  }
}

// host side: fill a pack from the C-ABI arrays; returns 0 or a negative error
int fill_relax_pack(RelaxPack& P, const float* const* in, float* const* out, float* const* noise, const int* rows,
                    const int* cols, int n) {
  if (!in || !out || !rows || !cols || n < 1) return BMNAS_E_ARG;
  if (n > BMNAS_MAX_PTRS) return BMNAS_E_LIMIT;
  int64_t total = 0;
  for (int t = 0; t < BMNAS_MAX_PTRS; ++t) {
    P.a[t] = nullptr; P.z[t] = nullptr; P.noise[t] = nullptr; P.cnt[t] = 0;
  }
  for (int t = 0; t < n; ++t) {
    if (!in[t] || !out[t] || rows[t] < 1 || cols[t] < 1) return BMNAS_E_ARG;
    const int64_t c = (int64_t)rows[t] * cols[t];
    total += c;
    if (total > kMaxElems) return BMNAS_E_LIMIT;
    P.a[t] = in[t];
    P.z[t] = out[t];
    P.noise[t] = noise ? noise[t] : nullptr;
    P.cnt[t] = (int)c;
  }
  P.n = n;
  P.total = (int)total;
  return 0;
}

}  // namespace

extern "C" int bmnas_arch_relax_fwd(const float* const* a, float* const* z, float* const* noise, const int* rows,
                                    const int* cols, int n, int64_t e0, bmnas_arch_relax_state_t* state, int gumbel,
                                    int advance, void* stream) {
  RelaxPack P;
  if (!state || e0 < 0) return BMNAS_E_ARG;
  const int rc = fill_relax_pack(P, a, z, noise, rows, cols, n);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(arch_relax_fwd_k, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, P, e0, state, gumbel, advance);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

extern "C" int bmnas_arch_relax_bwd(const float* const* dz, float* const* da, const int* rows, const int* cols, int n,
                                    const bmnas_arch_relax_state_t* state, void* stream) {
  RelaxPack P;
  if (!state) return BMNAS_E_ARG;
  const int rc = fill_relax_pack(P, dz, da, nullptr, rows, cols, n);
  if (rc != 0) return rc;
  hipLaunchKernelGGL(arch_relax_bwd_k, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, P, state);
  BMNAS_CHECK_LAUNCH();
  return 0;
}
