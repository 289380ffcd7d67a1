// The pooling in front of the reshape convs: AdaptiveMaxPool2d of every modality's backbone
// feature map, for the whole group of modalities in ONE launch per direction, written straight in the (b, C_in, L)
// layout the grouped GEMM reads.
//   ReshapeInputLayer        (aux_models.py:62-70):   (b, C_in, T, ...) -> view (b, C_in, T, R) -> pool to (L, 1)
//                                                      (-> F.interpolate(., L): nearest, an identity at size L)
//   ReshapeInputLayer_MMIMDB (aux_models.py:101-108): (b, C_in[, H, W]) -> view (b, C_in, H, W) -> pool to (s, s), s*s = L
// Window of output row i: [floor(i H / oh), ceil((i + 1) H / oh)), columns alike (torch's adaptive rule); the first
// maximum in row-major window order wins, a NaN is a maximum (at::native adaptive_max_pool2d).  The argmax (flat h*W+w,
// int32) is kept for the backward, which is written in GATHER form: one thread per INPUT element sums the gradients
// of the <= 2 x 2 windows it belongs to and whose argmax it is — every dx element is written exactly once, so there
// is neither a zero-fill launch nor an atomic (windows overlap when H % oh != 0).
//
// Element types.  x / dx of a problem are fp32, bf16 or fp16 (PoolProb::dt, block-uniform: one branch per block);
// out, g and idx are fp32 / int32 for all of them.  fp32 problems run the scalar loops they always ran.  Half problems
// move 16 bytes (8 elements) per lane: the tensor is cut into CHUNKS of 8 elements at the 16-byte boundaries of its
// own addresses (chunk starts are the flat element indices e with (x / 2 + e) % 8 == 0, whatever the alignment of x,
// the plane size H * W or the row width W), a lane loads / stores whole chunks and masks the elements that are not
// its own.  A chunk is accessed as one 16-byte vector ONLY if 0 <= start and start + 8 <= b C H W, i.e. only if all of
// its bytes lie in [x, x + 2 b C H W); the at most two chunks that stick out of the tensor are accessed element by
// element, and only at their elements inside it.  So no access touches a byte outside the tensor.
#include "common.hpp"
#include "../../include/bmnas_hip.h"

namespace {

constexpr int kPoolGroup = BMNAS_MAX_GROUP;

struct PoolProb {
  const void* x;       // (b, C, H, W) of type dt
  float* out;          // (b, C, oh * ow)
  int* idx;            // (b, C, oh * ow), nullable in forward
  const float* g;      // backward: gradient of out
  void* dx;            // backward: (b, C, H, W) of type dt
  int C, H, W, oh, ow, G;          // G = lanes per output element (power of two <= 64)
  int dt;                          // BMNAS_DT_*: element type of x / dx
};
struct PoolGroup {
  PoolProb p[kPoolGroup];
  long long start[kPoolGroup + 1];  // first block of problem q
  int n;
};

__device__ __forceinline__ int pool_problem(const PoolGroup& S) {
  int q = 0;
#pragma unroll
  for (int r = 1; r < kPoolGroup; ++r) q += (r < S.n && (long long)blockIdx.x >= S.start[r]) ? 1 : 0;
  return __builtin_amdgcn_readfirstlane(q);
}

// (chains over the compile-time-indexed elements: a run-time index sends the by-value argument struct through scratch)
__device__ __forceinline__ PoolProb pool_pick(const PoolGroup& S, int q, long long* start) {
  PoolProb P = S.p[0];
  *start = S.start[0];
#pragma unroll
  for (int r = 1; r < kPoolGroup; ++r)
    if (q == r) { P = S.p[r]; *start = S.start[r]; }
  return P;
}

// combine the G lanes of an output element: larger value wins, a NaN beats everything, ties go to the smaller flat
// index (= the first in row-major window order); lane 0 of the group writes
__device__ __forceinline__ void pool_combine_store(const PoolProb& P, int G, int gl, bool on, long long o, float best,
                                                   int bi, bool have) {
  for (int off = G >> 1; off > 0; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(bi, off, 64);
    const bool oh_ = __shfl_xor((int)have, off, 64) != 0;
    const bool mine_nan = have && best != best, other_nan = oh_ && ov != ov;
    bool take = false;
    if (oh_ && !have) take = true;
    else if (oh_ && have) {
      if (mine_nan && other_nan) take = oi < bi;
      else if (other_nan) take = true;
      else if (mine_nan) take = false;
      else take = (ov > best) || (ov == best && oi < bi);
    }
    if (take) { best = ov; bi = oi; have = true; }
  }
  if (on && gl == 0) {
    P.out[o] = best;
    if (P.idx != nullptr) P.idx[o] = bi;
  }
}

__device__ __forceinline__ void pool_fwd_f32(const PoolProb& P, int b, long long st) {
  const int G = P.G;
  const long long n_out = (long long)b * P.C * P.oh * P.ow;
  const long long o = (((long long)blockIdx.x - st) * 256 + threadIdx.x) / G;       // this lane group's output element
  const int gl = threadIdx.x & (G - 1);
  const bool on = o < n_out;
  const long long oc = on ? o : n_out - 1;
  const int j = (int)(oc % P.ow), i = (int)((oc / P.ow) % P.oh);
  const long long bc = oc / ((long long)P.oh * P.ow);
  const int hs = (i * P.H) / P.oh, he = ((i + 1) * P.H + P.oh - 1) / P.oh;
  const int ws = (j * P.W) / P.ow, we = ((j + 1) * P.W + P.ow - 1) / P.ow;
  const float* __restrict__ src = (const float*)P.x + bc * P.H * P.W;
  float best = -__builtin_inff();
  int bi = hs * P.W + ws;
  bool have = false;
  for (int h = hs; h < he; ++h)
    for (int w = ws + gl; w < we; w += G) {
      const float v = src[(long long)h * P.W + w];
      const bool nan = v != v;
      if (!have || nan || v > best) {                   // first maximum in this lane's (row-major) order; NaN wins
        if (!(have && best != best)) { best = v; bi = h * P.W + w; }
        have = true;
      }
    }
  pool_combine_store(P, G, gl, on, o, best, bi, have);
}

template <int DT>
__device__ __forceinline__ float pool_widen(unsigned u) {             // the low 16 bits of u, widened (exact)
  if (DT == BMNAS_DT_BF16) return __uint_as_float(u << 16);
  const unsigned short s = (unsigned short)u;
  _Float16 h;
  __builtin_memcpy(&h, &s, 2);
  return (float)h;
}

template <int DT>
__device__ __forceinline__ unsigned pool_narrow(float v) {           // round to nearest even, once; a NaN stays a NaN
  if (DT == BMNAS_DT_BF16) {
    const unsigned u = __float_as_uint(v);
    if (v != v) return (u >> 16) | 0x40u;
    return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
  }
  const _Float16 h = (_Float16)v;
  unsigned short s;
  __builtin_memcpy(&s, &h, 2);
  return s;
}

// Half problems.  The window of an output element is one contiguous span of the plane when it is as wide as the plane
// (ow == 1: ReshapeInputLayer, [hs W, he W)), else he - hs row segments [h W + ws, h W + we).  The G lanes of the
// element share a segment chunk by chunk (see the head of this file): lane gl takes chunks gl, gl + G, ... of the
// segment, each of them one 16-byte load, and visits the elements of a chunk — and its chunks — in increasing flat
// index, so "the first maximum" holds inside a lane as in the scalar loop; pool_combine_store settles it between lanes.
template <int DT>
__device__ __forceinline__ void pool_fwd_half(const PoolProb& P, int b, long long st) {
  const int G = P.G;
  const long long n_out = (long long)b * P.C * P.oh * P.ow;
  const long long o = (((long long)blockIdx.x - st) * 256 + threadIdx.x) / G;
  const int gl = threadIdx.x & (G - 1);
  const bool on = o < n_out;
  const long long oc = on ? o : n_out - 1;
  const int j = (int)(oc % P.ow), i = (int)((oc / P.ow) % P.oh);
  const long long bc = oc / ((long long)P.oh * P.ow);
  const int hs = (i * P.H) / P.oh, he = ((i + 1) * P.H + P.oh - 1) / P.oh;
  const int ws = (j * P.W) / P.ow, we = ((j + 1) * P.W + P.ow - 1) / P.ow;
  const unsigned short* __restrict__ x = (const unsigned short*)P.x;
  const long long n_in = (long long)b * P.C * P.H * P.W;
  const long long pb = bc * P.H * P.W;                               // first element of the plane
  const int mis = (int)(((uintptr_t)x >> 1) & 7);                    // elements of x behind a 16-byte boundary
  const bool span = P.ow == 1;
  const int nseg = span ? 1 : he - hs;
  float best = -__builtin_inff();
  int bi = hs * P.W + ws;
  bool have = false;
  for (int r = 0; r < nseg; ++r) {
    const int lo = span ? hs * P.W : (hs + r) * P.W + ws;            // the segment, flat in the plane
    const int hi = span ? he * P.W : (hs + r) * P.W + we;
    const long long e0 = pb + lo, e1 = pb + hi;
    for (long long cs = e0 - ((e0 + mis) & 7) + 8ll * gl; cs < e1; cs += 8ll * G) {
      const int s0 = (int)(cs - pb);                                 // > lo - 8
      unsigned q[4];
      if (cs >= 0 && cs + 8 <= n_in) {                               // the whole chunk lies inside the tensor
        const uint4 v = *reinterpret_cast<const uint4*>(x + cs);
        q[0] = v.x; q[1] = v.y; q[2] = v.z; q[3] = v.w;
      } else {                                                       // first / last chunk of the tensor: own elements only
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int sa = s0 + 2 * k, sb = sa + 1;
          const unsigned a = (sa >= lo && sa < hi) ? x[cs + 2 * k] : 0u;
          const unsigned c = (sb >= lo && sb < hi) ? x[cs + 2 * k + 1] : 0u;
          q[k] = a | (c << 16);
        }
      }
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int s = s0 + k;
        const float v = pool_widen<DT>((k & 1) ? (q[k >> 1] >> 16) : (q[k >> 1] & 0xffffu));
        if (s >= lo && s < hi && (!have || v != v || v > best)) {    // first maximum in this lane's order; NaN wins
          if (!(have && best != best)) { best = v; bi = s; }
          have = true;
        }
      }
    }
  }
  pool_combine_store(P, G, gl, on, o, best, bi, have);
}

__global__ __launch_bounds__(256) void pool_fwd_group_k(PoolGroup S, int b) {
  long long st;
  const PoolProb P = pool_pick(S, pool_problem(S), &st);
  if (P.dt == BMNAS_DT_F32) pool_fwd_f32(P, b, st);
  else if (P.dt == BMNAS_DT_BF16) pool_fwd_half<BMNAS_DT_BF16>(P, b, st);
  else pool_fwd_half<BMNAS_DT_F16>(P, b, st);
}

// the gradient of input element (bc, h, w): the fp32 sum, in (i, j) order, over the windows that cover it and chose it
__device__ __forceinline__ float pool_gather(const PoolProb& P, long long bc, int h, int w) {
  const int i0 = (h * P.oh) / P.H, i1 = ((h + 1) * P.oh + P.H - 1) / P.H - 1;
  const int j0 = (w * P.ow) / P.W, j1 = ((w + 1) * P.ow + P.W - 1) / P.W - 1;
  const int me = h * P.W + w;
  const long long ob = bc * P.oh * P.ow;
  float acc = 0.f;
  for (int i = i0; i <= i1; ++i)
    for (int j = j0; j <= j1; ++j) {
      const long long o = ob + (long long)i * P.ow + j;
      if (P.idx[o] == me) acc += P.g[o];
    }
  return acc;
}

__device__ __forceinline__ void pool_bwd_f32(const PoolProb& P, int b, long long st) {
  const long long n_in = (long long)b * P.C * P.H * P.W;
  const long long e = ((long long)blockIdx.x - st) * 256 + threadIdx.x;
  if (e >= n_in) return;
  const int w = (int)(e % P.W), h = (int)((e / P.W) % P.H);
  const long long bc = e / ((long long)P.H * P.W);
  ((float*)P.dx)[e] = pool_gather(P, bc, h, w);
}

// Half problems: one lane per chunk of dx (8 adjacent elements, see the head of this file), stored as one 16-byte
// vector when the whole chunk lies inside the tensor, else element by element at its elements inside it.
template <int DT>
__device__ __forceinline__ void pool_bwd_half(const PoolProb& P, int b, long long st) {
  unsigned short* __restrict__ dx = (unsigned short*)P.dx;
  const long long n_in = (long long)b * P.C * P.H * P.W;
  const int mis = (int)(((uintptr_t)dx >> 1) & 7);
  const long long cs = (((long long)blockIdx.x - st) * 256 + threadIdx.x) * 8 - mis;
  if (cs >= n_in) return;
  const long long e = cs < 0 ? 0 : cs;
  int w = (int)(e % P.W), h = (int)((e / P.W) % P.H);
  long long bc = e / ((long long)P.H * P.W);
  unsigned r[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    r[k] = 0u;
    if (cs + k >= 0 && cs + k < n_in) {
      r[k] = pool_narrow<DT>(pool_gather(P, bc, h, w));
      if (++w == P.W) {
        w = 0;
        if (++h == P.H) { h = 0; ++bc; }
      }
    }
  }
  if (cs >= 0 && cs + 8 <= n_in) {
    *reinterpret_cast<uint4*>(dx + cs) = make_uint4(r[0] | (r[1] << 16), r[2] | (r[3] << 16), r[4] | (r[5] << 16),
                                                    r[6] | (r[7] << 16));
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (cs + k >= 0 && cs + k < n_in) dx[cs + k] = (unsigned short)r[k];
  }
}

__global__ __launch_bounds__(256) void pool_bwd_group_k(PoolGroup S, int b) {
  long long st;
  const PoolProb P = pool_pick(S, pool_problem(S), &st);
  if (P.dt == BMNAS_DT_F32) pool_bwd_f32(P, b, st);
  else if (P.dt == BMNAS_DT_BF16) pool_bwd_half<BMNAS_DT_BF16>(P, b, st);
  else pool_bwd_half<BMNAS_DT_F16>(P, b, st);
}

int fill_group(PoolGroup& S, const bmnas_pool_prob_ex_t* probs, int n, int b, bool backward, long long* blocks) {
  if (!probs || n < 1 || b < 0) return BMNAS_E_ARG;
  if (n > kPoolGroup) return BMNAS_E_LIMIT;
  S.n = n;
  long long tot = 0;
  for (int q = 0; q < n; ++q) {
    const bmnas_pool_prob_ex_t& p = probs[q];
    if (p.dtype != BMNAS_DT_F32 && p.dtype != BMNAS_DT_BF16 && p.dtype != BMNAS_DT_F16) return BMNAS_E_ARG;
    if (p.C < 1 || p.H < 1 || p.W < 1 || p.oh < 1 || p.ow < 1) return BMNAS_E_ARG;
    if ((long long)p.H * p.W >= (1ll << 31)) return BMNAS_E_LIMIT;
    if (backward ? (!p.g || !p.idx || !p.dx) : (!p.x || !p.out)) return BMNAS_E_ARG;
    const bool half = p.dtype != BMNAS_DT_F32;
    const uintptr_t addr = (uintptr_t)(backward ? p.dx : p.x);
    if (half && (addr & 1)) return BMNAS_E_ARG;        // the chunk rule needs element-aligned half tensors
    PoolProb& P = S.p[q];
    P.x = p.x; P.out = p.out; P.idx = p.idx; P.g = p.g; P.dx = p.dx;
    P.C = p.C; P.H = p.H; P.W = p.W; P.oh = p.oh; P.ow = p.ow; P.dt = p.dtype;
    const int ww = (p.W + p.ow - 1) / p.ow;            // window width (within one of the adaptive rule)
    // lanes per output element: one per element of a window row (fp32), one per 8-element chunk of a segment (half:
    // the whole window when it is a span, else a window row)
    const long long seg = half ? ((p.ow == 1 ? (long long)((p.H + p.oh - 1) / p.oh) * p.W : ww) + 7) / 8 : ww;
    int G = 1;
    while (G * 2 <= seg && G < 64) G *= 2;
    P.G = G;
    S.start[q] = tot;
    const long long n_in = (long long)b * p.C * p.H * p.W;
    long long work = backward ? n_in : (long long)b * p.C * p.oh * p.ow * G;
    if (backward && half && n_in > 0) work = (n_in + (long long)((addr >> 1) & 7) + 7) / 8;   // chunks of dx
    tot += (work + 255) / 256;
  }
  S.start[n] = tot;
  if (tot >= (1ll << 31)) return BMNAS_E_LIMIT;
  *blocks = tot;
  return 0;
}

int launch_group(const bmnas_pool_prob_ex_t* probs, int n, int b, bool backward, void* stream) {
  PoolGroup S{};
  long long blocks = 0;
  if (int e = fill_group(S, probs, n, b, backward, &blocks)) return e;
  if (blocks == 0) return 0;
  if (backward) hipLaunchKernelGGL(pool_bwd_group_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, S, b);
  else hipLaunchKernelGGL(pool_fwd_group_k, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, S, b);
  BMNAS_CHECK_LAUNCH();
  return 0;
}

// the entry points without a type: the same descriptors with dtype 0
int launch_group_f32(const bmnas_pool_prob_t* probs, int n, int b, bool backward, void* stream) {
  if (!probs || n < 1 || b < 0) return BMNAS_E_ARG;
  if (n > kPoolGroup) return BMNAS_E_LIMIT;
  bmnas_pool_prob_ex_t ex[kPoolGroup];
  for (int q = 0; q < n; ++q) {
    const bmnas_pool_prob_t& p = probs[q];
    ex[q] = bmnas_pool_prob_ex_t{p.x, p.out, p.idx, p.g, p.dx, p.C, p.H, p.W, p.oh, p.ow, BMNAS_DT_F32};
  }
  return launch_group(ex, n, b, backward, stream);
}

}  // namespace

extern "C" int bmnas_adaptive_maxpool_fwd_group(const bmnas_pool_prob_t* probs, int n, int b, void* stream) {
  return launch_group_f32(probs, n, b, false, stream);
}

extern "C" int bmnas_adaptive_maxpool_bwd_group(const bmnas_pool_prob_t* probs, int n, int b, void* stream) {
  return launch_group_f32(probs, n, b, true, stream);
}

extern "C" int bmnas_adaptive_maxpool_fwd_group_ex(const bmnas_pool_prob_ex_t* probs, int n, int b, void* stream) {
  return launch_group(probs, n, b, false, stream);
}

extern "C" int bmnas_adaptive_maxpool_bwd_group_ex(const bmnas_pool_prob_ex_t* probs, int n, int b, void* stream) {
  return launch_group(probs, n, b, true, stream);
}
