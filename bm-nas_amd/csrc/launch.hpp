// Host side of the mix and per-sample LayerNorm launches (mixsum.hip, layernorm.hip, bnmix.hip, lazyln.hip,
// nodemix_sel.hip): run-time count -> template argument, the launch shape of a one-workgroup-per-sample LayerNorm
// kernel, the streaming / reduction grids, and the entry checks those sources share.  Host code only.
#pragma once
#include "common.hpp"
#include "../../include/bmnas_hip.h"
#include "bn_fin.hpp"
#include <type_traits>
#include <utility>

namespace {

// ---- dispatchers: f(int_c<N>{}) for the N that equals the run-time value; 0, or BMNAS_E_LIMIT
// when no N does.  The launch stands once, in a generic lambda:
//   dispatch_range<1, 15>(n_in, [&](auto N) { hipLaunchKernelGGL((k<decltype(N)::value>), ...); });
// Only the listed values are instantiated, and in list order (a recursion, not a fold over ||, which instantiates
// back to front): the device object lists a family's kernels in the order the source names them.
template <int N>
using int_c = std::integral_constant<int, N>;
template <int V0, int... Vs, class F>
inline int dispatch_of(int v, F&& f) {
  if (v == V0) {
    f(int_c<V0>{});
    return 0;
  }
  if constexpr (sizeof...(Vs) > 0) return dispatch_of<Vs...>(v, f);
  else return BMNAS_E_LIMIT;
}
template <int Lo, int... Is, class F>
inline int dispatch_seq(int n, F&& f, std::integer_sequence<int, Is...>) {
  return dispatch_of<(Lo + Is)...>(n, f);
}
template <int Lo, int Hi, class F>
inline int dispatch_range(int n, F&& f) {
  return dispatch_seq<Lo>(n, f, std::make_integer_sequence<int, Hi - Lo + 1>{});
}
template <class F>
inline void dispatch_bool(bool flag, F&& f) {
  if (flag) f(std::true_type{});
  else f(std::false_type{});
}

// ---- launch shape of a kernel that holds one sample (d4 float4) in the registers of one workgroup: 512 threads when
// the batch leaves CUs idle (b <= 256 workgroups on 256 CUs) and the sample fills them, else 256; vpt float4 per
// thread from {1, 2, 3, 4, 8, 16}, -1 above 16.
struct LnShape {
  bool wide;
  int bs;
  int vpt;
};
constexpr LnShape ln_launch_shape(int b, int d4) {
  const bool wide = b <= 256 && d4 >= 512;
  const int bs = wide ? 512 : 256;
  const int need = (d4 + bs - 1) / bs;
  const int vpt = need <= 1 ? 1 : need <= 4 ? need : need <= 8 ? 8 : need <= 16 ? 16 : -1;
  return LnShape{wide, bs, vpt};
}
constexpr bool ln_shape_is(int b, int d4, bool wide, int vpt) {
  const LnShape s = ln_launch_shape(b, d4);
  return s.wide == wide && s.bs == (wide ? 512 : 256) && s.vpt == vpt;
}
// both sides of the 512-thread rule ...
static_assert(ln_shape_is(256, 512, true, 1) && ln_shape_is(257, 512, false, 2), "b 256 | 257 at d4 512");
static_assert(ln_shape_is(256, 511, false, 2) && ln_shape_is(256, 512, true, 1), "d4 511 | 512 at b 256");
// ... and of every values-per-thread step, d4 = k bs | k bs + 1, at 256 threads (b = 257, or d4 < 512) ...
static_assert(ln_shape_is(1, 256, false, 1) && ln_shape_is(1, 257, false, 2), "");
static_assert(ln_shape_is(257, 512, false, 2) && ln_shape_is(257, 513, false, 3), "");
static_assert(ln_shape_is(257, 768, false, 3) && ln_shape_is(257, 769, false, 4), "");
static_assert(ln_shape_is(257, 1024, false, 4) && ln_shape_is(257, 1025, false, 8), "");
static_assert(ln_shape_is(257, 2048, false, 8) && ln_shape_is(257, 2049, false, 16), "");
static_assert(ln_shape_is(257, 4096, false, 16) && ln_shape_is(257, 4097, false, -1), "");
// ... and at 512
static_assert(ln_shape_is(256, 512, true, 1) && ln_shape_is(256, 513, true, 2), "");
static_assert(ln_shape_is(256, 1024, true, 2) && ln_shape_is(256, 1025, true, 3), "");
static_assert(ln_shape_is(256, 1536, true, 3) && ln_shape_is(256, 1537, true, 4), "");
static_assert(ln_shape_is(256, 2048, true, 4) && ln_shape_is(256, 2049, true, 8), "");
static_assert(ln_shape_is(256, 4096, true, 8) && ln_shape_is(256, 4097, true, 16), "");
static_assert(ln_shape_is(256, 8192, true, 16) && ln_shape_is(256, 8193, true, -1), "");

// f(V, BS), both integral constants, for the shape's values per thread (out of Vs...) and block size; BMNAS_E_LIMIT
// when the kernel family has no instantiation that wide
template <int... Vs, class F>
inline int dispatch_ln(const LnShape& s, F&& f) {
  return dispatch_of<Vs...>(s.vpt, [&](auto V) {
    dispatch_bool(s.wide, [&](auto W) { f(V, int_c<decltype(W)::value ? 512 : 256>{}); });
  });
}

// ---- grid of the streaming kernels: one float4 per lane, at most 2048 workgroups (the kernels stride)
constexpr int stream_grid(int64_t total) {
  int64_t blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}
static_assert(stream_grid(0) == 1 && stream_grid(1) == 1 && stream_grid(256) == 1 && stream_grid(257) == 2, "");
static_assert(stream_grid(2048 * 256) == 2048 && stream_grid(2048 * 256 + 1) == 2048, "");
static_assert(stream_grid((int64_t)1 << 40) == 2048, "");

// samples walked per workgroup in the backward reductions: keep >= ~512 workgroups
constexpr int pick_chunk(int b, int slots4) {
  // 4 sample lanes walk the chunk.  Measured (MM-IMDB b = 128, dgamma atomics sharded):
  // chunk 4: 10.2 us, 8: 10.2 us, 16: 12.8 us, 32: 16.5 us.  (Before the dgamma adds were
  // sharded, small chunks were much WORSE: every extra workgroup queued on the same 4 scalars.)
  // Narrow samples (NTU / Ego: C L / 4 = 256 slots = 4 column blocks): eight-sample chunks leave 32 / 24 workgroups at
  // b = 64 / 48, each lane walking two samples in turn.  Four-sample chunks there: node_mix_bwd_k<2> 8.7 -> 6.6 us
  // (NTU b64), <3> 8.9 -> 6.8 (Ego b48); step 0.1905 -> 0.1878 ms and 0.2449 -> 0.2357 (profiles/r05_knob_sweep.txt).
  const int cols = (slots4 + 63) / 64;
  return (b >= 32 && cols * ((b + 7) / 8) >= 128) ? 8 : 4;
}
// MM-IMDB b128 at the widest sample that still takes four (7 column blocks x 16 = 112) and the first that takes eight
static_assert(pick_chunk(128, 448) == 4 && pick_chunk(128, 449) == 8, "");
static_assert(pick_chunk(64, 256) == 4 && pick_chunk(48, 256) == 4, "NTU b64, Ego b48: 4 column blocks");
static_assert(pick_chunk(31, 1 << 20) == 4 && pick_chunk(32, 1 << 20) == 8, "b 31 | 32");

// ---- entry checks
// host pointer list -> pointer array of a kernel argument block (PtrsIn::p, PtrsOut::p, ...; the caller has checked
// n against its size); a source may not be null, a destination may (the kernels skip it)
template <int N>
inline int fill_ptrs(const float* (&dst)[N], const float* const* src, int n) {
  for (int j = 0; j < n; ++j) {
    if (!src[j]) return BMNAS_E_ARG;
    dst[j] = src[j];
  }
  return 0;
}
template <int N>
inline void fill_ptrs_out(float* (&dst)[N], float* const* src, int n) {
  for (int j = 0; j < n; ++j) dst[j] = src[j];
}

// sequence lengths: the forward kernels index (l / 4) quads, the backward row reductions walk L / 4 in {1, 2, 4} lanes
constexpr bool len_fwd_ok(int L) { return L % 4 == 0 && L <= 16; }
constexpr bool len_bwd_ok(int L) { return L == 4 || L == 8 || L == 16; }

// bmnas_bn_fin_t -> BnFin; < 0 on a bad descriptor
inline int to_fin(const bmnas_bn_fin_t& f, BnFin* o) {
  o->on = f.on ? 1 : 0;
  if (!o->on) {
    *o = BnFin{};
    return 0;
  }
  if (!f.bn_w || !f.bn_b || f.shards < 0 || f.n_nbt < 0) return BMNAS_E_ARG;
  if (f.shards > 4) return BMNAS_E_LIMIT;
  if (f.training && (!f.stat || f.shards < 1)) return BMNAS_E_ARG;
  if (!f.training && (!f.running_mean || !f.running_var)) return BMNAS_E_ARG;
  if ((f.running_mean == nullptr) != (f.running_var == nullptr)) return BMNAS_E_ARG;
  o->stat = f.stat; o->conv_bias = f.conv_bias; o->bn_w = f.bn_w; o->bn_b = f.bn_b;
  o->running_mean = f.running_mean; o->running_var = f.running_var;
  o->nbt = reinterpret_cast<long long*>(f.num_batches_tracked);
  o->shards = f.shards; o->n_nbt = f.n_nbt; o->training = f.training ? 1 : 0;
  return fin_momentum(f, o);
}
// ... for a launch over b samples of length L: batch statistics need two values per channel
inline int fin_for(const bmnas_bn_fin_t& fin, int b, int L, BnFin* f) {
  if (int e = to_fin(fin, f)) return e;
  return (f->on && f->training && b * L < 2) ? BMNAS_E_ARG : 0;
}
// bn_fin_fill keeps scale | shift of the rows * C BatchNorm channels in LDS, written four adjacent channels per thread
constexpr bool fin_lds_ok(int rows, int C) { return (int64_t)rows * C <= 4096 && ((int64_t)rows * C) % 4 == 0; }

}  // namespace
