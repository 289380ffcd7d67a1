// Helpers shared by the sources that apply / differentiate the NodeMixedOp mix as a launch of its own (bnmix.hip,
// lazyln.hip, nodemix_sel.hip): row reductions, descriptor conversion, launch geometry.  The per-element arithmetic is
// in mix_terms.hpp, which mixconv.hip and conv1x1.hip include on its own.
#pragma once
#include "common.hpp"
#include "bn_fin.hpp"
#include "mix_terms.hpp"
#include "drop_cfg.hpp"

namespace {

// reduce v over the l4n adjacent lanes that share a channel row (l4n in {1, 2, 4})
__device__ __forceinline__ float row_sum(float v, int l4n) {
  if (l4n >= 2) v += lane_xor1(v);
  if (l4n >= 4) v += lane_xor2(v);
  return v;
}

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
  return 0;
}

// ---- launch geometry of the streaming mix kernels (bnmix.hip, nodemix_sel.hip)
inline int stream_grid(int64_t total) {
  int64_t blocks = (total + 255) / 256;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  return (int)blocks;
}

// samples walked per workgroup in the backward reductions: keep >= ~512 workgroups
inline int pick_chunk(int b, int slots4) {
  // 4 sample lanes walk the chunk.  Measured (MM-IMDB b = 128, dgamma atomics sharded):
  // chunk 4: 10.2 us, 8: 10.2 us, 16: 12.8 us, 32: 16.5 us.  (Before the dgamma adds were
  // sharded, small chunks were much WORSE: every extra workgroup queued on the same 4 scalars.)
  // Narrow samples (NTU / Ego: C L / 4 = 256 slots = 4 column blocks): eight-sample chunks leave 32 / 24 workgroups at
  // b = 64 / 48, each lane walking two samples in turn.  Four-sample chunks there: node_mix_bwd_k<2> 8.7 -> 6.6 us
  // (NTU b64), <3> 8.9 -> 6.8 (Ego b48); step 0.1905 -> 0.1878 ms and 0.2449 -> 0.2357 (profiles/r05_knob_sweep.txt).
  const int cols = (slots4 + 63) / 64;
  return (b >= 32 && cols * ((b + 7) / 8) >= 128) ? 8 : 4;
}

}  // namespace
