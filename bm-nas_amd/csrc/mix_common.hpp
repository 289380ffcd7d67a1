// Helpers shared by the sources that apply / differentiate the NodeMixedOp mix as a launch of its own (bnmix.hip,
// lazyln.hip, nodemix_sel.hip): the row reduction; descriptor conversion and launch geometry come with launch.hpp.  The
// per-element arithmetic is in mix_terms.hpp, which mixconv.hip and conv1x1.hip include on its own.
#pragma once
#include "common.hpp"
#include "bn_fin.hpp"
#include "mix_terms.hpp"
#include "drop_cfg.hpp"
#include "launch.hpp"

namespace {

// reduce v over the l4n adjacent lanes that share a channel row (l4n in {1, 2, 4})
__device__ __forceinline__ float row_sum(float v, int l4n) {
  if (l4n >= 2) v += lane_xor1(v);
  if (l4n >= 4) v += lane_xor2(v);
  return v;
}

}  // namespace
