// bmnas_dropout_t (the C ABI's dropout site) -> DropCfg (what the kernels take): the one conversion.
#pragma once
#include "common.hpp"
#include "../../include/bmnas_hip.h"

namespace {

inline DropCfg to_cfg(const bmnas_dropout_t& d) {
  DropCfg c;
  c.thr = d.thr; c.scale = d.scale; c.seed = d.seed; c.offset = d.offset; c.step = d.step;
  return c;
}

}  // namespace
