// A trajectory's own length (include/bsig_ragged.h) as the kernels of csrc/xcorr.h and csrc/kme.h take it.
#pragma once
#include <cstdint>

#include "common.h"

namespace bsig {
namespace ragged {

struct Steps {
  int steps;       // M_n of the length clamped into [Lmin, ts]: what may index the trajectory
  bool valid;      // the length as given was inside the range
};

// lengths[traj] as feature steps.  `diff`: differences are formed (Lmin = 2, M = L - 1), else Lmin = 1, M = L.
__device__ __forceinline__ Steps steps_of(const int32_t* __restrict__ lengths, int64_t traj, int ts, int diff) {
  const int len = lengths[traj], lmin = diff ? 2 : 1;
  Steps s;
  s.valid = len >= lmin && len <= ts;
  s.steps = min(max(len, lmin), ts) - (diff ? 1 : 0);
  return s;
}

}  // namespace ragged
}  // namespace bsig
