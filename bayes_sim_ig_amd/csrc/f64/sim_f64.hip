// include/bsig_sim.h with double data: bsig_sim_rollout_f64, the twin of csrc/sim.hip on the same kernel
// template (csrc/sim.h); the arithmetic is the same doubles, stored unrounded.
#include "f64.h"
#include "../sim.h"

using namespace bsig;

extern "C" int bsig_sim_rollout_f64(int task, const double* params, const double* init, const double* actions,
                                    double* states, double* actions_out, int32_t* lengths, int64_t n, int T,
                                    int Ta, int terminate, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sim_rollout_f64");
  return sim::run<double>("sim_rollout_f64", task, params, init, actions, states, actions_out, lengths, n, T, Ta,
                          terminate, nonfinite, stream);
}
