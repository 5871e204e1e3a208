// include/bsig_sim_policy.h with double data: bsig_sim_rollout_policy_f64, the twin of csrc/sim_policy.hip on
// the same kernel template and the same policy; the arithmetic is the same doubles, stored unrounded.
#include "f64.h"
#include "../sim_policy.h"

using namespace bsig;

extern "C" int bsig_sim_rollout_policy_f64(int task, const double* params, const double* init,
                                           const double* actions, const uint8_t* replace, const double* policy,
                                           int n_hidden, int h0, int h1, int activation, double* states,
                                           double* actions_out, int32_t* lengths, int64_t n, int T, int Ta,
                                           int terminate, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sim_rollout_policy_f64");
  return sim::run_policy<double>("sim_rollout_policy_f64", task, params, init, actions, replace, policy, n_hidden,
                                 h0, h1, activation, states, actions_out, lengths, n, T, Ta, terminate, nonfinite,
                                 stream);
}
