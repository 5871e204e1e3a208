// include/bsig_sim_policy.h with fp32 data: the packed policy's size (host arithmetic) and
// bsig_sim_rollout_policy.  The kernel is csrc/sim.h with the policy of csrc/sim_policy.h.
#include "sim_policy.h"

using namespace bsig;

extern "C" int64_t bsig_sim_policy_size(int task, int n_hidden, int h0, int h1) {
  int sd = 0;
  BSIG_TRY(sim::dims(task, nullptr, nullptr, &sd));
  BSIG_REQUIRE(n_hidden >= 0 && n_hidden <= BSIG_SIM_POLICY_MAX_HIDDEN, "sim_policy_size: n_hidden %d outside 0..%d",
               n_hidden, BSIG_SIM_POLICY_MAX_HIDDEN);
  int64_t size = 0, in = sd;
  const int widths[2] = {h0, h1};
  for (int l = 0; l < n_hidden; ++l) {
    BSIG_REQUIRE(widths[l] >= 1 && widths[l] <= BSIG_SIM_POLICY_MAX_WIDTH, "sim_policy_size: h%d %d outside 1..%d", l,
                 widths[l], BSIG_SIM_POLICY_MAX_WIDTH);
    size += in * widths[l] + widths[l];
    in = widths[l];
  }
  return size + in + 1;
}

extern "C" int bsig_sim_rollout_policy(int task, const float* params, const float* init, const float* actions,
                                       const uint8_t* replace, const double* policy, int n_hidden, int h0, int h1,
                                       int activation, float* states, float* actions_out, int32_t* lengths,
                                       int64_t n, int T, int Ta, int terminate, int32_t* nonfinite,
                                       bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sim_rollout_policy");
  return sim::run_policy<float>("sim_rollout_policy", task, params, init, actions, replace, policy, n_hidden, h0,
                                h1, activation, states, actions_out, lengths, n, T, Ta, terminate, nonfinite,
                                stream);
}
