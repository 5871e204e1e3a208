// include/bsig_sim_draws.h with double data: bsig_sim_rollout_drawn_f64, the twin of csrc/sim_draws.hip on the
// same kernel template and the same draws; the draws are the same doubles, stored unrounded.
#include "f64.h"
#include "../sim_draws.h"

using namespace bsig;

extern "C" int bsig_sim_rollout_drawn_f64(int task, const double* params, const double* init, const double* lows,
                                          const double* highs, const double* init_lows, const double* init_highs,
                                          double act_low, double act_high, double frac_rnd, double noise_std,
                                          uint64_t seed, uint64_t first_episode, const double* policy, int n_hidden,
                                          int h0, int h1, int activation, double* params_out, double* init_out,
                                          double* states, double* actions_out, int32_t* lengths,
                                          double* explore_out, uint8_t* replace_out, int64_t n, int T, int terminate,
                                          int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sim_rollout_drawn_f64");
  return sim::run_drawn<double>("sim_rollout_drawn_f64", task, params, init, lows, highs, init_lows, init_highs,
                                act_low, act_high, frac_rnd, noise_std, seed, first_episode, policy, n_hidden, h0, h1,
                                activation, params_out, init_out, states, actions_out, lengths, explore_out,
                                replace_out, n, T, terminate, nonfinite, stream);
}
