// include/bsig_sim.h with fp32 data: the dimensions' query (host arithmetic) and bsig_sim_rollout.  The
// kernel, the two tasks and the launch shape are csrc/sim.h.
#include "sim.h"

using namespace bsig;

extern "C" int bsig_sim_dims(int task, int* pd, int* id, int* sd) { return sim::dims(task, pd, id, sd); }

extern "C" int bsig_sim_rollout(int task, const float* params, const float* init, const float* actions,
                                float* states, float* actions_out, int32_t* lengths, int64_t n, int T, int Ta,
                                int terminate, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sim_rollout");
  return sim::run<float>("sim_rollout", task, params, init, actions, states, actions_out, lengths, n, T, Ta,
                         terminate, nonfinite, stream);
}
