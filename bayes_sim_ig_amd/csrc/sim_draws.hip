// include/bsig_sim_draws.h with fp32 data: the generator by itself (bsig_philox4x32_10) and
// bsig_sim_rollout_drawn.  The kernel is csrc/sim.h with the draws of csrc/sim_draws.h.
#include "sim_draws.h"

using namespace bsig;

namespace {

constexpr int kPhiloxThreads = 256;

__global__ __launch_bounds__(kPhiloxThreads) void philox_kernel(const uint32_t* __restrict__ counters, uint32_t key0,
                                                                uint32_t key1, uint32_t* __restrict__ out,
                                                                int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * kPhiloxThreads + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * kPhiloxThreads) {
    const sim::Piece c = *reinterpret_cast<const sim::Piece*>(counters + 4 * i);
    const sim::Words w = sim::philox4x32_10(c.w[0], c.w[1], c.w[2], c.w[3], key0, key1);
    *reinterpret_cast<sim::Piece*>(out + 4 * i) = sim::Piece{{w.x0, w.x1, w.x2, w.x3}};
  }
}

}  // namespace

extern "C" int bsig_philox4x32_10(const uint32_t* counters, uint32_t key0, uint32_t key1, uint32_t* out, int64_t n,
                                  bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_philox4x32_10");
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "philox4x32_10: bad n=%lld", (long long)n);
  BSIG_REQUIRE(counters && out, "philox4x32_10: null counters or out");
  BSIG_REQUIRE(aligned(counters, 16) && aligned(out, 16), "philox4x32_10: counters and out must lie on 16 bytes");
  const dim3 grid(capped_grid(ceil_div<int64_t>(n, kPhiloxThreads), BSIG_SIM_GRID_CAP)), block(kPhiloxThreads);
  hipLaunchKernelGGL(philox_kernel, grid, block, 0, as_stream(stream), counters, key0, key1, out, n);
  BSIG_CHECK_LAUNCH("philox4x32_10");
  return BSIG_OK;
}

extern "C" int bsig_sim_rollout_drawn(int task, const float* params, const float* init, const double* lows,
                                      const double* highs, const double* init_lows, const double* init_highs,
                                      double act_low, double act_high, double frac_rnd, double noise_std,
                                      uint64_t seed, uint64_t first_episode, const double* policy, int n_hidden,
                                      int h0, int h1, int activation, float* params_out, float* init_out,
                                      float* states, float* actions_out, int32_t* lengths, float* explore_out,
                                      uint8_t* replace_out, int64_t n, int T, int terminate, int32_t* nonfinite,
                                      bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sim_rollout_drawn");
  return sim::run_drawn<float>("sim_rollout_drawn", task, params, init, lows, highs, init_lows, init_highs, act_low,
                               act_high, frac_rnd, noise_std, seed, first_episode, policy, n_hidden, h0, h1,
                               activation, params_out, init_out, states, actions_out, lengths, explore_out,
                               replace_out, n, T, terminate, nonfinite, stream);
}
