// The draws of include/bsig_sim_draws.h as the Draws parameter of rollout_kernel (csrc/sim.h): what the kernel
// asks of it is episode() once per episode (theta and the initial state, drawn or the caller's) and step() in the
// walk of phase 2 (e_t and r_t of the thread's own episode).  Every draw is formed in double, uncontracted, in the
// header's order, and rounded once to T where it is returned.
//
// The design points.
// Generator: Philox4x32-10 on (g_lo, g_hi, t, purpose) under (seed_lo, seed_hi): ten rounds of two 32 x 32 -> 64
//   products (the low words by a multiply, the high words by __umulhi) and three xors, all in registers; the four
//   words are scalars, never an indexed array, so nothing goes to scratch.  One call per step serves the mark,
//   the replacement action and both uniforms of the Gaussian.
// Divergence: a marked step forms v_t alone; an unmarked one the Gaussian, unless noise_std is 0, when it forms
//   nothing.  Nothing here is a barrier, and no trip count depends on a draw.
// Bounds and the key travel in the kernel's arguments (uniform registers): no table is loaded.
#pragma once
#include "../../include/bsig_sim_draws.h"
#include "sim_policy.h"

namespace bsig {
namespace sim {

constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr int kMaxPd = 3, kMaxId = 4;
static_assert(Pendulum::pd <= kMaxPd && CartPole::pd <= kMaxPd && Pendulum::id <= kMaxId && CartPole::id <= kMaxId,
              "one call of the generator gives an episode's theta, and one its initial state");

struct Words { uint32_t x0, x1, x2, x3; };

__device__ inline Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint32_t hi0 = __umulhi(kPhiloxM0, c0), lo0 = kPhiloxM0 * c0;
    const uint32_t hi1 = __umulhi(kPhiloxM1, c2), lo1 = kPhiloxM1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return Words{c0, c1, c2, c3};
}

// x * 2^-32: exact
__device__ inline double unit(uint32_t x) { return (double)x * 0x1p-32; }

template <typename T>
struct EpisodeDraws {
  static constexpr bool kOn = true;
  uint32_t key0, key1;        // seed_lo, seed_hi
  uint64_t first;             // first_episode
  uint64_t thresh;            // floor(frac_rnd * 2^32)
  double low[kMaxPd], high[kMaxPd], init_low[kMaxId], init_high[kMaxId];
  double act_low, act_high, noise_std;
  T* params_out;              // [N, pd]
  T* init_out;                // [N, id]
  T* explore_out;             // [N, T] or null
  uint8_t* replace_out;       // [N, T] or null
  int vec_e;                  // every run of explore_out starts and ends on 16 bytes

  // Episode g's theta p [pd] and initial state s0 [id]: row `row` of the caller's arrays where given, else drawn.
  template <int pd, int id>
  __device__ void episode(uint64_t g, const T* __restrict__ params, const T* __restrict__ init, int64_t row, T* p,
                          T* s0) const {
#pragma clang fp contract(off)
    const uint32_t g_lo = (uint32_t)g, g_hi = (uint32_t)(g >> 32);
    if (params) {
#pragma unroll
      for (int c = 0; c < pd; ++c) p[c] = params[row * pd + c];
    } else {
      const Words w = philox4x32_10(g_lo, g_hi, 0u, BSIG_SIM_DRAW_THETA, key0, key1);
      const uint32_t x[4] = {w.x0, w.x1, w.x2, w.x3};
#pragma unroll
      for (int c = 0; c < pd; ++c) p[c] = (T)(low[c] + ((high[c] - low[c]) * unit(x[c])));
    }
    if (init) {
#pragma unroll
      for (int c = 0; c < id; ++c) s0[c] = init[row * id + c];
    } else {
      const Words w = philox4x32_10(g_lo, g_hi, 0u, BSIG_SIM_DRAW_INIT, key0, key1);
      const uint32_t x[4] = {w.x0, w.x1, w.x2, w.x3};
#pragma unroll
      for (int c = 0; c < id; ++c) s0[c] = (T)(init_low[c] + ((init_high[c] - init_low[c]) * unit(x[c])));
    }
  }

  // Step t of episode g: e_t rounded to T and the mark r_t; without a policy v_t and 1.
  template <bool kPolicy>
  __device__ T step(uint64_t g, int t, bool* mark) const {
#pragma clang fp contract(off)
    const Words w = philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), (uint32_t)t, BSIG_SIM_DRAW_STEP, key0, key1);
    const bool r = !kPolicy || (uint64_t)w.x0 < thresh;
    *mark = r;
    double e = 0.0;
    if (r) {
      e = act_low + ((act_high - act_low) * unit(w.x1));
    } else if (noise_std != 0.0) {
      const double u1 = ((double)w.x2 + 1.0) * 0x1p-32, u2 = unit(w.x3);
      const double z = sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2);
      e = noise_std * z;
    }
    return (T)e;
  }
};

inline bool ordered_bounds(const double* lo, const double* hi, int k) {
  for (int i = 0; i < k; ++i) {
    if (!std::isfinite(lo[i]) || !std::isfinite(hi[i]) || lo[i] > hi[i]) return false;
  }
  return true;
}

// The entry point of either type: the checks of the draws, the policy's where there is one, run()'s.
template <typename T>
int run_drawn(const char* what, int task, const T* params, const T* init, const double* lows, const double* highs,
              const double* init_lows, const double* init_highs, double act_low, double act_high, double frac_rnd,
              double noise_std, uint64_t seed, uint64_t first_episode, const double* policy, int n_hidden, int h0,
              int h1, int activation, T* params_out, T* init_out, T* states, T* actions_out, int32_t* lengths,
              T* explore_out, uint8_t* replace_out, int64_t n, int steps, int terminate, int32_t* nonfinite,
              bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  int pd = 0, id = 0;
  BSIG_TRY(dims(task, &pd, &id, nullptr));      // (an unknown task is refused here)
  BSIG_REQUIRE(params || (lows && highs), "%s: null lows or highs, and no params", what);
  BSIG_REQUIRE(params || ordered_bounds(lows, highs, pd), "%s: lows and highs must be finite with low <= high", what);
  BSIG_REQUIRE(init || (init_lows && init_highs), "%s: null init_lows or init_highs, and no init", what);
  BSIG_REQUIRE(init || ordered_bounds(init_lows, init_highs, id),
               "%s: init_lows and init_highs must be finite with low <= high", what);
  BSIG_REQUIRE(ordered_bounds(&act_low, &act_high, 1), "%s: act_low %g and act_high %g must be finite with low <= high",
               what, act_low, act_high);
  BSIG_REQUIRE(frac_rnd >= 0.0 && frac_rnd <= 1.0, "%s: frac_rnd %g outside [0, 1]", what, frac_rnd);
  BSIG_REQUIRE(std::isfinite(noise_std) && noise_std >= 0.0, "%s: noise_std %g is negative or not finite", what,
               noise_std);
  BSIG_REQUIRE(params_out, "%s: null params_out", what);
  BSIG_REQUIRE(init_out, "%s: null init_out", what);
  BSIG_REQUIRE(states, "%s: null states", what);
  BSIG_REQUIRE(actions_out, "%s: null actions_out", what);
  BSIG_REQUIRE(lengths, "%s: null lengths", what);
  EpisodeDraws<T> drw;
  drw.key0 = (uint32_t)seed;
  drw.key1 = (uint32_t)(seed >> 32);
  drw.first = first_episode;
  drw.thresh = (uint64_t)std::floor(frac_rnd * 4294967296.0);
  for (int i = 0; i < kMaxPd; ++i) {
    drw.low[i] = !params && i < pd ? lows[i] : 0.0;
    drw.high[i] = !params && i < pd ? highs[i] : 0.0;
  }
  for (int i = 0; i < kMaxId; ++i) {
    drw.init_low[i] = !init && i < id ? init_lows[i] : 0.0;
    drw.init_high[i] = !init && i < id ? init_highs[i] : 0.0;
  }
  drw.act_low = act_low;
  drw.act_high = act_high;
  drw.noise_std = noise_std;
  drw.params_out = params_out;
  drw.init_out = init_out;
  drw.explore_out = explore_out;
  drw.replace_out = replace_out;
  drw.vec_e = explore_out && aligned(explore_out, 16) && ((int64_t)steps * (int64_t)sizeof(T)) % 16 == 0;
  const T* none = nullptr;      // the launch reads no [N, T] array
  if (!policy) {
    return run<T, NoPolicy, EpisodeDraws<T>>(what, task, params, init, none, states, actions_out, lengths, n, steps,
                                             steps, terminate, nonfinite, stream, NoPolicy(), drw);
  }
  BSIG_REQUIRE(n_hidden >= 0 && n_hidden <= BSIG_SIM_POLICY_MAX_HIDDEN, "%s: n_hidden %d outside 0..%d", what,
               n_hidden, BSIG_SIM_POLICY_MAX_HIDDEN);
  BSIG_REQUIRE(n_hidden < 1 || (h0 >= 1 && h0 <= BSIG_SIM_POLICY_MAX_WIDTH), "%s: h0 %d outside 1..%d", what, h0,
               BSIG_SIM_POLICY_MAX_WIDTH);
  BSIG_REQUIRE(n_hidden < 2 || (h1 >= 1 && h1 <= BSIG_SIM_POLICY_MAX_WIDTH), "%s: h1 %d outside 1..%d", what, h1,
               BSIG_SIM_POLICY_MAX_WIDTH);
  BSIG_REQUIRE(activation == BSIG_SIM_ACT_IDENTITY || activation == BSIG_SIM_ACT_RELU ||
                   activation == BSIG_SIM_ACT_TANH,
               "%s: unknown activation %d", what, activation);
  MlpPolicy pol;
  pol.packed = policy;
  pol.replace = nullptr;
  pol.nl = n_hidden;
  pol.h0 = n_hidden >= 1 ? h0 : 0;
  pol.h1 = n_hidden == 2 ? h1 : 0;
  pol.act = activation;
  return run<T, MlpPolicy, EpisodeDraws<T>>(what, task, params, init, none, states, actions_out, lengths, n, steps,
                                            steps, terminate, nonfinite, stream, pol, drw);
}

}  // namespace sim
}  // namespace bsig
