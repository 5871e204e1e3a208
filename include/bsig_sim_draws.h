/*
 * bsig_sim_draws.h — rollouts whose random numbers are drawn on the device, inside the rollout kernel, by a
 * counter-based generator: an episode is a pure function of (seed, global episode index), whatever N, the order
 * of the launches or the shard that makes it.  Companion of bsig_sim_policy.h and bsig_sim.h; every rule of those
 * files (the tasks, the arithmetic, the policy, the ends and fills, the non-finite flag, fp32 = the double rounded
 * once, the invariants) holds here unless stated below.
 *
 * The generator.  Philox4x32-10 (Salmon, Moraes, Dror, Shaw: Parallel random numbers: as easy as 1, 2, 3,
 * SC 2011): multipliers M0 = 0xD2511F53, M1 = 0xCD9E8D57, key increments 0x9E3779B9, 0xBB67AE85, ten rounds.  One
 * round of the counter (c0, c1, c2, c3) under the key (k0, k1) is
 *   c' = (hi(M1 c2) ^ c1 ^ k0,  lo(M1 c2),  hi(M0 c0) ^ c3 ^ k1,  lo(M0 c0)),
 * then k0 += 0x9E3779B9, k1 += 0xBB67AE85 (mod 2^32).  Known answers, (counter, key) -> output:
 *   (0, 0, 0, 0), (0, 0)                                       -> 6627e8d5 e169c58d bc57ac4c 9b00dbd8
 *   (ffffffff x 4), (ffffffff x 2)                             -> 408f276d 41c83b0e a20bc7c6 6d5451fd
 *   (243f6a88 85a308d3 13198a2e 03707344), (a4093822 299f31d0) -> d16cfe09 94fdcceb 5001e420 24126ea1
 *
 * The draws of an episode.  The key is (seed_lo, seed_hi) of the 64-bit `seed`; the counter is
 * (g_lo, g_hi, t, purpose) with g = first_episode + n (mod 2^64) the GLOBAL index of the launch's episode n.
 * purpose 0: the draws of step t; 1: theta (t = 0); 2: the initial internal state (t = 0).  One call gives four
 * words x0..x3.  Every draw is formed in double by exactly the operations written (no contraction), then ROUNDED
 * ONCE TO THE LAUNCH'S DATA TYPE before it is used or recorded, as if it had been stored in the arrays the entry
 * points of bsig_sim.h and bsig_sim_policy.h read; x 2^-32 and x + 1 are exact.
 *   theta (purpose 1):  theta_i = low_i + ((high_i - low_i) * (x_i * 2^-32)), i < pd (pd <= 3).  low_i == high_i
 *     gives low_i exactly (the product is +0 or -0): a constant such as CartPole's cart mass.
 *   initial internal state (purpose 2): the same form with init_low_i, init_high_i, i < id (id <= 4).
 *   step t (purpose 0):
 *     the mark       r_t = (uint64) x0 < thresh,  thresh = floor(frac_rnd * 2^32) in 0..2^32
 *                    (frac_rnd = 1 marks always, 0 never);
 *     the replacement action  v_t = act_low + ((act_high - act_low) * (x1 * 2^-32));
 *     the Gaussian   z_t = sqrt(-2 * log(u1)) * cos(6.283185307179586 * u2),  u1 = (x2 + 1) * 2^-32 in (0, 1],
 *                    u2 = x3 * 2^-32 (Box and Muller; log, cos and sqrt are the device library's);
 *     the exploration term    e_t = r_t ? v_t : noise_std * z_t.  With noise_std == 0 the unreplaced e_t is +0
 *                    and neither the logarithm nor the cosine is evaluated.
 *   The action of step t.  Without a policy (a null `policy`) every step counts as marked: a_t = v_t, and the
 *   recorded mark is 1.  With a policy a_t = e_t where r_t, else pi(o_t) + e_t: the rule of bsig_sim_policy.h.
 * `params` and `init` are optional DEVICE inputs: one that is given is used as it is, copied to its `_out` array,
 * and its draw is not made (its bounds are then not read and may be null).
 *
 * Outputs.  params_out [N, pd] and init_out [N, id] (what the episode ran with), states, actions_out and lengths
 * as in bsig_sim.h, and two OPTIONAL recordings: explore_out [N, T] in the launch's type (e_t; v_t without a
 * policy) and replace_out [N, T] uint8 (r_t; 1 without a policy).  An ended episode stops drawing as it stops
 * stepping: its explore_out and replace_out from step L_n - 1 on are +0 and 0.  So bsig_sim_rollout_policy (or,
 * without a policy, bsig_sim_rollout) fed params_out, init_out, explore_out and replace_out of a launch returns
 * that launch's states, actions_out and lengths bit for bit.
 *
 * The kernel (csrc/sim.h with csrc/sim_draws.h): the rollout kernel with the draws as a further template
 * parameter.  A thread draws its own episode's numbers in registers; the launch reads no [N, T] array at all, and
 * the recordings leave through the same staged, coalesced write-out as actions_out.
 */
#ifndef BSIG_SIM_DRAWS_H
#define BSIG_SIM_DRAWS_H

#include "bsig_sim_policy.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSIG_SIM_DRAW_STEP 0      /* the counter's purpose word: the draws of step t */
#define BSIG_SIM_DRAW_THETA 1     /* theta (t = 0) */
#define BSIG_SIM_DRAW_INIT 2      /* the initial internal state (t = 0) */

/* The generator itself: out[i, 0..3] = Philox4x32-10(counters[i, 0..3], (key0, key1)) for i < n; both arrays
 * DEVICE uint32 [n, 4] on a 16-byte boundary.  BSIG_EINVAL for n < 0, a null or misaligned pointer with n > 0;
 * n == 0: BSIG_OK, nothing touched. */
int bsig_philox4x32_10(const uint32_t* counters, uint32_t key0, uint32_t key1, uint32_t* out, int64_t n,
                       bsig_stream_t stream);

/* The drawn rollout with fp32 data.  lows, highs [pd] and init_lows, init_highs [id] are HOST arrays of doubles,
 * read before the call returns.  `policy` null: no policy (n_hidden, h0, h1, activation are ignored); else the
 * packed DEVICE policy of bsig_sim_policy.h.  BSIG_EINVAL (message names the argument; checked before any
 * launch): an unknown task, T < 1, n < 0, terminate not 0 / 1; with a policy n_hidden outside 0..2, a used width
 * outside 1..64, an unknown activation; null bounds of a draw that is made, a bound that is not finite or
 * low > high (act_low, act_high always); frac_rnd outside [0, 1]; noise_std negative or not finite; a null
 * params_out / init_out / states / actions_out / lengths (explore_out, replace_out and nonfinite may be null).
 * n == 0: BSIG_OK, nothing touched. */
int bsig_sim_rollout_drawn(int task, const float* params, const float* init, const double* lows,
                           const double* highs, const double* init_lows, const double* init_highs, double act_low,
                           double act_high, double frac_rnd, double noise_std, uint64_t seed,
                           uint64_t first_episode, const double* policy, int n_hidden, int h0, int h1,
                           int activation, float* params_out, float* init_out, float* states, float* actions_out,
                           int32_t* lengths, float* explore_out, uint8_t* replace_out, int64_t n, int T,
                           int terminate, int32_t* nonfinite, bsig_stream_t stream);

/* The same call on double data. */
int bsig_sim_rollout_drawn_f64(int task, const double* params, const double* init, const double* lows,
                               const double* highs, const double* init_lows, const double* init_highs,
                               double act_low, double act_high, double frac_rnd, double noise_std, uint64_t seed,
                               uint64_t first_episode, const double* policy, int n_hidden, int h0, int h1,
                               int activation, double* params_out, double* init_out, double* states,
                               double* actions_out, int32_t* lengths, double* explore_out, uint8_t* replace_out,
                               int64_t n, int T, int terminate, int32_t* nonfinite, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_SIM_DRAWS_H */
