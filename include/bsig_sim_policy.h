/*
 * bsig_sim_policy.h — closed-loop rollouts of the two analytic tasks: an MLP policy evaluated inside the
 * rollout kernel, step by step on each episode's own observation.  Companion of bsig_sim.h; every rule of that
 * file (the tasks, the arithmetic, the ends and fills, the non-finite flag, the invariants) holds here unless
 * stated below.
 *
 * The policy.  An MLP with n_hidden = 0, 1 or 2 hidden layers.  Layer l has W_l [out_l, in_l] row-major and
 * b_l [out_l]; in_0 = sd of the task; the hidden widths h0, h1 are 1..BSIG_SIM_POLICY_MAX_WIDTH; the last layer
 * has ONE output and no activation.  One activation code applies to all hidden layers:
 * BSIG_SIM_ACT_IDENTITY, _RELU or _TANH.  `policy` is ONE packed DEVICE array of doubles, whatever the data
 * type of the launch: W_0, b_0, W_1, b_1, ... in that order, bsig_sim_policy_size() doubles in all (fp32 weights
 * are widened exactly when packed).
 * Arithmetic: double and uncontracted, like bsig_sim.h.  z_j = b_j, then for k ascending
 * z_j = z_j + (W_jk * x_k): two roundings a term.  relu(z) = z < 0 ? 0 : z (a NaN passes, as clip passes it);
 * tanh is the device library's.
 * The input is the observation o_t in double exactly as the task forms it, BEFORE any rounding to fp32:
 * Pendulum (cos th, sin th, thdot), CartPole the state.
 *
 * The action of step t.  With e_t = actions[n, min(t, Ta - 1)] and r_t = replace[n, min(t, Ta - 1)]
 * (`replace`: an optional DEVICE uint8 array [N, Ta]; null means all 0):
 *   a_t = e_t               where r_t != 0,
 *   a_t = pi(o_t) + e_t     otherwise (one add).
 * a_t is what the task's step takes (the task clips inside) and what actions_out[t] records.  So e = 0, r = 0 is
 * the policy alone; r Bernoulli with e uniform where replaced is the reference's policy_rl_randomized; e
 * Gaussian with r = 0 is additive exploration noise; r = 1 is the open-loop launch of bsig_sim.h.
 *
 * Ends and fills are exactly the open-loop rules: an ended episode's thread evaluates nothing more,
 * actions_out[T] repeats step T - 1.  The fp32 outputs are the double outputs rounded once (the step takes the
 * double a_t, actions_out its rounding).  Two runs are bitwise equal; an episode depends neither on its
 * neighbours nor on N; no barrier and no trip count depends on the data.
 *
 * The kernel (csrc/sim.h, csrc/sim_policy.h): the rollout kernel of bsig_sim.h with the policy as a template
 * parameter.  The weights are staged once per workgroup in LDS; its size follows the policy's widths.
 */
#ifndef BSIG_SIM_POLICY_H
#define BSIG_SIM_POLICY_H

#include "bsig_sim.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSIG_SIM_ACT_IDENTITY 0
#define BSIG_SIM_ACT_RELU 1
#define BSIG_SIM_ACT_TANH 2

#define BSIG_SIM_POLICY_MAX_HIDDEN 2   /* hidden layers at most */
#define BSIG_SIM_POLICY_MAX_WIDTH 64   /* units of a hidden layer at most */
#define BSIG_SIM_POLICY_UNITS 4        /* units of a layer the kernel forms side by side */

/* The doubles of the packed policy of `task` with n_hidden hidden layers of h0 (and h1) units; widths beyond
 * n_hidden are ignored.  A negative code for an unknown task, n_hidden outside 0..2 or a width outside 1..64. */
int64_t bsig_sim_policy_size(int task, int n_hidden, int h0, int h1);

/* The closed-loop rollout with fp32 data.  BSIG_EINVAL (message names the argument; checked before any
 * launch): everything bsig_sim_rollout checks, a null `policy` with n > 0, n_hidden outside 0..2, a used width
 * outside 1..64, an unknown activation.  `replace` may be null.  n == 0: BSIG_OK, nothing touched. */
int bsig_sim_rollout_policy(int task, const float* params, const float* init, const float* actions,
                            const uint8_t* replace, const double* policy, int n_hidden, int h0, int h1,
                            int activation, float* states, float* actions_out, int32_t* lengths, int64_t n, int T,
                            int Ta, int terminate, int32_t* nonfinite, bsig_stream_t stream);

/* The same call on double data. */
int bsig_sim_rollout_policy_f64(int task, const double* params, const double* init, const double* actions,
                                const uint8_t* replace, const double* policy, int n_hidden, int h0, int h1,
                                int activation, double* states, double* actions_out, int32_t* lengths, int64_t n,
                                int T, int Ta, int terminate, int32_t* nonfinite, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_SIM_POLICY_H */
