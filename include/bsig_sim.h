/*
 * bsig_sim.h — open-loop rollouts of the two analytic tasks on the device, with episode ends: the data source
 * of the (theta, trajectory) pairs the summarizers and the estimator eat.  Pendulum is the reference's numpy
 * task (pairs.pendulum_pairs states it); CartPole is not in the reference.  Companion of bsig.h (and of
 * bsig_f64.h for the double entry point), whose rules hold here too: raw DEVICE pointers, leading dimensions
 * in elements (every array here is contiguous), every call asynchronous on `stream`, no allocation, no
 * synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h.
 *
 * Definition.  Inputs: params [N, pd] (the task parameters of each episode), init [N, id] (its initial internal
 * state), actions [N, Ta, 1] (open loop; the action of step t is actions[min(t, Ta - 1)], the library's
 * padding rule), T >= 1 steps, terminate 0 / 1.  Outputs: states [N, T + 1, sd], actions_out [N, T + 1, 1],
 * lengths [N] int32, the valid STATES of each episode.
 * Arithmetic.  The internal state and every operation are in double, whatever the output type; every
 * operation below is one correctly rounded double operation in the order written (no contraction to fma),
 * sine and cosine are the device library's.  An output element is that double, stored as it is by the double
 * entry point and rounded once by the fp32 one; fp32 inputs are widened exactly.
 *
 * BSIG_SIM_PENDULUM (pd 2: length l, mass m; id 2: th, thdot; sd 3).  dt = 0.05, g = 10.
 *   u = clip(2 a, -2, 2);
 *   w = thdot + ((-3 g / (2 l)) sin(th + pi) + (3 / (m (l l))) u) dt;  th' = th + w dt;  thdot' = clip(w, -8, 8).
 *   Observation (cos th, sin th, thdot).  It never terminates.
 * BSIG_SIM_CARTPOLE (pd 3: pole mass m_p, pole half-length l, cart mass m_c; id 4 and sd 4: x, xdot, th,
 *   thdot): the frictionless equations of Barto, Sutton and Anderson (1983), Euler steps.  g = 9.8, dt = 0.02.
 *   F = 10 clip(a, -1, 1);  s = sin th, c = cos th, mt = m_p + m_c;
 *   tmp = (F + ((m_p l) (thdot thdot)) s) / mt;
 *   tha = (g s - c tmp) / (l (4/3 - (m_p (c c)) / mt));
 *   xa  = tmp - (((m_p l) tha) c) / mt;
 *   then all four components step from the OLD values: x += dt xdot, xdot += dt xa, th += dt thdot,
 *   thdot += dt tha.  The observation is the state.  It ends when the NEW state has |x| > 2.4 or
 *   |th| > 12 * 2 * pi / 360 (that constant formed in double by exactly those operations).
 * A clip passes a NaN on.
 *
 * Episode ends, with terminate = 1.  If state j (1 <= j <= T) is the first that meets the end condition,
 * L_n = j + 1: the terminal state is recorded.  States from L_n on repeat state L_n - 1; actions from step
 * L_n - 1 on repeat action L_n - 2 (pairs.end_episodes' rule; lengths is what the ragged summaries take; its
 * minimum is 2).  An episode that never ends has L_n = T + 1.
 * With terminate = 0, or for Pendulum: the physics goes on, lengths are all T + 1, actions_out[t] is the action
 * of step t for t < T and actions_out[T] repeats step T - 1.  The first L_n states of a terminate = 1 launch
 * are bitwise those of the terminate = 0 launch.
 * Non-finite values.  `nonfinite` (optional, a DEVICE int32 the caller has zeroed) is set to 1 where a stored
 * state is not finite.  Nothing is clamped or repaired; no other episode changes.
 * Two runs are bitwise equal, an episode depends neither on its neighbours nor on N, every output element is
 * written once and nothing beyond the three outputs' extents is written.  No atomics but the flag's.
 *
 * The kernel (csrc/sim.h).  One thread carries an episode through its steps; a workgroup is one wavefront of
 * BSIG_SIM_EPISODES consecutive episodes, and at most BSIG_SIM_GRID_CAP workgroups stride over the rest.  The
 * states and actions of BSIG_SIM_STEP_BLOCK consecutive state indices are staged in LDS and written out an
 * episode's contiguous run at a time, consecutive lanes on consecutive addresses, in 16-byte stores where
 * the run's address and length allow.
 */
#ifndef BSIG_SIM_H
#define BSIG_SIM_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSIG_SIM_PENDULUM 0
#define BSIG_SIM_CARTPOLE 1

#define BSIG_SIM_EPISODES 64     /* episodes (threads) of a workgroup */
#define BSIG_SIM_STEP_BLOCK 8    /* state indices staged in LDS between two write-outs */
#define BSIG_SIM_GRID_CAP 2048   /* workgroups of a launch at most */

/* The task's dimensions: params' width, the internal state's, the observation's.  BSIG_EINVAL for an unknown
 * task; a null pointer is skipped. */
int bsig_sim_dims(int task, int* pd, int* id, int* sd);

/* The rollout with fp32 data.  BSIG_EINVAL (message names the argument; checked before any launch): an unknown
 * task, T < 1, Ta < 1, n < 0, terminate not 0 / 1, a null params / init / actions / states / actions_out /
 * lengths with n > 0 (nonfinite may be null).  n == 0: BSIG_OK, nothing touched. */
int bsig_sim_rollout(int task, const float* params, const float* init, const float* actions, float* states,
                     float* actions_out, int32_t* lengths, int64_t n, int T, int Ta, int terminate,
                     int32_t* nonfinite, bsig_stream_t stream);

/* The same call on double data (the fp64 mode of bsig_f64.h). */
int bsig_sim_rollout_f64(int task, const double* params, const double* init, const double* actions,
                         double* states, double* actions_out, int32_t* lengths, int64_t n, int T, int Ta,
                         int terminate, int32_t* nonfinite, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_SIM_H */
