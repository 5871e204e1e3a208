/*
 * bsig_sysid.h — the least-squares dynamics summary of a trajectory: the ridge fit of the state's step
 * s_(t+1) - s_t on [1 | s_t | a_t] over the trajectory's own steps (the classic system-identification
 * statistic), and the root mean square of what the fit leaves.  Not in the reference.  Companion of bsig.h
 * (and of bsig_f64.h for the double entry point), whose rules hold here too: raw DEVICE pointers, leading
 * dimensions in elements, every call asynchronous on `stream`, no allocation, no synchronisation, BSIG_OK
 * or a negative code, the thread-local message of bsig.h.
 *
 * Definition.  states [N, ts, sd], actions [N, ta, ad], contiguous, ts >= 2, ta >= 1.
 *   - actions as pad_states_actions leaves them: a_t = actions[min(t, ta - 1)]; M = ts - 1 steps,
 *     p = 1 + sd + ad regressors; actions from step M on are ignored;
 *   - phi_t = [1 | s_t | a_t] and y_t = s_(t+1) - s_t for t = 0..M-1;
 *   - G = 1/M sum_t phi_t phi_t^T (p x p), B = 1/M sum_t phi_t y_t^T (p x sd);
 *   - rho = ridge * trace(G) / p.  The intercept column makes trace(G) >= 1, so G + rho I is positive
 *     definite for every finite trajectory, a constant one included;
 *   - W = (G + rho I)^(-1) B;  r_j = sqrt(1/M sum_t (y_tj - phi_t . W_:j)^2);
 *   - the row: [W row-major (p * sd numbers) | r (sd numbers)]: bsig_sysid_dim = (1 + sd + ad) sd + sd
 *     elements (Pendulum 18, Ant 4 200, ShadowHand 49 163), whatever the trajectory's length.
 * Conditioning.  The eigenvalues of G + rho I lie in [rho, trace(G) + rho], so its condition number is at
 * most 1 + p / ridge.  A Cholesky solve in a precision of unit roundoff u loses about p^2 u (1 + p / ridge)
 * relative to ||W||; where p^2 u / ridge nears 1 (fp32: ridge 1e-6 on Ant) the remedy is the double entry
 * point, not a larger ridge picked by the library.
 *
 * Which system a launch solves: a function of the shape only.
 *   - p <= M: the primal p x p system above; the residuals are formed from W and the staged trajectory.
 *   - M <  p: the dual M x M system.  With Phi [M, p] and Y [M, sd] the rows phi_t and y_t, K = Phi Phi^T / M
 *     and alpha = (K + rho I)^(-1) Y:  W = Phi^T alpha / M, the same W, and the residual y_t - phi_t . W is
 *     rho alpha_t exactly, which is how r is formed.  rho there is ridge * trace(K) / p (trace(K) = trace(G)).
 * So the factorised matrix is min(p, M) squared, whatever the task's width.
 * Arithmetic.  Every sum is one fma chain in a fixed ascending order in the output precision; the Cholesky
 * factorisation and the two triangular solves divide and take roots correctly rounded.  No atomics in the
 * arithmetic, two runs are bitwise equal, a row depends neither on the rows around it nor on N, each output
 * element is written once and nothing beyond a row's width is written.
 * Non-finite values.  `nonfinite` (optional, a DEVICE int32 the caller has zeroed) is set to 1, and the
 * WHOLE row is NaN, where a value of the trajectory that enters the definition is not finite or a pivot
 * of the factorisation is not positive and finite (rounding can produce one at a tiny ridge in fp32).  An
 * output element that overflows without either sets the flag as well.  No other row changes.
 *
 * The kernel (csrc/sysid.h).  A workgroup of 256 threads holds G trajectories at a time, 256 / G threads
 * each, and grid-strides over the rest (bsig_sysid_group answers G: 16 for Pendulum, 1 for Ant).  A
 * trajectory is staged in LDS once, as the rows [1 | s_t | a_t]; the Gram and cross products, the
 * factorisation, the solves for all sd right-hand sides and the residuals run from there.
 *
 * What is covered (the kernel's LDS arithmetic, restated by bsig_sysid_fits).  With k = min(p, M) one
 * trajectory takes 16 bytes and, in elements of itemsize bytes,
 *   ts * (p | 1)  +  k * (k | 1)  +  k * sd  +  (primal only) nseg * sd,
 * nseg = min(max(threads of the trajectory / sd, 1), M) the runs of steps the residuals' sums are cut into,
 * each part rounded up to 16 bytes; a launch is covered when that is at most 160 KiB, one workgroup's LDS
 * on gfx950.  G is the largest power of two up to 16 with 256 / G threads at most the row's width (from 32
 * outputs on) whose trajectories take at most 64 KiB together.  A shape beyond the 160 KiB is
 * BSIG_EUNSUPPORTED ("... LDS ..."): refused, never spilled to scratch.
 * Covered, among others: Pendulum (sd 3, ad 1), Ant (60, 8) at 50 and 100 states in fp32 and double,
 * ShadowHand (211, 20) at 50 states in fp32.  ShadowHand at 50 states in double is NOT covered (195 152 B).
 */
#ifndef BSIG_SYSID_H
#define BSIG_SYSID_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Width of a row: (1 + sd + ad) * sd + sd.  -1 for sd < 1, ad < 1 or a width past 2^31 - 1. */
int64_t bsig_sysid_dim(int sd, int ad);

/* Whether a launch on trajectories of `ts` states and `ta` actions is covered.  Host arithmetic only, no
 * device asked: BSIG_OK, else the code (and message) the launch would return.  itemsize 4 (bsig_sysid) or
 * 8 (bsig_sysid_f64). */
int bsig_sysid_fits(int ts, int ta, int sd, int ad, int itemsize);

/* Trajectories that share a workgroup (G above) for that launch; the negative code where bsig_sysid_fits
 * gives one. */
int bsig_sysid_group(int ts, int ta, int sd, int ad, int itemsize);

/* The summary in fp32.  BSIG_EINVAL (message names the argument; checked before any launch): ts < 2, ta < 1,
 * sd < 1, ad < 1, a ridge that is not a positive finite number (in fp32 too), ld_out below the width, a
 * null states / actions / out with n > 0, n < 0.  BSIG_EUNSUPPORTED: see above.  n == 0: BSIG_OK, nothing
 * touched. */
int bsig_sysid(const float* states, const float* actions, float* out, int64_t n, int ts, int ta, int sd,
               int ad, double ridge, int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream);

/* The summary in double (the fp64 mode of bsig_f64.h): as bsig_sysid on double trajectories, every value a
 * double. */
int bsig_sysid_f64(const double* states, const double* actions, double* out, int64_t n, int ts, int ta,
                   int sd, int ad, double ridge, int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_SYSID_H */
