/*
 * bsig_xcorr.h — the time-lagged cross-correlation summary of the BayesSim paper (Ramos, Possas, Fox,
 * RSS 2019, section IV.F): for every state dimension i and action dimension j the dot product over
 * TIME of the state(-difference) series with the action series, then the mean and the standard
 * deviation of every state(-difference) series.  Not in the reference, whose cross_correlation
 * (bayes_sim_ig/utils/summarizers.py:90-122, bsig_crosscorr) subsamples the trajectory, differences
 * across the state dimension and takes the outer product of all (step, dim) entries.  Companion of
 * bsig.h (and of bsig_f64.h for the double entry point), whose rules hold here too: raw DEVICE
 * pointers, leading dimensions in elements, every call asynchronous on `stream`, no allocation, no
 * synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h.
 *
 * Definition.  states [N, ts, sd], actions [N, ta, ad], contiguous, ts >= 1, ta >= 1; T = ts.
 *   - actions as pad_states_actions leaves them: a_t = actions[min(t, ta - 1)] for t < T; actions
 *     beyond T are ignored;
 *   - state features: state_diff != 0: f_t = s_(t+1) - s_t for t = 0..T-2, M = T - 1 (the difference
 *     in time); state_diff == 0: f_t = s_t, M = T.  M >= 1;
 *   - lags tau = 0..max_lag, 0 <= max_lag <= M - 1;
 *   - c_tau[i, j] = 1/(M - tau) * sum_{t=0}^{M-tau-1} f_(t+tau),i * a_t,j   (the state responds tau
 *     steps after the action);
 *   - mu_i = 1/M sum_t f_t,i;  sigma_i = sqrt(1/M sum_t (f_t,i - mu_i)^2): the population form, in two
 *     passes (never E[f^2] - mu^2), 0 for M = 1;
 *   - the row: [c_0 | c_1 | ... | c_max_lag | mu | sigma], each c_tau flattened with i major:
 *     bsig_xcorr_dim = (max_lag + 1) sd ad + 2 sd elements, whatever the trajectory length.
 * Arithmetic.  Every output is ONE fma chain over ascending t in the output precision (mu: a chain of
 * adds); the reciprocal of the count is a constant made on the host, multiplied in once at the end.  No
 * atomics in the arithmetic, two runs are bitwise equal, a row does not depend on the rows around it,
 * each output element is written once and nothing beyond a row's width is written.
 * Non-finite values.  `nonfinite` (optional, a DEVICE int32 the caller has zeroed): a non-finite
 * OUTPUT sets it to 1, as bsig_crosscorr's flag word.
 *
 * The kernel (csrc/xcorr.h).  A workgroup of 256 threads holds G trajectories at a time, 256 / G
 * threads each, and grid-strides over the rest (bsig_xcorr_group answers G: 16 for Pendulum's 9
 * outputs, 1 from 129 outputs on; a trajectory that takes more than half a CU's LDS has 512 threads).
 * A trajectory's T sd states and M ad padded actions are staged in LDS, read from memory once; the
 * differences are formed in place there; threads own outputs and run their chains from LDS.
 *
 * What is covered (the kernel's LDS arithmetic, restated by bsig_xcorr_fits).  One trajectory takes
 *   ts * sd * itemsize  +  M * ad * itemsize   bytes
 * and the workgroup (max_lag + 2) * itemsize more for the reciprocals, each part rounded up to 16
 * bytes; a launch is covered when one trajectory and the reciprocals are at most 160 KiB, one
 * workgroup's LDS on gfx950.  G is the largest power of two up to 256 / max(16, outputs rounded up to a
 * power of two) whose trajectories take at most 64 KiB together.  A shape beyond the 160 KiB is
 * BSIG_EUNSUPPORTED ("... LDS ..."): refused, never spilled to scratch.  So is max_lag above
 * BSIG_XCORR_MAX_LAG: the reciprocals travel with the launch.  Covered, among others: ShadowHand
 * (sd 211, ad 20) up to 88 steps in double and 177 in fp32.
 */
#ifndef BSIG_XCORR_H
#define BSIG_XCORR_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSIG_XCORR_MAX_LAG 255

/* Width of a row: (max_lag + 1) * sd * ad + 2 * sd.  -1 for sd < 1, ad < 1, max_lag < 0 or a width
 * past 2^31 - 1. */
int64_t bsig_xcorr_dim(int sd, int ad, int max_lag);

/* Whether a launch on trajectories of `length` states and `ta` actions is covered.  Host arithmetic
 * only, no device asked: BSIG_OK, else the code (and message) the launch would return.  itemsize 4
 * (bsig_xcorr) or 8 (bsig_xcorr_f64). */
int bsig_xcorr_fits(int length, int ta, int sd, int ad, int max_lag, int state_diff, int itemsize);

/* Trajectories that share a workgroup (G above) for that launch; the negative code where
 * bsig_xcorr_fits gives one. */
int bsig_xcorr_group(int length, int ta, int sd, int ad, int max_lag, int state_diff, int itemsize);

/* The summary in fp32.  BSIG_EINVAL (message names the argument; checked before any launch): ts < 1,
 * ta < 1, sd < 1, ad < 1, M < 1 (state_diff with ts = 1), max_lag outside 0..M-1, ld_out below the
 * width, a null states / actions / out with n > 0, n < 0.  BSIG_EUNSUPPORTED: see above.  n == 0:
 * BSIG_OK, nothing touched. */
int bsig_xcorr(const float* states, const float* actions, float* out, int64_t n, int ts, int ta, int sd,
               int ad, int max_lag, int state_diff, int64_t ld_out, int32_t* nonfinite,
               bsig_stream_t stream);

/* The summary in double (the fp64 mode of bsig_f64.h): as bsig_xcorr on double trajectories, every
 * value a double. */
int bsig_xcorr_f64(const double* states, const double* actions, double* out, int64_t n, int ts, int ta,
                   int sd, int ad, int max_lag, int state_diff, int64_t ld_out, int32_t* nonfinite,
                   bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_XCORR_H */
