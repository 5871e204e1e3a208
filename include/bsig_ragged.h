/*
 * bsig_ragged.h — per-trajectory lengths for the two summaries that read the whole trajectory: the
 * time-lagged cross-correlation (bsig_xcorr.h) and the kernel mean embedding (bsig_kme.h).  Recorded
 * episodes end early and the recorder fills the tail with the last state (pad_states_actions); on those
 * two summaries the filled tail changes every count, mean and deviation.  Here the caller says how long
 * each trajectory is.  Companion of bsig_xcorr.h and bsig_kme.h, whose definitions, layouts and rules
 * (raw DEVICE pointers, leading dimensions in elements, every call asynchronous on `stream`, no
 * allocation, no synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h) hold
 * here too.
 *
 * Definition.  states [N, ts, sd], actions [N, ta, ad] as in the parent headers, and lengths [N], a
 * DEVICE int32 vector: lengths[n] = L_n is the number of valid STATES of trajectory n,
 * Lmin <= L_n <= ts with Lmin = 2 where differences are formed (state_diff / diff) and 1 where not.
 * Row n is what the parent header's definition gives for states[n, :L_n] and the whole actions[n], with
 * T = L_n in every formula:
 *   - a_t = actions[n, min(t, ta - 1)] for t < T;
 *   - M_n = L_n - 1 steps, or L_n without differences;
 *   - xcorr: the reciprocals 1/(M_n - tau) and 1/M_n; max_lag is checked against the M of `ts` on the
 *     host, and for a trajectory with tau >= M_n (a lag with no term) the block c_tau is exactly +0;
 *   - kme: r = 1 / max(M_n - 1, 1) and a/M_n.
 * Nothing at or beyond state L_n of a trajectory, and no action of a step t >= M_n, enters any output.
 * A length outside [Lmin, ts], which only the device sees: every element of that row is NaN and
 * `nonfinite` is set; no other row changes; the length is clamped into the range before it indexes
 * anything, so no address outside the trajectory is read.
 * Arithmetic.  Row n is BITWISE the row the parent's fixed-length entry point returns for the one
 * trajectory sliced to L_n, in fp32 and in double, whatever the trajectories around it; with every
 * L_n = ts a call is bitwise the fixed-length call.  The kernels are the parents' (csrc/xcorr.h,
 * csrc/kme.h: one chain per output in ascending t; ascending blocks of BSIG_KME_BLOCK_ROWS rows with
 * masked rows) with the trajectory's own step count; the constants the parents' hosts make -- (T)1 /
 * (T)(M - tau), (T)1 / (T)max(M - 1, 1), (T)(sqrt(1.0 / m) / (double)M) -- are made on the device by the
 * same correctly rounded divisions in the same types (the root stays on the host).  No atomics in the
 * arithmetic, two runs bitwise equal, nothing written beyond a row's width.
 *
 * What is covered: what the fixed-length launch at `ts` covers (bsig_xcorr_fits, bsig_kme_fits: the same
 * codes and messages).  The launch shape comes from `ts` as well; only where bsig_xcorr_group answers
 * G > 1 the workgroup holds G sets of reciprocals instead of one, (G - 1) (max_lag + 2) elements more,
 * and G is halved where that passes 64 KiB.
 */
#ifndef BSIG_RAGGED_H
#define BSIG_RAGGED_H

#include "bsig_kme.h"
#include "bsig_xcorr.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bsig_xcorr with lengths, in fp32.  BSIG_EINVAL (message names the argument; checked before any
 * launch): everything bsig_xcorr refuses, and a null lengths with n > 0.  BSIG_EUNSUPPORTED: as
 * bsig_xcorr at `ts`.  n == 0: BSIG_OK, nothing touched. */
int bsig_xcorr_ragged(const float* states, const float* actions, const int32_t* lengths, float* out,
                      int64_t n, int ts, int ta, int sd, int ad, int max_lag, int state_diff,
                      int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream);

/* The same in double. */
int bsig_xcorr_ragged_f64(const double* states, const double* actions, const int32_t* lengths,
                          double* out, int64_t n, int ts, int ta, int sd, int ad, int max_lag,
                          int state_diff, int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream);

/* bsig_kme with lengths, in fp32 (on v_mfma_f32_32x32x2_f32 as bsig_kme): G comes from `ts`, a
 * trajectory walks ceil(M_n / BSIG_KME_BLOCK_ROWS) blocks.  BSIG_EINVAL: everything bsig_kme refuses, and
 * a null lengths with n > 0.  BSIG_EUNSUPPORTED: as bsig_kme at `ts`.  n == 0: BSIG_OK, nothing touched. */
int bsig_kme_ragged(const float* states, const float* actions, const int32_t* lengths, const float* coeff,
                    int64_t ld_coeff, float* out, int64_t n, int ts, int ta, int sd, int ad, int m, int diff,
                    int time, int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream);

/* The same in double. */
int bsig_kme_ragged_f64(const double* states, const double* actions, const int32_t* lengths,
                        const double* coeff, int64_t ld_coeff, double* out, int64_t n, int ts, int ta, int sd,
                        int ad, int m, int diff, int time, int64_t ld_out, int32_t* nonfinite,
                        bsig_stream_t stream);

/* The VALID rows x_t only, compacted, in fp32: trajectory n's M_n rows start at row offsets[n] of `rows`
 * (pitch ld_rows >= d), offsets a DEVICE int64 vector, the exclusive prefix sum of the M_n, which the
 * caller makes; rows beyond the total are not touched.  A length outside [Lmin, ts] is clamped into it:
 * the caller's offsets decide where its rows go.  For the one-off statistics of the scale and for tests,
 * never on the fit path.  BSIG_EINVAL: everything bsig_kme_rows refuses, and a null lengths or offsets
 * with n > 0.  n == 0: BSIG_OK, nothing touched. */
int bsig_kme_rows_ragged(const float* states, const float* actions, const int32_t* lengths,
                         const int64_t* offsets, float* rows, int64_t n, int ts, int ta, int sd, int ad,
                         int diff, int time, int64_t ld_rows, bsig_stream_t stream);

/* The same in double. */
int bsig_kme_rows_ragged_f64(const double* states, const double* actions, const int32_t* lengths,
                             const int64_t* offsets, double* rows, int64_t n, int ts, int ta, int sd, int ad,
                             int diff, int time, int64_t ld_rows, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_RAGGED_H */
