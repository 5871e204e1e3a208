/*
 * bsig_kme.h — the random-feature kernel mean embedding of a trajectory's transitions: the summary
 * (1/M) sum_t phi(x_t) with random Fourier features phi of the rows x_t = [s_t | a_t | s_(t+1) - s_t], a
 * fixed number of values whatever the task's dimensions and length, made from every step.  Not in the
 * reference.  Companion of bsig.h (and of bsig_f64.h for the double entry points), whose rules hold here
 * too: raw DEVICE pointers, leading dimensions in elements, every call asynchronous on `stream`, no
 * allocation, no synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h.
 *
 * Definition.  states [N, ts, sd], actions [N, ta, ad], contiguous, ts >= 1, ta >= 1; T = ts.
 *   - actions as pad_states_actions leaves them: a_t = actions[min(t, ta - 1)];
 *   - rows: diff != 0: x_t = [tau_t? | s_t | a_t | s_(t+1) - s_t] for t = 0..T-2, M = T - 1,
 *     d = 2 sd + ad (+1); diff == 0: x_t = [tau_t? | s_t | a_t], M = T, d = sd + ad (+1).  M >= 1.
 *     With time != 0 the leading column is tau_t = t * r, r = 1 / max(M - 1, 1) made on the host in the
 *     output precision: one multiplication.  The difference is one subtraction in the output precision;
 *   - coefficients coeff [m, d], pitch ld_coeff >= d, in the output precision;
 *     z_t,j = sum_k x_t,k coeff_j,k;
 *   - the output row, 2 m wide: [a/M sum_t cos z_t,j (j < m) | a/M sum_t sin z_t,j (j < m)] with
 *     a = sqrt(1/m); a/M is ONE constant made on the host in the output precision, multiplied in once at
 *     the end.
 * Arithmetic.  No atomics in the arithmetic, a fixed order of every sum (below), two runs bitwise equal,
 * a row bitwise independent of the rows around it and of N, nothing written beyond a row's 2 m elements.
 * Non-finite values.  `nonfinite` (optional, a DEVICE int32 the caller has zeroed): a non-finite OUTPUT
 * sets it to 1, as bsig_xcorr's flag word.
 *
 * The kernel (csrc/kme.h).  A workgroup of 256 threads takes a trajectory and walks it in TIME BLOCKS of
 * BSIG_KME_BLOCK_ROWS rows in ascending t; the rows of a block are formed in LDS while loading (they never
 * exist in memory), at a row pitch of d rounded up to 8 plus 1 elements (odd: the 32 rows a half-wavefront
 * reads at one k lie on 32 banks), columns d.. zero.  Column tiles of 32 frequencies are dealt to the
 * four wavefronts.  fp32: z of a (block, tile) runs on v_mfma_f32_32x32x2_f32, A from LDS, B the
 * coefficient tile read from memory in the MFMA's register layout (the same m x d matrix for every
 * workgroup: it stays in L2), k ascending in steps of 8 -- an MFMA adds the products of k0 + e and
 * k0 + 4 + e, e = 0..3 in turn.  double: one fma chain over ascending k per (row, frequency).  Then,
 * per block, cos and sin of every z (fp32: up to |z| = 8192 a Cody-Waite reduction by pi/2 and the minimax
 * polynomials of single precision, within 4e-7 of the true values; beyond, and for a non-finite z, sincosf;
 * double: sincos), rows t >= M masked out, a lane's 16 rows summed in ascending row
 * order, the two lanes of a frequency added (lower rows + upper rows), and the blocks accumulated in
 * ascending t.  A trajectory of M <= BSIG_KME_BLOCK_ROWS rows is one block; G such trajectories share a
 * workgroup's launch of loads (bsig_kme_group answers G: the largest power of two up to 8 whose blocks
 * take at most 32 KiB together; 1 for a longer trajectory).
 *
 * What is covered (the kernel's LDS arithmetic, restated by bsig_kme_fits).  A block takes
 *   BSIG_KME_BLOCK_ROWS * (round_up(d, 8) + 1) * itemsize   bytes,
 * rounded up to 16; no trajectory is refused for its length.  Only a shape whose single block is beyond
 * 160 KiB, one workgroup's LDS on gfx950, is BSIG_EUNSUPPORTED ("... LDS ..."): d above 1272 in fp32,
 * 632 in double.
 *
 * The scale.  The bandwidth of the embedding is per column: coeff[j, k] = freqs[j, k] * inv_std[k] * kappa
 * with inv_std the reciprocal standard deviation of column k over sample rows (bsig_input_norm_stats of
 * the rows bsig_kme_rows writes: 0 for a flat column, which drops out of every z) and
 * kappa = 1 / (scale * sqrt(d)) made on the host.
 */
#ifndef BSIG_KME_H
#define BSIG_KME_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows of a time block (see above). */
#define BSIG_KME_BLOCK_ROWS 32

/* d: the width of a row x_t.  -1 for sd < 1, ad < 1 or a width past 2^31 - 1. */
int64_t bsig_kme_row_dim(int sd, int ad, int diff, int time);

/* Whether a launch on trajectories of `ts` states and `ta` actions with m frequencies is covered.  Host
 * arithmetic only, no device asked: BSIG_OK, else the code (and message) the launch would return.
 * itemsize 4 (bsig_kme) or 8 (bsig_kme_f64). */
int bsig_kme_fits(int ts, int ta, int sd, int ad, int m, int diff, int time, int itemsize);

/* Trajectories that share a workgroup (G above) for that launch; the negative code where bsig_kme_fits
 * gives one. */
int bsig_kme_group(int ts, int ta, int sd, int ad, int m, int diff, int time, int itemsize);

/* The rows x_t of n trajectories as rows [n * M, d] with pitch ld_rows >= d, in fp32: a plain
 * copy / difference kernel for the one-off statistics of the scale and for tests, never on the fit path.
 * Columns >= d of a padded row are not written.  BSIG_EINVAL (message names the argument; checked before
 * any launch): ts < 1, ta < 1, sd < 1, ad < 1, M < 1, ld_rows < d, a null states / actions / rows with
 * n > 0, n < 0.  n == 0: BSIG_OK, nothing touched. */
int bsig_kme_rows(const float* states, const float* actions, float* rows, int64_t n, int ts, int ta, int sd,
                  int ad, int diff, int time, int64_t ld_rows, bsig_stream_t stream);

/* The same in double. */
int bsig_kme_rows_f64(const double* states, const double* actions, double* rows, int64_t n, int ts, int ta,
                      int sd, int ad, int diff, int time, int64_t ld_rows, bsig_stream_t stream);

/* coeff[j, k] = round(((double)freqs[j, k] * inv_std[k]) * kappa) for j < m, k < d: two double
 * multiplications, left to right, not fused, and one rounding to fp32; columns d..ld_coeff-1 are zeroed.
 * freqs: fp32 [m, d] with pitch ld_freqs >= d; inv_std: double [d]; both on the DEVICE, nothing is read
 * back.  BSIG_EINVAL: a null pointer, m < 1, d < 1, ld_freqs < d, ld_coeff < d. */
int bsig_kme_coeff(const float* freqs, int64_t ld_freqs, const double* inv_std, double kappa, float* coeff,
                   int64_t ld_coeff, int64_t m, int64_t d, bsig_stream_t stream);

/* The same with double coefficients (the product is a double already: no rounding). */
int bsig_kme_coeff_f64(const float* freqs, int64_t ld_freqs, const double* inv_std, double kappa,
                       double* coeff, int64_t ld_coeff, int64_t m, int64_t d, bsig_stream_t stream);

/* The embedding in fp32: out [n, 2 m] with pitch ld_out.  BSIG_EINVAL (message names the argument; checked
 * before any launch): ts < 1, ta < 1, sd < 1, ad < 1, M < 1 (diff with ts = 1), m < 1, ld_out < 2 m,
 * ld_coeff < d, a null states / actions / coeff / out with n > 0, n < 0.  BSIG_EUNSUPPORTED: see above.
 * n == 0: BSIG_OK, nothing touched. */
int bsig_kme(const float* states, const float* actions, const float* coeff, int64_t ld_coeff, float* out,
             int64_t n, int ts, int ta, int sd, int ad, int m, int diff, int time, int64_t ld_out,
             int32_t* nonfinite, bsig_stream_t stream);

/* The embedding in double (the fp64 mode of bsig_f64.h): as bsig_kme on double trajectories and
 * coefficients, every value a double.  The accuracy mode: a plain fma kernel on the same staging. */
int bsig_kme_f64(const double* states, const double* actions, const double* coeff, int64_t ld_coeff,
                 double* out, int64_t n, int ts, int ta, int sd, int ad, int m, int diff, int time,
                 int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_KME_H */
