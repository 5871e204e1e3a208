/*
 * bsig_input_norm.h — standardisation of the estimator's input rows on the device: per-column mean and
 * reciprocal standard deviation of a block of rows, and z = (x - mean) * inv_std applied to rows.  Companion
 * of bsig.h (and of bsig_f64.h for the double entry points), whose rules hold here too: raw DEVICE pointers,
 * leading dimensions in elements, every call asynchronous on `stream`, no allocation, no synchronisation,
 * BSIG_OK or a negative code, the thread-local message of bsig.h, arguments checked before any launch.
 *
 * Why.  The path of a signature summary starts with the time index 1..L, so a level-k term reaches
 * (L-1)^k / k! and the pure time terms are the same number in every row; the reference normalises the
 * targets (normalize_samples) and never the inputs.  Raw rows of that kind saturate a tanh first layer and
 * turn cos(w.x / sigma) into noise.
 *
 * Definition (fixed here).  For rows x[n, width] (fp32 or double, row pitch ld >= width):
 *   - mean_j    = the column mean.
 *   - std_j     = sqrt(sum_i (x_ij - mean_j)^2 / n): the population form, so n = 1 is defined and gives 0.
 *   - u         = 2^-23 for fp32 rows, 2^-52 for double rows.  Column j is FLAT when
 *                 std_j <= 8 u |mean_j|, which includes std_j == 0: a spread within a few roundings of the
 *                 mean carries rounding noise only.  The rule also bounds |mean_j| / std_j by 1 / (8 u) for
 *                 every column that is kept.
 *   - inv_std_j = 0 for a flat column, otherwise 1 / std_j.
 *   - z_ij      = (x_ij - mean_j) * inv_std_j.  A flat column comes out as zero, for the rows the statistics
 *                 were made from and for any later row.
 * `mean` and `inv_std` are always double[width] on the device, whatever the rows' type.
 *
 * The apply step, per element: widen x to double, ONE double subtraction, ONE double multiplication, round
 * once to the output type (round to nearest even).  There is no fused form of subtract-then-multiply, so the
 * result is bitwise ((double)x - mean) * inv_std rounded to the rows' type, on any host as on the device.
 *
 * How the statistics are made: two launches, no atomics.
 *   1. The rows are cut into SLABS of BSIG_INPUT_NORM_SLAB_ROWS consecutive rows (a compile-time constant,
 *      independent of the device and of n; the last slab holds the remainder).  One thread owns one column
 *      of one slab -- or 16 bytes of adjacent columns (4 fp32, 2 double) where the pointer and the pitch are
 *      16-byte aligned -- and runs Welford's recurrence over the slab's rows in double, in ascending row order
 *      (count k: delta = x - mean; mean += delta * (1 / k); M2 += delta * (x - mean)).  Adjacent lanes read
 *      adjacent columns.  The partials (mean, M2) go to the caller's workspace.
 *   2. One thread per column merges the slabs in ascending order with Chan's formula
 *      (delta = mean_b - mean_a; mean = mean_a + delta * n_b / (n_a + n_b);
 *       M2 = M2_a + M2_b + delta^2 * n_a n_b / (n_a + n_b)), then writes mean and inv_std by the flat rule.
 *   Every output is one chain of operations in a fixed order: two runs are bitwise equal, on any number of
 *   compute units.  The one-pass sum-of-squares formula is NOT used (it loses log10(mean^2 / std^2) digits).
 *   A non-finite value propagates: the column's mean and inv_std come out non-finite, and so does every
 *   standardised element of that column.  Nothing is reported here; the estimator's non-finite flag sees it.
 *
 * Padding.  Columns >= width of a padded row are neither read nor written, by either call.
 */
#ifndef BSIG_INPUT_NORM_H
#define BSIG_INPUT_NORM_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows per slab of the statistics pass (see above). */
#define BSIG_INPUT_NORM_SLAB_ROWS 64

/* Bytes of workspace bsig_input_norm_stats / _f64 need for n rows of `width` columns:
 * 2 * ceil(n / BSIG_INPUT_NORM_SLAB_ROWS) * width doubles.  -1 for n <= 0 or width <= 0 (or a size past
 * 2^63 - 1). */
int64_t bsig_input_norm_workspace_bytes(int64_t n, int64_t width);

/* mean[width], inv_std[width] (double, DEVICE) of the fp32 rows x[n, width] with pitch ld.
 * BSIG_EINVAL (message names the argument): a null x / mean / inv_std / workspace, n < 1 (the statistics of
 * no rows do not exist), width < 1, ld < width, workspace_bytes below bsig_input_norm_workspace_bytes, a
 * workspace that is not 8-byte aligned. */
int bsig_input_norm_stats(const float* x, int64_t ld, int64_t n, int64_t width, double* mean,
                          double* inv_std, void* workspace, size_t workspace_bytes, bsig_stream_t stream);

/* The same of double rows (u = 2^-52 in the flat rule). */
int bsig_input_norm_stats_f64(const double* x, int64_t ld, int64_t n, int64_t width, double* mean,
                              double* inv_std, void* workspace, size_t workspace_bytes, bsig_stream_t stream);

/* out[n, width] (pitch ld_out) = (x[n, width] (pitch ld_x) - mean) * inv_std in fp32 rows.  In place
 * (out == x with ld_out == ld_x) is allowed; any other overlap of the two row blocks is BSIG_EINVAL, decided
 * from the pointer ranges on the host.  16-byte loads and stores where both pointers and both pitches allow,
 * element by element otherwise.  BSIG_EINVAL also: a null x / mean / inv_std / out with n > 0, n < 0,
 * width < 1, ld_x or ld_out below width.  n == 0: BSIG_OK, nothing touched. */
int bsig_input_norm_apply(const float* x, int64_t ld_x, const double* mean, const double* inv_std,
                          float* out, int64_t ld_out, int64_t n, int64_t width, bsig_stream_t stream);

/* The same on double rows. */
int bsig_input_norm_apply_f64(const double* x, int64_t ld_x, const double* mean, const double* inv_std,
                              double* out, int64_t ld_out, int64_t n, int64_t width, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_INPUT_NORM_H */
