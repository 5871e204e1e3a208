/*
 * bsig_rff_bandwidth.h — the kernel bandwidth of a Random-Fourier-Feature map by the median heuristic, made on
 * the device: sigma = scale * (median pairwise distance of a sample of the rows), and coeff = freqs / sigma
 * from that device scalar.  Companion of bsig.h (and of bsig_f64.h for the double entry points), whose rules
 * hold here too: raw DEVICE pointers, leading dimensions in elements, every call asynchronous on `stream`, no
 * allocation, no synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h, arguments
 * checked before any launch.
 *
 * Why.  The features are cos / sin(x . freqs / sigma) with a sigma the caller gives (BayesSim: 4.0).  The
 * summaries differ in scale by orders of magnitude (a raw depth-3 signature: a median distance of 1.2e3; any
 * standardised summary of width I: about sqrt(2 I)), and a sigma far below the distances makes the kernel a
 * delta.  The median heuristic relates sigma to the rows.
 *
 * Definition (fixed here).  For rows x[n, width] (fp32 or double, row pitch ld >= width):
 *   - Rows used: the first m = min(n, BSIG_RFF_BANDWIDTH_MAX_ROWS).  Pairs are i < j: P = m (m - 1) / 2.
 *   - d2_ij = sum_k (x_ik - x_jk)^2 in double: each element widened to double, ONE double subtraction, then
 *     acc = fma(diff, diff, acc) over ascending k, one chain per pair.  The Gram form |x|^2 + |y|^2 - 2 x.y is
 *     NOT used (it cancels for close rows).
 *   - d2_med = the element of 0-based rank (P - 1) / 2 (integer division) of the ascending d2: the LOWER median,
 *     one of the values, never an average of two.
 *   - sigma = scale * sqrt(d2_med): one double sqrt, one double multiplication.
 *   - d2_med == 0 gives sigma = 1.0 exactly (rows that coincide carry no scale).
 *   - A non-finite d2 (any pair) gives sigma = NaN: it propagates into coeff and the features, where the
 *     estimator's non-finite flag sees it.  Nothing is reported here.
 *   - m < 2 is BSIG_EINVAL.
 * Padding: columns >= width of a pitched row are never read.  Rows >= m are never read.
 *
 * How it is made.
 *   1. Pair distances: one workgroup of 256 threads per upper-triangular tile of 64 x 64 row pairs, 4 x 4 double
 *      accumulators per thread; the two row blocks of a chunk of 32 columns are staged in LDS, widened on the
 *      way in (16-byte loads where pointer and pitch allow, element by element otherwise).  K is never split.
 *      The P values go to the workspace; only their multiset matters.
 *   2. Selection: a radix select over the bit patterns of the non-negative doubles (monotone as unsigned
 *      integers), 8 passes of 8 bits from the top.  A pass counts, per digit, the values that share the prefix
 *      decided so far: a histogram per workgroup in LDS, merged into the workspace with INTEGER atomic adds
 *      (their result does not depend on the order); every workgroup of the next pass derives the prefix and
 *      the remaining rank from the finished histograms by itself, so nothing is read back and the launches
 *      are enqueued blind.  The first pass also counts the non-finite values.  No floating-point atomics.
 *   The selection is exact and every output is one fixed chain of operations: two runs are bitwise equal, on
 *   any number of compute units.
 */
#ifndef BSIG_RFF_BANDWIDTH_H
#define BSIG_RFF_BANDWIDTH_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Rows the median is taken over, at most (see above). */
#define BSIG_RFF_BANDWIDTH_MAX_ROWS 1024

/* Bytes of workspace the selection stage needs, whatever the count. */
#define BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES 8448

/* Bytes of workspace bsig_rff_bandwidth_median / _f64 need for n rows of `width` columns: 8 P for the squared
 * distances plus BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES.  -1 for n < 2 or width < 1. */
int64_t bsig_rff_bandwidth_workspace_bytes(int64_t n, int64_t width);

/* *sigma_out (double, DEVICE) = scale * median pairwise distance of the fp32 rows x[n, width] with pitch ld,
 * by the definition above.  BSIG_EINVAL (message names the argument): a null x / sigma_out / workspace, n < 2,
 * width < 1, ld < width, a scale that is not a positive finite number, workspace_bytes below
 * bsig_rff_bandwidth_workspace_bytes, a workspace that is not 8-byte aligned. */
int bsig_rff_bandwidth_median(const float* x, int64_t ld, int64_t n, int64_t width, double scale,
                              double* sigma_out, void* workspace, size_t workspace_bytes, bsig_stream_t stream);

/* The same of double rows. */
int bsig_rff_bandwidth_median_f64(const double* x, int64_t ld, int64_t n, int64_t width, double scale,
                                  double* sigma_out, void* workspace, size_t workspace_bytes,
                                  bsig_stream_t stream);

/* The selection stage on its own: *out (double, DEVICE) = the lower median (0-based rank (count - 1) / 2 of the
 * ascending order) of values[count], a device array of non-negative doubles (sign bit clear); NaN if any value
 * is +-inf or NaN.  `values` is only read.  BSIG_EINVAL: a null pointer, count < 1 or count >= 2^31,
 * workspace_bytes below BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES, a workspace that is not 8-byte aligned. */
int bsig_rff_bandwidth_select(const double* values, int64_t count, double* out, void* workspace,
                              size_t workspace_bytes, bsig_stream_t stream);

/* coeff[r, c] = (float)((double)freqs[r, c] / *sigma_dev) for r < m, c < d; freqs is [m, d] contiguous, coeff has
 * pitch ld >= d and its columns d .. ld - 1 are set to zero (as bsig_rff_coeff leaves them).  sigma_dev is one
 * double on the DEVICE: the bandwidth never visits the host.  BSIG_EINVAL: a null pointer, m < 0, d < 1,
 * ld < d.  m == 0: BSIG_OK. */
int bsig_rff_coeff_dev(const float* freqs, const double* sigma_dev, float* coeff, int64_t m, int64_t d,
                       int64_t ld, bsig_stream_t stream);

/* The fp64 mode's coefficient: coeff[r, c] = (double)freqs[r, c] / *sigma_dev, the widened fp32 draws divided in
 * double. */
int bsig_rff_coeff_dev_f64(const float* freqs, const double* sigma_dev, double* coeff, int64_t m, int64_t d,
                           int64_t ld, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_RFF_BANDWIDTH_H */
