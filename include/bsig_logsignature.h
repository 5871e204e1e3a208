/*
 * bsig_logsignature.h — the log-signature of a trajectory at the Lyndon words (what `signatory` calls
 * logsignature(path, depth, mode="words")), as an epilogue on the general signature kernel.  Companion
 * of bsig_signature.h (and of bsig_f64.h for the double entry point), whose rules hold here too: raw
 * DEVICE pointers, leading dimensions in elements, every call asynchronous on `stream`, no allocation,
 * no synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h.
 *
 * Definition (fixed here: `signatory` is not at hand, exactly as for the signature).
 *   - The path is X_l = [l + 1 | picked channels] of dimension d = 1 + n_channels, as in
 *     bsig_signature.h; S is its signature truncated at `depth`, S_() = 1.
 *   - log S = sum_{n=1..depth} (-1)^(n+1)/n (S - 1)^(x)n in the truncated tensor algebra.
 *   - The output row holds the coefficients of log S at the LYNDON WORDS over the alphabet
 *     0 < 1 < ... < d-1 (letter 0 is the time channel): the words strictly smaller than all their proper
 *     rotations, lengths 1..depth, ordered by length, then lexicographically.  d = 2, depth 4:
 *     0, 1, 01, 001, 011, 0001, 0011, 0111.
 *   - The width is Witt's formula, sum_{k=1..depth} (1/k) sum_{e | k} mu(e) d^(k/e): 2 860 for d = 10 at
 *     depth 4 (the signature: 11 110), 3 795 for d = 22 at depth 3 (11 154), 964 for d = 4 at depth 6
 *     (5 460).  These coordinates determine the whole truncated signature.
 *
 * What the kernel evaluates, per word w of length k: the same series, term by term,
 *   (log S)_w = sum over the 2^(k-1) ways to cut w into n >= 1 consecutive non-empty pieces u1..un
 *               of (-1)^(n+1)/n S_u1 S_u2 ... S_un
 * The cuts are enumerated by ascending bit mask (bit j set: a cut after letter j) and accumulated in that
 * order, each product from the left with its coefficient last: every output is ONE chain, no atomics, two
 * runs are bitwise equal, each output element is written once.  Level 1 is S_1 itself, bit for bit.
 *
 * Routing.  depth 1 (given, or by the reference's rule on d) is bsig_signature_ex / _f64 at depth 1,
 * unchanged: the log-signature IS level 1 there, and `words` is not read.  Every other call runs the
 * log-signature kernel of csrc/logsignature.h, channels == NULL at depth <= 3 included (the tuned depth
 * <= 3 kernels of bsig.h keep their levels in registers and have no epilogue).  That kernel is the path
 * loop of the general signature kernel (csrc/signature_ex.h: the same LDS layout, the same chains, one
 * workgroup per trajectory, grid-striding), so the levels it holds when a path ends are bitwise what
 * bsig_signature_ex returns with a non-NULL `channels`; the store of the levels is replaced by the
 * epilogue above, which reads them from LDS.  The [N, width] signature never goes to memory.
 *
 * What is covered.  The epilogue needs no LDS of its own: the need is EXACTLY the general signature
 * kernel's, and bsig_signature_ex_fits(path_dim, length, depth, itemsize) answers for both.  What it
 * refuses is BSIG_EUNSUPPORTED ("... LDS ...") here too.
 *
 * The words table.  `words` is a DEVICE int32[bsig_logsignature_dim(d, depth)]: per output element, the
 * flat offset of its word in the signature row (levels concatenated, each in C order).
 * bsig_logsignature_words fills it on the host, the caller uploads it (once per (d, depth) and device).
 * THE LIBRARY CANNOT RANGE-CHECK A DEVICE ARRAY: an entry outside [0, bsig_signature_ex_dim(d, depth))
 * reads LDS out of bounds, and a table made for another (d, depth) gives other coordinates.  The same
 * caveat holds for `channels`, as in bsig_signature.h.
 */
#ifndef BSIG_LOGSIGNATURE_H
#define BSIG_LOGSIGNATURE_H

#include "bsig_signature.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Width of a log-signature row: the number of Lyndon words of length 1..depth over path_dim letters.
 * -1 where bsig_signature_ex_dim(path_dim, depth) is: path_dim < 2, depth outside
 * 1..BSIG_SIGNATURE_MAX_DEPTH, or a signature width past 2^31 - 1. */
int64_t bsig_logsignature_dim(int path_dim, int depth);

/* The offset table of (path_dim, depth) in output order, written to the HOST array words_host: host
 * arithmetic only (Duval's algorithm), no device asked.  BSIG_EINVAL: no width for (path_dim, depth), a
 * null words_host, capacity (in elements) below the width.  Nothing is written then. */
int bsig_logsignature_words(int path_dim, int depth, int32_t* words_host, int64_t capacity);

/* The log-signature of [t | picked channels] in fp32: the arguments of bsig_signature_ex plus `words`.
 * depth <= 0: the reference's rule on d.  BSIG_EINVAL (message names the argument; checked before any
 * launch): what bsig_signature_ex reports -- depth above BSIG_SIGNATURE_MAX_DEPTH, length < 2, a null
 * states / actions / out with n > 0, channels != NULL with n_channels < 1 --, a null `words` at depth
 * >= 2, ld_out below bsig_logsignature_dim(d, depth).  BSIG_EUNSUPPORTED: see above.  n == 0: BSIG_OK,
 * nothing touched. */
int bsig_logsignature(const float* states, const float* actions, const int32_t* channels, int n_channels,
                      const int32_t* words, float* out, int64_t n, int length, int sd, int ad, int depth,
                      int64_t ld_out, bsig_stream_t stream);

/* The same in double (the fp64 mode of bsig_f64.h): double trajectories, every value a double. */
int bsig_logsignature_f64(const double* states, const double* actions, const int32_t* channels,
                          int n_channels, const int32_t* words, double* out, int64_t n, int length, int sd,
                          int ad, int depth, int64_t ld_out, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_LOGSIGNATURE_H */
