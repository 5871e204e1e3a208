/*
 * bsig_signature.h — path signatures beyond depth 3 and on a chosen subset of channels: the general
 * form of bsig_signature / bsig_signature_f64.  Companion of bsig.h (and of bsig_f64.h for the double
 * entry point), whose rules hold here too: raw DEVICE pointers, leading dimensions in elements, every
 * call asynchronous on `stream`, no allocation, no synchronisation, BSIG_OK or a negative code, the
 * thread-local message of bsig.h.
 *
 * The reference (bayes_sim_ig/utils/summarizers.py:144-168) builds the path [t | all states | all
 * actions] and hands it to `signatory`, which takes any depth; its own depth rule (:133-141) caps a
 * level at 110^2 = 12 100 terms and never looks past depth 3.  Here:
 *   - depth is 1..BSIG_SIGNATURE_MAX_DEPTH (depth <= 0: the reference's rule applied to the path
 *     dimension d);
 *   - the path is X_l = [l + 1 | picked channels], d = 1 + n_channels.  `channels` is a DEVICE
 *     int32[n_channels], or NULL for all sd + ad channels in order (n_channels is then ignored).
 *     Entry c < sd picks states[..., c], any other entry picks actions[..., c - sd].  Any order,
 *     repeats allowed.  The time channel is generated, the picked channels are gathered straight from
 *     `states` / `actions` (states [N, length, sd], actions [N, length, ad], contiguous): no compacted
 *     copy of the trajectories exists.
 *     THE LIBRARY CANNOT RANGE-CHECK A DEVICE ARRAY: an entry outside [0, sd + ad) reads out of
 *     bounds.  The caller checks the list on the host (bayes_sim_ig_amd.summarizers does).
 *   - the output row is signatory's: levels 1..depth concatenated, each flattened in C order,
 *     bsig_signature_ex_dim(d, depth) elements.
 *
 * Routing.  channels == NULL with depth <= 3 is exactly bsig_signature / bsig_signature_f64: the
 * same launch, the same refusals, the same bits.  Every other call -- depth 4..6, or ANY non-NULL
 * `channels`, the identity list included -- runs the general kernel of csrc/signature_ex.h.
 *
 * The general kernel.  One workgroup per trajectory, grid-striding over the rest (at most as many
 * workgroups as the other summarizers of the precision launch).  All levels of a trajectory stay in
 * the workgroup's LDS for the whole path; per segment, Chen's identity in Horner form
 *   S_k[i1..ik] += (...((D[i1]/k + S_1[i1]) D[i2]/(k-1) + S_2[i1,i2]) D[i3]/(k-2) ...) D[ik]
 * with the reciprocals as constants.  Every output is ONE chain in ascending segment order: no
 * atomics, two runs are bitwise equal, each output element is written once.  Level 1 is the sum of
 * the increments (the depth <= 3 kernels of bsig.h take last - first: the two agree to rounding, not
 * bitwise).  Depth 1 reads the first and the last point only and needs no LDS.
 *
 * What is covered (the kernel's LDS arithmetic, restated by bsig_signature_ex_fits).  With
 * w_k = d^k, low = w_1 + ... + w_(depth-1), rows = 1 + d + ... + d^(depth-1), a workgroup holds
 *   (2 low + w_depth + (length - 1) d + 8) * itemsize  +  8 rows  +  4 d   bytes
 * (the levels below the top twice: a segment reads one copy and writes the other), each part rounded
 * up to 16 bytes, and a launch is covered when that is at most 160 KiB, one workgroup's LDS on gfx950.
 * A shape beyond it is BSIG_EUNSUPPORTED ("... LDS ..."): refused, never spilled to scratch.  Covered
 * in both precisions, among others: depth 4 at d <= 10, depth 5 at d <= 6, depth 6 at d <= 4 (every
 * d^depth <= 12 100, the reference's cap), depth 3 at d <= 22, each up to length 64; depth 2 at
 * d <= 110 up to length 32; depth 1 at any d and length.
 */
#ifndef BSIG_SIGNATURE_H
#define BSIG_SIGNATURE_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSIG_SIGNATURE_MAX_DEPTH 6

/* Width of a signature row (summarizers.py:144-168: signatory's output): sum_{k=1..depth} path_dim^k.
 * -1 for path_dim < 2, depth outside 1..BSIG_SIGNATURE_MAX_DEPTH, or a width past 2^31 - 1. */
int64_t bsig_signature_ex_dim(int path_dim, int depth);

/* Whether the general kernel covers a launch on paths of `length` points of dimension `path_dim`
 * (summarizers.py:144-168 at any depth).  Host arithmetic only, no device asked: BSIG_OK, else the code
 * (and message) the launch would return.  itemsize 4 (bsig_signature_ex) or 8 (bsig_signature_ex_f64).
 * depth <= 0: the reference's rule.  It answers for the GENERAL kernel, also where a launch with
 * channels == NULL and depth <= 3 would be routed to bsig_signature / bsig_signature_f64. */
int bsig_signature_ex_fits(int path_dim, int length, int depth, int itemsize);

/* summary_signatory, summarizers.py:144-168, in fp32: the signature of [t | picked channels], levels
 * 1..depth.  BSIG_EINVAL (message names the argument; checked before any launch): depth above
 * BSIG_SIGNATURE_MAX_DEPTH, length < 2, ld_out below the width, a null states / actions / out with
 * n > 0, channels != NULL with n_channels < 1.  BSIG_EUNSUPPORTED: see above.  n == 0: BSIG_OK,
 * nothing touched. */
int bsig_signature_ex(const float* states, const float* actions, const int32_t* channels, int n_channels,
                      float* out, int64_t n, int length, int sd, int ad, int depth, int64_t ld_out,
                      bsig_stream_t stream);

/* summary_signatory, summarizers.py:144-168, in double (the fp64 mode of bsig_f64.h): as
 * bsig_signature_ex on double trajectories, every value a double. */
int bsig_signature_ex_f64(const double* states, const double* actions, const int32_t* channels,
                          int n_channels, double* out, int64_t n, int length, int sd, int ad, int depth,
                          int64_t ld_out, bsig_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_SIGNATURE_H */
