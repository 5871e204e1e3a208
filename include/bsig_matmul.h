/*
 * bsig_matmul.h — the matmul precision of libbsig_hip.so's fp32 products: what
 * torch.set_float32_matmul_precision('high') means elsewhere ("TF32 or bf16x3"), built for gfx950,
 * which has no xf32/TF32 MFMA.  Companion of bsig.h, whose rules hold here too: raw DEVICE pointers,
 * leading dimensions in elements, every call asynchronous on `stream`, no allocation, no
 * synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h.
 *
 * BSIG_MATMUL_FP32 (the default everywhere): v_mfma_f32_32x32x2_f32 / 16x16x4_f32, the reference's
 * fp32 arithmetic -- the library issues exactly the launches it issues without this header.
 *
 * BSIG_MATMUL_SPLIT_BF16 (opt-in): every fp32 operand element x is split into three bf16 pieces,
 *   p0 = bf16_rne(x),  p1 = bf16_rne(x - p0),  p2 = bf16_rne(x - p0 - p1)     (p0 + p1 + p2 == x for normal x)
 * and the six piece products with i + j <= 2 are accumulated in the fp32 accumulators of
 * v_mfma_f32_32x32x16_bf16: one chain per output and K slice, ascending k, small terms first within
 * a k16 step; K slices are summed in slice order.  Nothing atomic: two runs are bitwise equal.  Each
 * kept product is exact in fp32; the three dropped ones are below 2.01 * 2^-24 |x||y| per term.  The
 * result is fp32-grade (its error against the fp64 product is about that of an fp32 chain), but it is
 * NOT the reference's fp32 arithmetic: results differ from BSIG_MATMUL_FP32 in the last bits.
 * Edge behaviour of the split mode:
 *   - a non-finite operand element gives non-finite outputs; NaN appears where fp32 gives inf
 *     (inf - inf occurs in the split);
 *   - |x| above the largest bf16 (about 3.39e38) rounds p0 to inf;
 *   - p2 of |x| < 2^-100 may underflow: the result then carries fewer than 24 bits of that element.
 * The mode is a permission, not a promise: a call the split kernel does not cover (a fused Adam step
 * without workspace for its slabs) runs exactly as with BSIG_MATMUL_FP32, and so do the two head products
 * of a large minibatch, where the split kernel measured slower (bsig_debug_gemm_path, out[6]; the
 * environment variable BSIG_SPLIT_BF16_EVERYWHERE=1, read per call, switches that rule off -- a diagnostic
 * for measuring what the rule rests on, tools/split_bf16_timing.py).  Below that there is no size
 * threshold.  A head product with the exp side output that would write more than 2048 partials unsplit
 * also keeps the fp32 kernels.
 */
#ifndef BSIG_MATMUL_H
#define BSIG_MATMUL_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

#define BSIG_MATMUL_FP32 0
#define BSIG_MATMUL_SPLIT_BF16 1

/* plan_flags of bsig_fit_create_ex: every product the plan issues through the per-phase GEMM
 * dispatch carries BSIG_MATMUL_SPLIT_BF16 -- forward and backward passes, weight gradients with the
 * fused Adam step, the MDRFF feature cache of bsig_fit_begin, held-out evaluations; in both graph
 * modes and under BSIG_FIT_SPLIT_ADAM.  The flag does not change which engine a plan picks: a plan
 * that a persistent update kernel covers keeps it (those kernels do their own fp32 MFMAs; combine with
 * BSIG_PLAN_NO_PERSISTENT for a plan that runs entirely in the split mode). */
#define BSIG_PLAN_SPLIT_BF16 2

/* bsig_gemm_f32 of bsig.h with the matmul precision as its last argument. */
int bsig_gemm_f32_ex(const float* a, int64_t lda, int a_kmajor, const int32_t* a_rows, const float* b,
                     int64_t ldb, int b_kmajor, const int32_t* b_rows, float* c, int64_t ldc, int64_t m,
                     int64_t n, int64_t k, int epilogue, int act, const float* bias, const float* aux,
                     int64_t ldaux, float alpha, void* workspace, size_t workspace_bytes,
                     bsig_stream_t stream, int matmul);

/* bsig_rff_project of bsig.h with the matmul precision as its last argument. */
int bsig_rff_project_ex(const float* x, int64_t ldx, const int32_t* x_rows, const float* coeff,
                        int64_t ld_coeff, const float* offset, float* feats, int64_t ld_feats,
                        int64_t batch, int64_t in_dim, int64_t m_feat, float a, int cos_only,
                        void* workspace, size_t workspace_bytes, bsig_stream_t stream, int matmul);

/* Which kernel a product would run as: host arithmetic only, no GPU.  The operands are taken as dense
 * and 16-byte aligned (A [m, k], or k-major [k, ceil16(m)]; B [n, k], or k-major [k, n]); `gathered`:
 * the rows of B's contraction come through an index vector; `epilogue`: BSIG_EPI_*, or 100 for the
 * fused Adam step of a fit's weight gradients.  Exact for the split kernel (the planner gemm_run calls);
 * the ids, tiles and slices reported for the fp32 kernels restate gemm_run's routing for such operands and
 * are APPROXIMATE: alignment, unaligned rows and the in-launch combine are not modelled.
 * out[0..7] (HOST int32):
 *   [0] kernel: 0 gemm_mfma_kernel, 1 gemm_lean_kernel, 2 / 3 the whole-width forward / gradient
 *       kernels, 4 the fp64-accumulation debug kernel, 10 gemm_split_bf16_kernel
 *   [1] [2] tile rows / columns   [3] K slices   [4] contraction elements per slice   [5] workgroups
 *   [6] BSIG_MATMUL_SPLIT_BF16 was asked for and the fp32 kernel reported runs instead -- 1: the split
 *       kernel does not cover the call; 2: the one class of shapes the mode leaves on the fp32 kernels,
 *       the two head products of a large minibatch (both operands k-contiguous, m >= 4096, k >= 1024, n a
 *       head width the whole-width kernels are built for; both k-major, k >= 4096, n >= 1024, m such a
 *       width): measured slower there (profiles/split_bf16_NOTES.md)
 *   [7] 0 */
#define BSIG_GEMM_PATH_SPLIT_BF16 10
int bsig_debug_gemm_path(int64_t m, int64_t n, int64_t k, int a_kmajor, int b_kmajor, int gathered,
                         int epilogue, size_t workspace_bytes, int matmul, int32_t* out);

#ifdef __cplusplus
}
#endif

#endif /* BSIG_MATMUL_H */
