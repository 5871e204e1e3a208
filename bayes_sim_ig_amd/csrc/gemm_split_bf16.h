// The split-bf16 GEMM (BSIG_MATMUL_SPLIT_BF16, include/bsig_matmul.h): the fp32 products of gemm_run on
// the bf16 matrix pipes, each fp32 operand element split into three bf16 pieces.  See
// gemm_split_bf16.hip for the arithmetic and the kernel.
#pragma once
#include "gemm.h"

namespace bsig {

// kernel ids of bsig_debug_gemm_path
enum { GEMM_PATH_MFMA = 0, GEMM_PATH_LEAN = 1, GEMM_PATH_WIDE_FORWARD = 2, GEMM_PATH_WIDE_GRADIENT = 3,
       GEMM_PATH_F64ACC = 4, GEMM_PATH_SPLIT_BF16 = 10 };

struct SplitBf16Plan {
  int tile = 0;        // 64 or 128: square tiles of 2 x 2 wavefronts
  int splits = 1;      // K slices
  int k_chunk = 0;     // contraction elements per slice (a multiple of 32)
  int slabs = 0;       // the kernel stores raw slabs and gemm_reduce_kernel applies the epilogue
  int64_t workgroups = 0;
};

// Does the split-bf16 kernel cover this product with this workspace?  Every operand form is covered;
// what can be missing is room for the slabs: a fused Adam step (EPI_ADAM) always goes through slabs
// and the reduce + Adam kernel (>= 1 slab; >= 2 where the bias gradients arrive as partial sums).
bool split_bf16_plan(int64_t m, int64_t n, int64_t k, int epilogue, bool partial_bias, size_t ws_bytes,
                     SplitBf16Plan* pl);

// p.splits / p.k_chunk / p.partial set from the plan
int launch_split_bf16(const GemmParams& p, const SplitBf16Plan& pl, hipStream_t st);

}  // namespace bsig
