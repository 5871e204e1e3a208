// Internal launchers of the flat-buffer kernels (flat_ops.hip).
#pragma once
#include "common.h"

namespace bsig {

int adam_launch(float* p, const float* g, float* m, float* v, int64_t n, float lr,
                float beta1, float beta2, float eps, int64_t t, const float* dyn,
                hipStream_t st);
int colsum_launch(const float* x, int64_t ld, int64_t rows, int64_t cols, float* out,
                  void* workspace, size_t workspace_bytes, hipStream_t st);

}  // namespace bsig
