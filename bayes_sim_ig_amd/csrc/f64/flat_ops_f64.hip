// Flat-buffer helpers of the fp64 mode (include/bsig_f64.h): Adam over the flat parameter buffer
// (torch.optim.Adam defaults, mdnn.py:203,234), column sums for the trunk bias gradients, theta
// normalisation (mdnn.py:245-248), strided row copies / gathers.
#include "f64.h"

#include <algorithm>
#include <cmath>

namespace bsig {
namespace f64 {

// torch's single-tensor Adam (torch/optim/adam.py, no amsgrad / weight decay):
//   m <- m + (g - m) * (1 - b1)        (lerp)
//   v <- v * b2 + (1 - b2) * g * g
//   p <- p - step_size * m / (sqrt(v) / sqrt(bc2) + eps)
// `dyn` (device, optional) = { ., ., step_size, sqrt(bc2) } of the engine's state block.
__global__ __launch_bounds__(256) void adam_f64_kernel(double* __restrict__ p, const double* __restrict__ g,
                                                       double* __restrict__ m, double* __restrict__ v,
                                                       int64_t n, double beta1, double beta2, double eps,
                                                       double step_size, double bc2_sqrt,
                                                       const double* __restrict__ dyn) {
  if (dyn) { step_size = dyn[2]; bc2_sqrt = dyn[3]; }
  const double omb1 = 1.0 - beta1, omb2 = 1.0 - beta2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    const double gi = g[i];
    const double mi = m[i] + (gi - m[i]) * omb1;
    const double vi = v[i] * beta2 + omb2 * gi * gi;
    p[i] = p[i] - step_size * (mi / (sqrt(vi) / bc2_sqrt + eps));
    m[i] = mi;
    v[i] = vi;
  }
}

int adam_launch(double* p, const double* g, double* m, double* v, int64_t n, double beta1, double beta2,
                double eps, double step_size, double bc2_sqrt, const double* dyn, hipStream_t st) {
  BSIG_REQUIRE(p && g && m && v && n >= 0, "adam_f64: bad args");
  if (n == 0) return BSIG_OK;
  const int blocks = (int)std::min<int64_t>(ceil_div<int64_t>(n, 256), 2048);
  hipLaunchKernelGGL(adam_f64_kernel, dim3(blocks), dim3(256), 0, st, p, g, m, v, n, beta1, beta2, eps,
                     step_size, bc2_sqrt, dyn);
  BSIG_CHECK_LAUNCH("adam_f64");
  return BSIG_OK;
}

// out[j] = sum_i x[i*ld + j]; block = 64 columns x 4 row lanes over all rows, fixed order
__global__ __launch_bounds__(256) void colsum_f64_kernel(const double* __restrict__ x, int64_t ld, int64_t rows,
                                                         int64_t cols, double* __restrict__ out) {
  __shared__ double part[4][64];
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int64_t j = (int64_t)blockIdx.x * 64 + cl;
  double acc = 0.0;
  if (j < cols)
    for (int64_t i = rl; i < rows; i += 4) acc += x[i * ld + j];
  part[rl][cl] = acc;
  __syncthreads();
  if (rl == 0 && j < cols) out[j] = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
}

int colsum_launch(const double* x, int64_t ld, int64_t rows, int64_t cols, double* out, hipStream_t st) {
  BSIG_REQUIRE(x && out && rows >= 0 && cols >= 1 && ld >= cols, "colsum_f64: bad args");
  hipLaunchKernelGGL(colsum_f64_kernel, dim3((unsigned)ceil_div<int64_t>(cols, 64)), dim3(256), 0, st, x, ld,
                     rows, cols, out);
  BSIG_CHECK_LAUNCH("colsum_f64");
  return BSIG_OK;
}

__global__ __launch_bounds__(256) void normalize_rows_f64_kernel(
    const double* __restrict__ theta, int64_t ld_in, const double* __restrict__ lows,
    const double* __restrict__ highs, double* __restrict__ out, int64_t ld_out, int64_t rows, int64_t cols) {
  for (int64_t r = blockIdx.x; r < rows; r += gridDim.x)
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x)
      out[r * ld_out + c] = (theta[r * ld_in + c] - lows[c]) / (highs[c] - lows[c]);
}

__global__ __launch_bounds__(256) void copy_rows_f64_kernel(const double* __restrict__ src, int64_t ld_src,
                                                            const int32_t* __restrict__ rows,
                                                            double* __restrict__ dst, int64_t ld_dst,
                                                            int64_t n_rows, int64_t cols) {
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const double* s = src + (rows ? (int64_t)rows[r] : r) * ld_src;
    double* d = dst + r * ld_dst;
    for (int64_t c = threadIdx.x; c < cols; c += blockDim.x) d[c] = s[c];
  }
}

}  // namespace f64
}  // namespace bsig

using namespace bsig;

extern "C" int bsig_adam_flat_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq,
                                  int64_t n, double lr, double beta1, double beta2, double eps, int64_t t,
                                  bsig_stream_t stream) {
  BSIG_REQUIRE(t >= 1, "adam_f64: step number is 1-based");
  double b1t = 1.0, b2t = 1.0;   // running products, as the fit loop forms them on the device
  if (t <= (1 << 20)) {
    for (int64_t i = 0; i < t; ++i) { b1t *= beta1; b2t *= beta2; }
  } else {
    b1t = std::pow(beta1, (double)t); b2t = std::pow(beta2, (double)t);
  }
  return f64::adam_launch(params, grads, exp_avg, exp_avg_sq, n, beta1, beta2, eps, lr / (1.0 - b1t),
                          std::sqrt(1.0 - b2t), nullptr, as_stream(stream));
}

extern "C" int bsig_normalize_rows_f64(const double* theta, int64_t ld_in, const double* lows,
                                       const double* highs, double* out, int64_t ld_out, int64_t rows,
                                       int64_t cols, bsig_stream_t stream) {
  BSIG_REQUIRE(theta && lows && highs && out && rows >= 0 && cols >= 1, "normalize_f64: bad args");
  if (rows == 0) return BSIG_OK;
  hipLaunchKernelGGL(f64::normalize_rows_f64_kernel, dim3((int)std::min<int64_t>(rows, 4096)),
                     dim3(cols >= 192 ? 256 : 64), 0, as_stream(stream), theta, ld_in, lows, highs, out,
                     ld_out, rows, cols);
  BSIG_CHECK_LAUNCH("normalize_rows_f64");
  return BSIG_OK;
}

extern "C" int bsig_copy_rows_f64(const double* src, int64_t ld_src, const int32_t* rows, double* dst,
                                  int64_t ld_dst, int64_t n_rows, int64_t cols, bsig_stream_t stream) {
  BSIG_REQUIRE(src && dst && n_rows >= 0 && cols >= 0, "copy_rows_f64: bad args");
  if (n_rows == 0 || cols == 0) return BSIG_OK;
  hipLaunchKernelGGL(f64::copy_rows_f64_kernel, dim3((int)std::min<int64_t>(n_rows, 8192)),
                     dim3(cols >= 192 ? 256 : 64), 0, as_stream(stream), src, ld_src, rows, dst, ld_dst,
                     n_rows, cols);
  BSIG_CHECK_LAUNCH("copy_rows_f64");
  return BSIG_OK;
}
