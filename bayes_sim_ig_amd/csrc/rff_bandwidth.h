// include/bsig_rff_bandwidth.h: the kernels and their launchers (csrc/rff_bandwidth.hip instantiates them for fp32
// and double rows).  Pair distances = one workgroup per upper-triangular 64 x 64 tile of row pairs, the row blocks
// staged in LDS as doubles, one fma chain per pair over ascending k; selection = an 8-pass radix select over the
// bit patterns, per-workgroup LDS histograms merged with integer atomic adds, every workgroup of a pass deriving
// the prefix decided so far from the finished histograms; then one thread writes sigma.  Everything a thread
// reads lies in rows [0, m) and columns [0, width) of x; everything it writes lies in the caller's workspace.
#pragma once
#include "common.h"
#include "../../include/bsig_rff_bandwidth.h"

#include <algorithm>
#include <cmath>

namespace bsig {
namespace rffbw {

constexpr int kMaxRows = BSIG_RFF_BANDWIDTH_MAX_ROWS;
constexpr int kThreads = 256;
constexpr int kTile = 64;            // rows on either side of a tile of pairs
constexpr int kSub = 4;              // a thread owns kSub x kSub pairs, 16 rows apart
constexpr int kChunk = 32;           // columns staged per step
constexpr int kPitch = kTile + 1;    // doubles between two staged columns (odd: the transposing writes spread over banks)
constexpr int kPasses = 8, kBins = 256;       // 8 bits per pass, from the top
constexpr int kFlagWords = 64;
constexpr int kSelectWords = kPasses * kBins + kFlagWords;     // [histograms | flags]
static_assert(kSelectWords * 4 == BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES, "header and kernels disagree");
static_assert(kThreads == kBins && kThreads == (kTile / kSub) * (kTile / kSub), "one thread per bin and per 4 x 4 pairs");
constexpr uint64_t kExpMask = 0x7FF0000000000000ull, kAbsMask = 0x7FFFFFFFFFFFFFFFull, kNaNBits = 0x7FF8000000000000ull;

template <typename T> struct Vec;
template <> struct Vec<float> { using type = float4; static constexpr int n = 4; };
template <> struct Vec<double> { using type = double2; static constexpr int n = 2; };

// s[k][r] <- (double) x[row0 + r, k0 + k] for r < kTile, k < kChunk; zero where the row is >= m or the column
// >= width (a zero pair of elements leaves a chain as it is: fma(0, 0, acc) == acc).  VEC: 16-byte loads of the
// column groups that lie inside the width (x and the pitch are 16-byte aligned, k0 is a multiple of kChunk).
template <typename T, bool VEC>
__device__ inline void stage(const T* __restrict__ x, int64_t ld, int64_t row0, int64_t m, int64_t k0,
                             int64_t width, double* s) {
  constexpr int V = VEC ? Vec<T>::n : 1;
  constexpr int groups = kChunk / V;
  for (int e = threadIdx.x; e < kTile * groups; e += kThreads) {
    const int r = e / groups, g = e % groups;
    const int64_t row = row0 + r, k = k0 + (int64_t)g * V;
    T q[V];
#pragma unroll
    for (int c = 0; c < V; ++c) q[c] = T(0);
    if (row < m) {
      const T* p = x + row * ld + k;
      bool whole = false;
      if constexpr (VEC) {
        if (k + V <= width) {
          const typename Vec<T>::type v = *reinterpret_cast<const typename Vec<T>::type*>(p);
          const T* el = reinterpret_cast<const T*>(&v);
#pragma unroll
          for (int c = 0; c < V; ++c) q[c] = el[c];
          whole = true;
        }
      }
      if (!whole) {
#pragma unroll
        for (int c = 0; c < V; ++c)
          if (k + c < width) q[c] = p[c];
      }
    }
#pragma unroll
    for (int c = 0; c < V; ++c) s[(g * V + c) * kPitch + r] = (double)q[c];
  }
}

// Block b: the b-th tile (ti <= tj) of the upper triangle, rows of ti against rows of tj.  d2: the P squared
// distances, pair (i < j) at i (2 m - i - 1) / 2 + (j - i - 1).
template <typename T, bool VEC>
__global__ __launch_bounds__(kThreads) void pair_d2_kernel(const T* __restrict__ x, int64_t ld, int64_t m,
                                                           int64_t width, int tiles_per_side,
                                                           double* __restrict__ d2) {
  __shared__ double sa[kChunk * kPitch], sb[kChunk * kPitch];
  int t = (int)blockIdx.x, ti = 0;
  for (int len = tiles_per_side; t >= len; t -= len, --len) ++ti;
  const int tj = ti + t;
  const int ty = threadIdx.x / (kTile / kSub), tx = threadIdx.x % (kTile / kSub);
  double acc[kSub][kSub];
#pragma unroll
  for (int a = 0; a < kSub; ++a)
#pragma unroll
    for (int b = 0; b < kSub; ++b) acc[a][b] = 0.0;
  for (int64_t k0 = 0; k0 < width; k0 += kChunk) {
    stage<T, VEC>(x, ld, (int64_t)ti * kTile, m, k0, width, sa);
    stage<T, VEC>(x, ld, (int64_t)tj * kTile, m, k0, width, sb);
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < kChunk; ++k) {
      double va[kSub], vb[kSub];
#pragma unroll
      for (int a = 0; a < kSub; ++a) va[a] = sa[k * kPitch + ty + a * (kTile / kSub)];
#pragma unroll
      for (int b = 0; b < kSub; ++b) vb[b] = sb[k * kPitch + tx + b * (kTile / kSub)];
#pragma unroll
      for (int a = 0; a < kSub; ++a)
#pragma unroll
        for (int b = 0; b < kSub; ++b) {
          const double diff = va[a] - vb[b];
          acc[a][b] = fma(diff, diff, acc[a][b]);
        }
    }
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < kSub; ++a)
#pragma unroll
    for (int b = 0; b < kSub; ++b) {
      const int64_t i = (int64_t)ti * kTile + ty + a * (kTile / kSub);
      const int64_t j = (int64_t)tj * kTile + tx + b * (kTile / kSub);
      if (i < j && j < m) d2[i * (2 * m - i - 1) / 2 + (j - i - 1)] = acc[a][b];
    }
}

// The prefix (the top 8 * passes bits of the median, right-aligned) and the rank that remains among the values
// sharing it, from the finished histograms of passes 0 .. passes - 1.  All kThreads threads call it and get the
// same answer; sh: 8 words of LDS.
__device__ inline void decide(const uint32_t* hist, int passes, uint32_t rank0, uint32_t* sh, uint64_t& prefix,
                              uint32_t& rank) {
  const int t = threadIdx.x, lane = t & (kWave - 1), w = t / kWave;
  prefix = 0;
  rank = rank0;
  for (int q = 0; q < passes; ++q) {
    const uint32_t v = hist[q * kBins + t];
    uint32_t incl = v;
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
      const uint32_t below = __shfl_up(incl, off, kWave);
      if (lane >= off) incl += below;
    }
    __syncthreads();
    if (lane == kWave - 1) sh[w] = incl;
    __syncthreads();
    uint32_t excl = incl - v;
    for (int i = 0; i < w; ++i) excl += sh[i];
    if (v > 0 && rank >= excl && rank - excl < v) {      // exactly one bin holds the rank
      sh[4] = (uint32_t)t;
      sh[5] = rank - excl;
    }
    __syncthreads();
    prefix = (prefix << 8) | sh[4];
    rank = sh[5];
  }
}

__global__ __launch_bounds__(kThreads) void select_zero_kernel(uint32_t* words) {
  for (int i = threadIdx.x; i < kSelectWords; i += kThreads) words[i] = 0u;
}

// Pass `pass`: the digit counts of the values whose higher bits are the prefix decided so far, added to
// hist[pass].  Pass 0 also raises flags[0] when a value is non-finite.
__global__ __launch_bounds__(kThreads) void select_pass_kernel(const uint64_t* __restrict__ bits, int64_t count,
                                                               int pass, uint32_t* hist, uint32_t* flags) {
  __shared__ uint32_t sh[8];
  __shared__ uint32_t bins[kBins];
  uint64_t prefix;
  uint32_t rank;
  decide(hist, pass, (uint32_t)((count - 1) / 2), sh, prefix, rank);
  bins[threadIdx.x] = 0u;
  __syncthreads();
  const int shift = 56 - 8 * pass;
  bool bad = false;
  for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < count; i += (int64_t)gridDim.x * kThreads) {
    const uint64_t b = bits[i];
    if (pass == 0) {
      bad = bad || (b & kAbsMask) >= kExpMask;
      atomicAdd(&bins[b >> 56], 1u);
    } else if ((b >> (shift + 8)) == prefix) {
      atomicAdd(&bins[(b >> shift) & (kBins - 1)], 1u);
    }
  }
  if (bad) atomicOr(&flags[0], 1u);
  __syncthreads();
  const uint32_t mine = bins[threadIdx.x];
  if (mine) atomicAdd(&hist[pass * kBins + threadIdx.x], mine);
}

// One workgroup: the selected value from all kPasses histograms; as_sigma: scale * sqrt(value), 1.0 for zero.
__global__ __launch_bounds__(kThreads) void select_finish_kernel(const uint32_t* hist, const uint32_t* flags,
                                                                 int64_t count, int as_sigma, double scale,
                                                                 double* __restrict__ out) {
  __shared__ uint32_t sh[8];
  uint64_t value_bits;
  uint32_t rank;
  decide(hist, kPasses, (uint32_t)((count - 1) / 2), sh, value_bits, rank);
  if (threadIdx.x != 0) return;
  const double v = __longlong_as_double((long long)value_bits);
  double r = v;
  if (flags[0] != 0u)
    r = __longlong_as_double((long long)kNaNBits);
  else if (as_sigma)
    r = v == 0.0 ? 1.0 : scale * __dsqrt_rn(v);
  *out = r;
}

template <typename C>
__global__ __launch_bounds__(kThreads) void coeff_dev_kernel(const float* __restrict__ freqs,
                                                             const double* __restrict__ sigma,
                                                             C* __restrict__ coeff, int64_t m, int64_t d, int64_t ld) {
  const double s = *sigma;
  const int64_t total = m * ld;
  for (int64_t e = (int64_t)blockIdx.x * kThreads + threadIdx.x; e < total; e += (int64_t)gridDim.x * kThreads) {
    const int64_t r = e / ld, c = e % ld;
    coeff[e] = c < d ? (C)((double)freqs[r * d + c] / s) : C(0);
  }
}

inline int64_t pairs_of(int64_t n) {
  const int64_t m = std::min<int64_t>(n, kMaxRows);
  return m * (m - 1) / 2;
}

inline int64_t workspace_bytes(int64_t n, int64_t width) {
  if (n < 2 || width < 1) return -1;
  return pairs_of(n) * (int64_t)sizeof(double) + BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES;
}

// values[count] -> *out, on `words` (kSelectWords, zeroed here).  The arguments are checked by the callers.
inline int select_launch(const char* who, const double* values, int64_t count, int as_sigma, double scale,
                         double* out, uint32_t* words, hipStream_t st) {
  uint32_t* hist = words;
  uint32_t* flags = words + kPasses * kBins;
  const unsigned blocks = (unsigned)std::max<int64_t>(1, std::min<int64_t>(ceil_div<int64_t>(count, kThreads * 4), 512));
  hipLaunchKernelGGL(select_zero_kernel, dim3(1), dim3(kThreads), 0, st, words);
  BSIG_CHECK_LAUNCH(who);
  for (int pass = 0; pass < kPasses; ++pass) {
    hipLaunchKernelGGL(select_pass_kernel, dim3(blocks), dim3(kThreads), 0, st,
                       reinterpret_cast<const uint64_t*>(values), count, pass, hist, flags);
    BSIG_CHECK_LAUNCH(who);
  }
  hipLaunchKernelGGL(select_finish_kernel, dim3(1), dim3(kThreads), 0, st, hist, flags, count, as_sigma, scale, out);
  BSIG_CHECK_LAUNCH(who);
  return BSIG_OK;
}

inline int select_run(const char* who, const double* values, int64_t count, double* out, void* workspace,
                      size_t ws_bytes, hipStream_t st) {
  BSIG_REQUIRE(count >= 1 && count <= INT32_MAX, "%s: count = %lld (1 .. 2^31 - 1)", who, (long long)count);
  BSIG_REQUIRE(values, "%s: null pointer values", who);
  BSIG_REQUIRE(out, "%s: null pointer out", who);
  BSIG_REQUIRE(workspace, "%s: null pointer workspace", who);
  BSIG_REQUIRE(ws_bytes >= (size_t)BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES,
               "%s: workspace_bytes %zu below the %d needed", who, ws_bytes, BSIG_RFF_BANDWIDTH_SELECT_WORKSPACE_BYTES);
  BSIG_REQUIRE(aligned(workspace, 8), "%s: workspace is not 8-byte aligned", who);
  return select_launch(who, values, count, 0, 1.0, out, static_cast<uint32_t*>(workspace), st);
}

template <typename T>
int median_run(const char* who, const T* x, int64_t ld, int64_t n, int64_t width, double scale, double* sigma_out,
               void* workspace, size_t ws_bytes, hipStream_t st) {
  BSIG_REQUIRE(n >= 2, "%s: n = %lld: a pairwise distance needs two rows", who, (long long)n);
  BSIG_REQUIRE(width >= 1, "%s: width = %lld", who, (long long)width);
  BSIG_REQUIRE(x, "%s: null pointer x", who);
  BSIG_REQUIRE(sigma_out, "%s: null pointer sigma_out", who);
  BSIG_REQUIRE(workspace, "%s: null pointer workspace", who);
  BSIG_REQUIRE(ld >= width, "%s: ld %lld below the width %lld", who, (long long)ld, (long long)width);
  BSIG_REQUIRE(std::isfinite(scale) && scale > 0.0, "%s: scale = %g is not a positive finite number", who, scale);
  const int64_t need = workspace_bytes(n, width);
  BSIG_REQUIRE(ws_bytes >= (size_t)need, "%s: workspace_bytes %zu below the %lld needed", who, ws_bytes,
               (long long)need);
  BSIG_REQUIRE(aligned(workspace, 8), "%s: workspace is not 8-byte aligned", who);
  const int64_t m = std::min<int64_t>(n, kMaxRows), pairs = pairs_of(n);
  BSIG_REQUIRE(m - 1 <= (INT64_MAX / 16 - width) / ld, "%s: ld %lld is too large", who, (long long)ld);
  double* d2 = static_cast<double*>(workspace);
  const int side = (int)ceil_div<int64_t>(m, kTile);
  const unsigned tiles = (unsigned)(side * (side + 1) / 2);
  if (aligned(x, 16) && (ld * (int64_t)sizeof(T)) % 16 == 0)
    hipLaunchKernelGGL((pair_d2_kernel<T, true>), dim3(tiles), dim3(kThreads), 0, st, x, ld, m, width, side, d2);
  else
    hipLaunchKernelGGL((pair_d2_kernel<T, false>), dim3(tiles), dim3(kThreads), 0, st, x, ld, m, width, side, d2);
  BSIG_CHECK_LAUNCH(who);
  return select_launch(who, d2, pairs, 1, scale, sigma_out, reinterpret_cast<uint32_t*>(d2 + pairs), st);
}

template <typename C>
int coeff_run(const char* who, const float* freqs, const double* sigma_dev, C* coeff, int64_t m, int64_t d,
              int64_t ld, hipStream_t st) {
  BSIG_REQUIRE(m >= 0, "%s: m = %lld", who, (long long)m);
  BSIG_REQUIRE(d >= 1, "%s: d = %lld", who, (long long)d);
  BSIG_REQUIRE(ld >= d, "%s: ld %lld below d %lld", who, (long long)ld, (long long)d);
  if (m == 0) return BSIG_OK;
  BSIG_REQUIRE(freqs, "%s: null pointer freqs", who);
  BSIG_REQUIRE(sigma_dev, "%s: null pointer sigma_dev", who);
  BSIG_REQUIRE(coeff, "%s: null pointer coeff", who);
  BSIG_REQUIRE(m <= (INT64_MAX / 16) / ld, "%s: m %lld x ld %lld is too large", who, (long long)m, (long long)ld);
  const unsigned blocks = (unsigned)std::min<int64_t>(ceil_div<int64_t>(m * ld, kThreads), 4096);
  hipLaunchKernelGGL(coeff_dev_kernel<C>, dim3(blocks), dim3(kThreads), 0, st, freqs, sigma_dev, coeff, m, d, ld);
  BSIG_CHECK_LAUNCH(who);
  return BSIG_OK;
}

}  // namespace rffbw
}  // namespace bsig
