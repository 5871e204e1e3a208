// include/bsig_input_norm.h: the kernels and their launchers, templated on the rows' type (float: csrc/input_norm.hip,
// double: csrc/f64/input_norm_f64.hip).  Statistics = a slab pass (Welford in double, one thread per column or per
// 16 bytes of columns) + a finishing pass (Chan's merge in ascending slab order, the flat rule); apply = one thread
// per column group striding over rows with its columns' mean / inv_std in registers.  Everything a thread touches
// lies in [0, width) of a row: the padding of a pitched row is neither read nor written.
#pragma once
#include "common.h"
#include "../../include/bsig_input_norm.h"

#include <algorithm>

namespace bsig {
namespace inorm {

constexpr int kSlabRows = BSIG_INPUT_NORM_SLAB_ROWS;
constexpr int kThreads = 256;     // columns groups per block
constexpr int kRowsInFlight = 4;  // rows a thread loads before it uses them

__host__ __device__ inline int64_t min64(int64_t a, int64_t b) { return a < b ? a : b; }

template <typename T> struct Row;
template <> struct Row<float> { using Vec = float4; static constexpr int kVec = 4; static constexpr double kU = 1.1920928955078125e-07; };
template <> struct Row<double> { using Vec = double2; static constexpr int kVec = 2; static constexpr double kU = 2.220446049250313e-16; };

// V elements of a row at p, of which the first nc exist (nc == V: one 16-byte access when V > 1)
template <typename T, int V>
__device__ inline void load_cols(const T* p, int nc, T (&q)[V]) {
  if constexpr (V > 1) {
    if (nc == V) {
      const typename Row<T>::Vec v = *reinterpret_cast<const typename Row<T>::Vec*>(p);
      const T* e = reinterpret_cast<const T*>(&v);
#pragma unroll
      for (int c = 0; c < V; ++c) q[c] = e[c];
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < V; ++c) q[c] = c < nc ? p[c] : T(0);
}

template <typename T, int V>
__device__ inline void store_cols(T* p, int nc, const T (&q)[V]) {
  if constexpr (V > 1) {
    if (nc == V) {
      typename Row<T>::Vec v;
      T* e = reinterpret_cast<T*>(&v);
#pragma unroll
      for (int c = 0; c < V; ++c) e[c] = q[c];
      *reinterpret_cast<typename Row<T>::Vec*>(p) = v;
      return;
    }
  }
#pragma unroll
  for (int c = 0; c < V; ++c)
    if (c < nc) p[c] = q[c];
}

// Pass 1.  Block b: column tile b % col_tiles, slab b / col_tiles.  part_mean / part_m2: [n_slabs, width].
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void stats_slab_kernel(const T* __restrict__ x, int64_t ld, int64_t n,
                                                              int64_t width, int64_t col_tiles,
                                                              double* __restrict__ part_mean,
                                                              double* __restrict__ part_m2) {
  const int64_t tile = (int64_t)blockIdx.x % col_tiles, slab = (int64_t)blockIdx.x / col_tiles;
  const int64_t col0 = (tile * kThreads + threadIdx.x) * V;
  if (col0 >= width) return;
  const int nc = (int)min64(V, width - col0);
  const int64_t row0 = slab * kSlabRows;
  const int rows = (int)min64(kSlabRows, n - row0);
  const T* p = x + row0 * ld + col0;
  double mean[V], m2[V];
#pragma unroll
  for (int c = 0; c < V; ++c) mean[c] = m2[c] = 0.0;
  for (int i = 0; i < rows; i += kRowsInFlight) {
    T q[kRowsInFlight][V];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u)
      if (i + u < rows) load_cols<T, V>(p + (int64_t)(i + u) * ld, nc, q[u]);
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      if (i + u < rows) {
        const double inv_k = 1.0 / (double)(i + u + 1);
#pragma unroll
        for (int c = 0; c < V; ++c) {
          const double xv = (double)q[u][c];
          const double delta = xv - mean[c];
          mean[c] += delta * inv_k;
          m2[c] += delta * (xv - mean[c]);
        }
      }
    }
  }
  double* pm = part_mean + slab * width + col0;
  double* p2 = part_m2 + slab * width + col0;
#pragma unroll
  for (int c = 0; c < V; ++c)
    if (c < nc) { pm[c] = mean[c]; p2[c] = m2[c]; }
}

// Pass 2.  One thread per column: the slabs in ascending order, then the flat rule (flat_tol = 8 u of the rows' type T).
template <typename T>
__global__ __launch_bounds__(64) void stats_finish_kernel(const double* __restrict__ part_mean,
                                                          const double* __restrict__ part_m2, int64_t n,
                                                          int64_t width, int64_t n_slabs, double flat_tol,
                                                          double* __restrict__ mean_out,
                                                          double* __restrict__ inv_std_out) {
  const int64_t j = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (j >= width) return;
  double mean = part_mean[j], m2 = part_m2[j];
  double na = (double)min64(kSlabRows, n);
  for (int64_t s = 1; s < n_slabs; s += kRowsInFlight) {
    double mb[kRowsInFlight], qb[kRowsInFlight];
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u)
      if (s + u < n_slabs) { mb[u] = part_mean[(s + u) * width + j]; qb[u] = part_m2[(s + u) * width + j]; }
#pragma unroll
    for (int u = 0; u < kRowsInFlight; ++u) {
      if (s + u < n_slabs) {
        const double nb = (double)min64(kSlabRows, n - (s + u) * kSlabRows);
        const double nab = na + nb;
        const double delta = mb[u] - mean;
        mean = mean + delta * (nb / nab);
        m2 = (m2 + qb[u]) + (delta * delta) * (na * nb / nab);
        na = nab;
      }
    }
  }
  const double sd = sqrt(m2 / (double)n);
  const bool flat = sd <= flat_tol * fabs(mean);      // (a NaN compares false: it propagates below)
  mean_out[j] = mean;
  inv_std_out[j] = flat ? 0.0 : 1.0 / sd;
}

// The rows lane, lane + row_lanes, ... of one thread's columns.  FULL: all V columns exist (16-byte accesses
// when V > 1).  The rows go in groups of kRowsInFlight; the loads of the next group are issued BEFORE the current
// group is converted and stored, and the loop over whole groups has no branch in it, so the compiler can wait for
// the current group alone (s_waitcnt vmcnt(kRowsInFlight)) while the next one is in flight: the conversions (two
// fp64 operations and two conversions per element) then do not empty the memory pipeline.  Without that the
// kernel ran 18 % behind copy_rows at 32 000 x 11 110 (profiles/input_norm_NOTES.md).
template <typename T, int V, bool FULL>
__device__ inline void apply_rows(const T* x, int64_t ld_x, const double (&mu)[V], const double (&is)[V], T* out,
                                  int64_t ld_out, int64_t n, int64_t lane, int64_t row_lanes, int nc) {
  constexpr int R = kRowsInFlight;
  const int64_t group = R * row_lanes;                       // rows between a thread's groups
  const int64_t last = n - 1 - lane - (R - 1) * row_lanes;   // >= 0: the first group has all its R rows
  const int64_t whole = last >= 0 ? last / group + 1 : 0;    // groups with all R rows
  auto load = [&](T (&q)[R][V], int64_t r) {
#pragma unroll
    for (int u = 0; u < R; ++u) load_cols<T, V>(x + (r + u * row_lanes) * ld_x, FULL ? V : nc, q[u]);
  };
  auto emit = [&](T (&q)[R][V], int64_t r) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
#pragma unroll
      for (int c = 0; c < V; ++c) q[u][c] = (T)(((double)q[u][c] - mu[c]) * is[c]);
      store_cols<T, V>(out + (r + u * row_lanes) * ld_out, FULL ? V : nc, q[u]);
    }
  };
  T cur[R][V], nxt[R][V];
  int64_t r = lane;
  if (whole > 0) {
    load(cur, r);
    for (int64_t g = 1; g < whole; ++g, r += group) {
      load(nxt, r + group);
      emit(cur, r);
#pragma unroll
      for (int u = 0; u < R; ++u)
#pragma unroll
        for (int c = 0; c < V; ++c) cur[u][c] = nxt[u][c];
    }
    emit(cur, r);
    r += group;
  }
  for (; r < n; r += row_lanes) {      // the rows of the last, partial group
    T q[V];
    load_cols<T, V>(x + r * ld_x, FULL ? V : nc, q);
#pragma unroll
    for (int c = 0; c < V; ++c) q[c] = (T)(((double)q[c] - mu[c]) * is[c]);
    store_cols<T, V>(out + r * ld_out, FULL ? V : nc, q);
  }
}

// out = (x - mean) * inv_std.  Block b: column tile b % col_tiles, row lane b / col_tiles of row_lanes.
// x and out may be the same rows (in place): an element is read and written by the same thread, read first.
template <typename T, int V>
__global__ __launch_bounds__(kThreads) void apply_kernel(const T* x, int64_t ld_x, const double* __restrict__ mean,
                                                         const double* __restrict__ inv_std, T* out,
                                                         int64_t ld_out, int64_t n, int64_t width,
                                                         int64_t col_tiles, int64_t row_lanes) {
  const int64_t tile = (int64_t)blockIdx.x % col_tiles, lane = (int64_t)blockIdx.x / col_tiles;
  const int64_t col0 = (tile * kThreads + threadIdx.x) * V;
  if (col0 >= width) return;
  const int nc = (int)min64(V, width - col0);
  double mu[V], is[V];
#pragma unroll
  for (int c = 0; c < V; ++c) {
    mu[c] = c < nc ? mean[col0 + c] : 0.0;
    is[c] = c < nc ? inv_std[col0 + c] : 0.0;
  }
  if (nc == V)
    apply_rows<T, V, true>(x + col0, ld_x, mu, is, out + col0, ld_out, n, lane, row_lanes, nc);
  else
    apply_rows<T, V, false>(x + col0, ld_x, mu, is, out + col0, ld_out, n, lane, row_lanes, nc);
}

inline int64_t workspace_bytes(int64_t n, int64_t width) {
  if (n <= 0 || width <= 0) return -1;
  const int64_t n_slabs = ceil_div<int64_t>(n, kSlabRows);
  if (n_slabs > (INT64_MAX / 16) / width) return -1;
  return 2 * n_slabs * width * (int64_t)sizeof(double);
}

template <typename T>
inline bool vec_ok(const T* p, int64_t ld) {
  return aligned(p, 16) && (ld * (int64_t)sizeof(T)) % 16 == 0;
}

template <typename T>
int stats_run(const char* who, const T* x, int64_t ld, int64_t n, int64_t width, double* mean, double* inv_std,
              void* workspace, size_t ws_bytes, hipStream_t st) {
  BSIG_REQUIRE(n >= 1, "%s: n = %lld: the statistics of no rows do not exist", who, (long long)n);
  BSIG_REQUIRE(width >= 1, "%s: width = %lld", who, (long long)width);
  BSIG_REQUIRE(x, "%s: null pointer x", who);
  BSIG_REQUIRE(mean, "%s: null pointer mean", who);
  BSIG_REQUIRE(inv_std, "%s: null pointer inv_std", who);
  BSIG_REQUIRE(workspace, "%s: null pointer workspace", who);
  BSIG_REQUIRE(ld >= width, "%s: ld %lld below the width %lld", who, (long long)ld, (long long)width);
  const int64_t need = workspace_bytes(n, width);
  BSIG_REQUIRE(need > 0, "%s: n %lld x width %lld is too large", who, (long long)n, (long long)width);
  BSIG_REQUIRE(ws_bytes >= (size_t)need, "%s: workspace_bytes %zu below the %lld needed", who, ws_bytes,
               (long long)need);
  BSIG_REQUIRE(aligned(workspace, 8), "%s: workspace is not 8-byte aligned", who);
  const int64_t n_slabs = ceil_div<int64_t>(n, kSlabRows);
  double* part_mean = static_cast<double*>(workspace);
  double* part_m2 = part_mean + n_slabs * width;
  constexpr int V = Row<T>::kVec;
  const bool vec = vec_ok(x, ld) && width >= V;
  const int64_t col_tiles = ceil_div<int64_t>(width, (int64_t)kThreads * (vec ? V : 1));
  const int64_t blocks = col_tiles * n_slabs;
  BSIG_REQUIRE(blocks <= INT32_MAX, "%s: n %lld x width %lld needs too many workgroups", who, (long long)n,
               (long long)width);
  if (vec)
    hipLaunchKernelGGL((stats_slab_kernel<T, V>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, ld, n, width,
                       col_tiles, part_mean, part_m2);
  else
    hipLaunchKernelGGL((stats_slab_kernel<T, 1>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, ld, n, width,
                       col_tiles, part_mean, part_m2);
  BSIG_CHECK_LAUNCH(who);
  hipLaunchKernelGGL(stats_finish_kernel<T>, dim3((unsigned)ceil_div<int64_t>(width, 64)), dim3(64), 0, st, part_mean,
                     part_m2, n, width, n_slabs, 8.0 * Row<T>::kU, mean, inv_std);
  BSIG_CHECK_LAUNCH(who);
  return BSIG_OK;
}

template <typename T>
int apply_run(const char* who, const T* x, int64_t ld_x, const double* mean, const double* inv_std, T* out,
              int64_t ld_out, int64_t n, int64_t width, hipStream_t st) {
  BSIG_REQUIRE(n >= 0, "%s: n = %lld", who, (long long)n);
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(width >= 1, "%s: width = %lld", who, (long long)width);
  BSIG_REQUIRE(x, "%s: null pointer x", who);
  BSIG_REQUIRE(mean, "%s: null pointer mean", who);
  BSIG_REQUIRE(inv_std, "%s: null pointer inv_std", who);
  BSIG_REQUIRE(out, "%s: null pointer out", who);
  BSIG_REQUIRE(ld_x >= width, "%s: ld_x %lld below the width %lld", who, (long long)ld_x, (long long)width);
  BSIG_REQUIRE(ld_out >= width, "%s: ld_out %lld below the width %lld", who, (long long)ld_out, (long long)width);
  BSIG_REQUIRE(n - 1 <= (INT64_MAX / 16 - width) / std::max(ld_x, ld_out), "%s: n %lld rows are too many", who,
               (long long)n);
  if (!(static_cast<const T*>(out) == x && ld_out == ld_x)) {
    const uintptr_t x0 = reinterpret_cast<uintptr_t>(x), o0 = reinterpret_cast<uintptr_t>(out);
    const uintptr_t x1 = x0 + (uintptr_t)((n - 1) * ld_x + width) * sizeof(T);
    const uintptr_t o1 = o0 + (uintptr_t)((n - 1) * ld_out + width) * sizeof(T);
    BSIG_REQUIRE(x1 <= o0 || o1 <= x0, "%s: out overlaps x (in place needs out == x and ld_out == ld_x)", who);
  }
  constexpr int V = Row<T>::kVec;
  const bool vec = vec_ok(x, ld_x) && vec_ok(out, ld_out) && width >= V;
  const int64_t col_tiles = ceil_div<int64_t>(width, (int64_t)kThreads * (vec ? V : 1));
  // enough workgroups to fill the chip several times over, each thread keeping its columns' statistics
  const int64_t row_lanes = std::max<int64_t>(1, std::min<int64_t>(ceil_div<int64_t>(n, kRowsInFlight),
                                                                    ceil_div<int64_t>(8192, col_tiles)));
  const int64_t blocks = col_tiles * row_lanes;
  BSIG_REQUIRE(blocks <= INT32_MAX, "%s: width %lld needs too many workgroups", who, (long long)width);
  if (vec)
    hipLaunchKernelGGL((apply_kernel<T, V>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, ld_x, mean, inv_std,
                       out, ld_out, n, width, col_tiles, row_lanes);
  else
    hipLaunchKernelGGL((apply_kernel<T, 1>), dim3((unsigned)blocks), dim3(kThreads), 0, st, x, ld_x, mean, inv_std,
                       out, ld_out, n, width, col_tiles, row_lanes);
  BSIG_CHECK_LAUNCH(who);
  return BSIG_OK;
}

}  // namespace inorm
}  // namespace bsig
