// The random-feature kernel mean embedding summary (include/bsig_kme.h) in fp32 (csrc/kme.hip) and in
// double (csrc/f64/kme_f64.hip) from this one template, and its two small companions: the rows x_t written
// out (kme_rows_kernel, for the statistics of the scale and for tests) and the coefficients from the
// frequencies and those statistics (kme_coeff_kernel).
//
// A workgroup of kThreads threads (kWaves wavefronts) takes a trajectory and walks it in time blocks of
// kBlock rows.  A block in LDS is X[kBlock][pitch], pitch = dpad + 1 with dpad = d rounded up to 8: row r is
// x_(t0 + r) = [tau | s | a | ds] formed from memory while loading (a state is read from HBM once, its second
// and third reads for the difference hit the cache; the lanes run along k, kStageBatch elements a thread in
// flight), rows t >= M and columns d..dpad-1 zero.  The odd pitch: the 32 lanes of a half-wavefront read X[r][k] at one k and 32 rows, 32 banks.
// Column tiles of kTile frequencies are dealt to the wavefronts (tile_sums):
//   fp32    z on v_mfma_f32_32x32x2_f32: lane l holds A[row l & 31][k] and B[k][frequency l & 31] at
//           k = k0 + 4 (l >> 5) + e for the e-th MFMA of a k-group of 8, so a lane reads four consecutive
//           coefficients of its frequency -- one 16-byte load where the pointer and the pitch allow
//           (Python's buffers do) -- and four consecutive words of its row.  A frequency beyond m reads
//           row m - 1 again (its sums are dropped), a coefficient column beyond d counts as zero whatever
//           the padding holds.  The accumulators: column l & 31, rows (reg & 3) + 8 (reg >> 2) + 4 (l >> 5).
//   double  lane l: frequency l & 31, rows 16 (l >> 5) .. + 15, sixteen fma chains over ascending k, X
//           broadcast from LDS.
// then sincos of every accumulator, rows >= the block's valid rows masked out (groups of 8 rows that are
// masked as a whole are skipped: their zeros would not change a bit), a lane's rows added in ascending
// order, lane l + lane l + 32 (lower rows first).
// A trajectory of one block (M <= kBlock): G of them are staged at once and their (trajectory, tile) items
// dealt to the wavefronts, any number of tiles.  A longer one: the blocks in ascending t, a wavefront keeps
// the running sums of ONE tile in two registers, so beyond kWaves tiles (m > 128) the trajectory is walked
// once per kWaves tiles (re-read through the cache); no register array is indexed by a run-time tile.
// The constants tau_r = 1 / max(M - 1, 1) (a division in T) and a / M = (T)(sqrt(1.0 / m) / M) (made in
// double, rounded once) come from the host.
// With lengths (include/bsig_ragged.h, kRagged) the same kernels take M per trajectory: G and the blocks' layout
// are those of ts; a row is masked, and its loads are clamped, by its own trajectory's M; a longer trajectory
// walks ceil(M_n / kBlock) blocks (G > 1 only where the M of ts is one block, so the members of a group never
// differ in that); and the two constants are made on the device by the host's own divisions in the host's
// types (the root of a / M comes from the host), so a row has the bits of the fixed-length launch on its slice.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "ragged.h"
#include "../../include/bsig_ragged.h"

namespace bsig {
namespace kme {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr int kBlock = BSIG_KME_BLOCK_ROWS;      // rows of a time block: the M of the MFMA tile
constexpr int kTile = 32;                        // frequencies of a column tile: its N
constexpr int kMaxGroup = 8;                     // one-block trajectories that share a workgroup at most
constexpr int64_t kGroupBytes = 32 * 1024;       // ... and the LDS their blocks take together at most
constexpr int kStageBatch = 8;                   // elements a thread has in flight while staging
constexpr int kAhead = 4;                        // k-groups of 8 whose operands are fetched a turn ahead
static_assert(kBlock == 32 && kTile == 32, "the tile is the 32x32 MFMA's");

typedef float f32x16 __attribute__((ext_vector_type(16)));

struct Plan {
  int steps = 0;           // M
  int d = 0, dpad = 0;     // the width of a row, and rounded up to 8
  int pitch = 0;           // elements between the rows of a block in LDS
  int block_elems = 0;     // of one block
  int n_blocks = 0;        // of a trajectory
  int tiles = 0;           // column tiles
  int group = 0;           // G
  int stage_shift = 0;     // log2 of the columns the threads spread over while staging: 8 .. kThreads
  size_t lds = 0;
};

inline int64_t row_dim(int64_t sd, int64_t ad, int diff, int time) {
  if (sd < 1 || ad < 1 || sd > INT32_MAX || ad > INT32_MAX) return -1;
  const int64_t d = (diff ? 2 : 1) * sd + ad + (time ? 1 : 0);
  return d > INT32_MAX - 8 ? -1 : d;
}

// The checks of a trajectory's shape that every entry point shares; M and d where they pass.
inline int dims(const char* what, int ts, int ta, int sd, int ad, int diff, int time, int* steps_out, int* d_out) {
  BSIG_REQUIRE(ts >= 1, "%s: ts %d below 1", what, ts);
  BSIG_REQUIRE(ta >= 1, "%s: ta %d below 1", what, ta);
  BSIG_REQUIRE(sd >= 1 && ad >= 1, "%s: bad dims sd=%d ad=%d", what, sd, ad);
  const int steps = diff ? ts - 1 : ts;
  BSIG_REQUIRE(steps >= 1, "%s: ts %d leaves no state difference (M = %d)", what, ts, steps);
  const int64_t d = row_dim(sd, ad, diff, time);
  BSIG_REQUIRE(d > 0, "%s: the row width for sd=%d ad=%d is past 2^31 - 1", what, sd, ad);
  *steps_out = steps;
  *d_out = (int)d;
  return BSIG_OK;
}

// The launch shape, or why there is none (the checks bsig_kme, bsig_kme_f64 and bsig_kme_fits share).
inline int plan(const char* what, int ts, int ta, int sd, int ad, int m, int diff, int time, int itemsize,
                Plan* p) {
  int steps = 0, d = 0;
  BSIG_TRY(dims(what, ts, ta, sd, ad, diff, time, &steps, &d));
  BSIG_REQUIRE(m >= 1, "%s: m %d below 1", what, m);
  BSIG_REQUIRE(m <= (INT32_MAX - kTile) / 2, "%s: m %d: the width 2 m is past 2^31 - 1", what, m);
  const int64_t dpad = round_up<int64_t>(d, 8), pitch = dpad + 1;
  const int64_t block_bytes = (int64_t)kBlock * pitch * itemsize;      // a multiple of 16
  if (block_bytes > (int64_t)kLdsBytes) {
    set_error("%s: %lld B of LDS needed for one block of %d rows of %d columns, sd=%d ad=%d (%zu in a "
              "workgroup)", what, (long long)block_bytes, kBlock, d, sd, ad, kLdsBytes);
    return BSIG_EUNSUPPORTED;
  }
  int group = 1;
  if (steps <= kBlock)
    while (group < kMaxGroup && 2 * group * block_bytes <= kGroupBytes) group *= 2;
  p->steps = steps;
  p->d = d;
  p->dpad = (int)dpad;
  p->pitch = (int)pitch;
  p->block_elems = (int)(kBlock * pitch);
  p->n_blocks = ceil_div(steps, kBlock);
  p->tiles = ceil_div(m, kTile);
  p->group = group;
  p->stage_shift = 3;
  while ((1 << p->stage_shift) < dpad && (1 << p->stage_shift) < kThreads) ++p->stage_shift;
  p->lds = (size_t)(group * block_bytes);
  return BSIG_OK;
}

// What a trajectory's shape is to the kernels: the same few numbers everywhere.
template <typename T>
struct Shape {
  int ts, ta, sd, ad, diff, time, steps, d;
  T tau_r;
};

// Element k of row x_t of the trajectory (s, a): 0 for t >= M or k >= d.
template <typename T>
__device__ __forceinline__ T element_at(const T* __restrict__ s, const T* __restrict__ a, const Shape<T>& g,
                                        int t, int k) {
  if (t >= g.steps || k >= g.d) return (T)0;
  if (g.time) {
    if (k == 0) return (T)t * g.tau_r;
    k -= 1;
  }
  if (k < g.sd) return s[(int64_t)t * g.sd + k];
  k -= g.sd;
  if (k < g.ad) return a[(int64_t)min(t, g.ta - 1) * g.ad + k];
  k -= g.ad;
  return s[(int64_t)(t + 1) * g.sd + k] - s[(int64_t)t * g.sd + k];
}

template <typename T>
__global__ __launch_bounds__(kThreads) void kme_rows_kernel(const T* __restrict__ states,
                                                            const T* __restrict__ actions,
                                                            T* __restrict__ rows, int64_t total,
                                                            int64_t ld_rows, Shape<T> g) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int64_t q = idx / g.d;                  // the row: trajectory i, step t
    const int k = (int)(idx - q * g.d);
    const int64_t i = q / g.steps;
    const int t = (int)(q - i * g.steps);
    rows[q * ld_rows + k] = element_at<T>(states + i * (int64_t)g.ts * g.sd,
                                          actions + i * (int64_t)g.ta * g.ad, g, t, k);
  }
}

// The valid rows only, compacted (bsig_kme_rows_ragged): a workgroup takes a trajectory at a time and writes its
// M_n rows from row offsets[n] on, an element a thread.
template <typename T>
__global__ __launch_bounds__(kThreads) void kme_rows_ragged_kernel(const T* __restrict__ states,
                                                                   const T* __restrict__ actions,
                                                                   const int32_t* __restrict__ lengths,
                                                                   const int64_t* __restrict__ offsets,
                                                                   T* __restrict__ rows, int64_t n, int64_t ld_rows,
                                                                   Shape<T> g) {
  for (int64_t i = blockIdx.x; i < n; i += gridDim.x) {
    Shape<T> own = g;
    own.steps = ragged::steps_of(lengths, i, g.ts, g.diff).steps;
    own.tau_r = (T)1 / (T)max(own.steps - 1, 1);
    const T* s = states + i * (int64_t)g.ts * g.sd;
    const T* a = actions + i * (int64_t)g.ta * g.ad;
    T* o = rows + offsets[i] * ld_rows;
    for (int e = threadIdx.x; e < own.steps * g.d; e += blockDim.x) {
      const int t = e / g.d, k = e - t * g.d;
      o[(int64_t)t * ld_rows + k] = element_at<T>(s, a, own, t, k);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void kme_coeff_kernel(const float* __restrict__ freqs, int64_t ld_freqs,
                                                             const double* __restrict__ inv_std, double kappa,
                                                             T* __restrict__ coeff, int64_t ld_coeff,
                                                             int64_t m, int64_t d) {
  const int64_t total = m * ld_coeff, stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += stride) {
    const int64_t j = idx / ld_coeff, k = idx - j * ld_coeff;
    coeff[idx] = k < d ? (T)__dmul_rn(__dmul_rn((double)freqs[j * ld_freqs + k], inv_std[k]), kappa) : (T)0;
  }
}

// Sine and cosine of an fp32 accumulator.  Sixteen of each follow every tile's MFMAs, on the vector ALU, whose
// instructions share the SIMD's issue with the MFMAs; up to |z| = 8192 this is the classic single-precision scheme
// -- some 30 instructions for the pair, where the library's sincosf with its large-argument path is several times
// that -- : n = rint(z 2/pi), r = z - n pi/2 with pi/2 in three pieces whose products with n are exact (Cody and
// Waite), the degree-7 / degree-8 minimax polynomials of sin and cos on [-pi/4, pi/4], the quadrant from n mod 4.
// (Measured, profiles/kme_NOTES.md: fewer instructions, but NO shorter launch at three waves a SIMD -- 1407
// against 1421 us for Ant -- because the wavefronts wait elsewhere; kept for when they do not.)
// n has 13 bits up to there and the first two pieces 7 and 11, so both products are exact; the reduction
// errs by a rounding or two of values below 4 and the polynomials by 2e-7 relative: some 4e-7 absolute in all
// (an fp32 emulation over three million arguments up to 8192: 9.3e-8), against the 3e-6 the summary's bound allows
// for either.  Beyond 8192, and for a non-finite z, sincosf answers.
__device__ __forceinline__ void sin_cos(float z, float* s, float* c) {
  if (!(fabsf(z) <= 8192.f)) {
    sincosf(z, s, c);
    return;
  }
  const float n = rintf(z * 0.636619772367581343f);
  float r = fmaf(-n, 1.5703125f, z);
  r = fmaf(-n, 4.83751296997070312e-4f, r);
  r = fmaf(-n, 7.54978995489188216e-8f, r);
  const float r2 = r * r;
  const float sp = fmaf(fmaf(fmaf(-1.9515295891e-4f, r2, 8.3321608736e-3f), r2, -1.6666654611e-1f), r2 * r, r);
  const float cp = fmaf(fmaf(fmaf(2.443315711809948e-5f, r2, -1.388731625493765e-3f), r2, 4.166664568298827e-2f),
                        r2 * r2, fmaf(-0.5f, r2, 1.f));
  const int q = (int)n;
  const float sv = (q & 1) ? cp : sp, cv = (q & 1) ? sp : cp;
  *s = (q & 2) ? -sv : sv;
  *c = ((q + 1) & 2) ? -cv : cv;
}
__device__ __forceinline__ void sin_cos(double z, double* s, double* c) { sincos(z, s, c); }

// A value loaded for a LATER iteration is a loop-carried load, and the compiler turns a loop-carried load back
// into a load at the top of the iteration that uses it (it carries the address instead), which puts the whole
// memory latency in front of every group of MFMAs.  It does not do so across something that may write memory:
// this empty statement is that, and emits no instruction.
#define BSIG_KME_KEEP_LOADS_AHEAD() asm volatile("" ::: "memory")

// z of a (block, tile) on the MFMA: acc += X[32 rows][k] * coeff[frequency][k] over k < dpad.  kVec: the
// coefficient rows allow 16-byte loads; then the k-groups whose 8 columns all exist run in a loop without a
// branch, kAhead groups a turn: the coefficients and the rows of the next turn are fetched before this turn's
// 4 kAhead MFMAs (a load from L2 takes longer than a group's four MFMAs; a turn's groups beyond the last
// read the last again with zero rows).  The
// last, partial group -- and every group without kVec -- reads its coefficients one by one, 0 beyond d.
template <bool kVec>
__device__ __forceinline__ void tile_z(const float* __restrict__ xr, const float* __restrict__ cj, int h, int d,
                                       int dpad, f32x16& acc) {
  const int full = kVec ? (d & ~7) : 0;
  if (full > 0) {
    const float* cq = cj + 4 * h;
    const float* xq = xr + 4 * h;
    const int last = full - 8;
    float4 cn[kAhead];
    float an[kAhead][4];
    // the coefficients and the rows of groups g0 .. g0 + kAhead - 1; a group beyond the last reads the last
    // again with zero rows: its products add +0
    auto fetch = [&](int g0) {
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        const int k = min((g0 + u) * 8, last);
        const bool in = (g0 + u) * 8 < full;
        cn[u] = *reinterpret_cast<const float4*>(cq + k);
#pragma unroll
        for (int e = 0; e < 4; ++e) an[u][e] = in ? xq[k + e] : 0.f;
      }
    };
    fetch(0);
    BSIG_KME_KEEP_LOADS_AHEAD();
    for (int g0 = 0; g0 * 8 < full; g0 += kAhead) {
      float4 c[kAhead];
      float a[kAhead][4];
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        c[u] = cn[u];
#pragma unroll
        for (int e = 0; e < 4; ++e) a[u][e] = an[u][e];
      }
      fetch(g0 + kAhead);
      BSIG_KME_KEEP_LOADS_AHEAD();
#pragma unroll
      for (int u = 0; u < kAhead; ++u) {
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][0], c[u].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][1], c[u].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][2], c[u].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[u][3], c[u].w, acc, 0, 0, 0);
      }
    }
  }
  for (int k0 = full; k0 < dpad; k0 += 8) {
    const int kb = k0 + 4 * h;
    const float b0 = kb + 0 < d ? cj[kb + 0] : 0.f, b1 = kb + 1 < d ? cj[kb + 1] : 0.f;
    const float b2 = kb + 2 < d ? cj[kb + 2] : 0.f, b3 = kb + 3 < d ? cj[kb + 3] : 0.f;
    const float a0 = xr[kb + 0], a1 = xr[kb + 1], a2 = xr[kb + 2], a3 = xr[kb + 3];
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a2, b2, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a3, b3, acc, 0, 0, 0);
  }
}

// The sums over the `valid` first rows of the block X of cos z and sin z for the frequencies of `tile`: both
// lanes l and l + 32 return those of frequency tile * kTile + (l & 31).
__device__ __forceinline__ void tile_sums(const float* __restrict__ X, const float* __restrict__ coeff,
                                          int64_t ld_coeff, int vec_ok, int tile, int m, int d, int dpad,
                                          int pitch, int valid, float* cs_out, float* sn_out) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  const float* cj = coeff + (int64_t)min(tile * kTile + l31, m - 1) * ld_coeff;
  const float* xr = X + l31 * pitch;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  if (vec_ok)
    tile_z<true>(xr, cj, h, d, dpad, acc);
  else
    tile_z<false>(xr, cj, h, d, dpad, acc);
  float cs = 0.f, sn = 0.f;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (8 * q < valid) {                          // (uniform: rows 8 q .. 8 q + 7 of both halves)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s, c;
        sin_cos(acc[4 * q + e], &s, &c);
        const bool on = 8 * q + 4 * h + e < valid;
        cs += on ? c : 0.f;
        sn += on ? s : 0.f;
      }
    }
  }
  const float co = __shfl_xor(cs, 32, 64), so = __shfl_xor(sn, 32, 64);
  *cs_out = h == 0 ? cs + co : co + cs;
  *sn_out = h == 0 ? sn + so : so + sn;
}

__device__ __forceinline__ void tile_sums(const double* __restrict__ X, const double* __restrict__ coeff,
                                          int64_t ld_coeff, int /*vec_ok*/, int tile, int m, int d,
                                          int /*dpad*/, int pitch, int valid, double* cs_out, double* sn_out) {
  const int lane = threadIdx.x & 63, l31 = lane & 31, h = lane >> 5;
  const double* cj = coeff + (int64_t)min(tile * kTile + l31, m - 1) * ld_coeff;
  const double* xr = X + 16 * h * pitch;
  double z[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) z[r] = 0.0;
  // eight coefficients of the next columns are on their way while the chains run over these eight (a column
  // beyond d reads d - 1 again and is not used)
  double bn[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) bn[u] = cj[min(u, d - 1)];
  BSIG_KME_KEEP_LOADS_AHEAD();
  for (int k0 = 0; k0 < d; k0 += 8) {
    double b[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      b[u] = bn[u];
      bn[u] = cj[min(k0 + 8 + u, d - 1)];
    }
    BSIG_KME_KEEP_LOADS_AHEAD();
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      if (k0 + u < d) {
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = fma(xr[r * pitch + k0 + u], b[u], z[r]);
      }
    }
  }
  double cs = 0.0, sn = 0.0;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    if (8 * q < valid) {                          // (uniform: rows 8 q .. of the lower half, 16 + 8 q .. of the upper)
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        double s, c;
        sin_cos(z[8 * q + e], &s, &c);
        const bool on = 16 * h + 8 * q + e < valid;
        cs += on ? c : 0.0;
        sn += on ? s : 0.0;
      }
    }
  }
  const double co = __shfl_xor(cs, 32, 64), so = __shfl_xor(sn, 32, 64);
  *cs_out = h == 0 ? cs + co : co + cs;
  *sn_out = h == 0 ? sn + so : so + sn;
}

// (kRagged: `lengths` holds every trajectory's own length and `a_root` is sqrt(1 / m), a_over_m is not read; else
// neither is read)
template <typename T, bool kRagged>
__global__ __launch_bounds__(kThreads) void kme_kernel(const T* __restrict__ states, const T* __restrict__ actions,
                                                       const int32_t* __restrict__ lengths,
                                                       const T* __restrict__ coeff, int64_t ld_coeff, int vec_ok,
                                                       T* __restrict__ out, int64_t n, int m, int64_t ld_out,
                                                       T a_over_m, double a_root, int32_t* __restrict__ nonfinite,
                                                       Shape<T> g, Plan p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char kme_smem[];
  T* X = reinterpret_cast<T*>(kme_smem);
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int dpad = p.dpad, pitch = p.pitch, G = p.group;
  const int64_t traj_s = (int64_t)g.ts * g.sd, traj_a = (int64_t)g.ta * g.ad;
  bool bad = false;

  // `nrows` rows of X from trajectory `first` on, kBlock rows each from step t0: row vr is step t0 + vr % kBlock
  // of trajectory first + vr / kBlock (the blocks of a group follow each other in LDS).  A thread owns a column
  // (of 2^stage_shift, the lanes along k: adjacent addresses) and every rpp-th row.  What a column is -- zero,
  // tau, a state, an action, a difference -- is decided once per column and turned into two base pointers and a
  // stride, so that an element is two loads and a few selects WITHOUT a branch (a plain column loads its value
  // twice): kStageBatch elements a thread are then on their way from memory before the first is stored.  (With a
  // branch per kind the compiler waits for an element's loads where its branches meet, one element after the other.)
  // kRagged: `own_steps` is the M of the one trajectory the rows come from, or -1: the rows of a group, each
  // trajectory's M looked up per row (a load more in the batch; the length is clamped before it indexes).
  auto stage = [&](int64_t first, int t0, int nrows, int own_steps) {
    T own_tau_r = g.tau_r;
    if constexpr (kRagged) {
      if (own_steps >= 0) own_tau_r = (T)1 / (T)max(own_steps - 1, 1);
    }
    const int cols = 1 << p.stage_shift, col = tid & (cols - 1), row0 = tid >> p.stage_shift;
    const int rpp = kThreads >> p.stage_shift, iters = nrows / rpp;
    for (int k = col; k < dpad; k += cols) {
      enum { kZero, kTau, kPlain, kDiff };
      int kind = kZero, stride = 0, tmax = 0;
      int64_t per_traj = traj_s;
      const T* hi = states;       // the value, or the later state of a difference
      const T* lo = states;       // the earlier state of a difference (else: hi again)
      const int c = k - g.time;
      if (k < g.d) {
        if (c < 0) {
          kind = kTau;
        } else if (c < g.sd) {
          kind = kPlain; hi = lo = states + c; stride = g.sd; tmax = g.steps - 1;
        } else if (c < g.sd + g.ad) {
          kind = kPlain; hi = lo = actions + (c - g.sd); stride = g.ad; tmax = min(g.steps, g.ta) - 1;
          per_traj = traj_a;
        } else {
          kind = kDiff; lo = states + (c - g.sd - g.ad); hi = lo + g.sd; stride = g.sd; tmax = g.steps - 1;
        }
      }
      for (int i0 = 0; i0 < iters; i0 += kStageBatch) {
        T v[kStageBatch];
#pragma unroll
        for (int u = 0; u < kStageBatch; ++u) {
          const int vr = min(row0 + (i0 + u) * rpp, nrows - 1);      // (beyond the last: read again, not stored)
          const int t = t0 + vr % kBlock;
          int steps = g.steps, tlast = tmax;
          T tau_r = g.tau_r;
          if constexpr (kRagged) {
            steps = own_steps;
            tau_r = own_tau_r;
            if (own_steps < 0) {
              steps = ragged::steps_of(lengths, first + vr / kBlock, g.ts, g.diff).steps;
              if (kind == kTau) tau_r = (T)1 / (T)max(steps - 1, 1);
            }
            tlast = min(tmax, steps - 1);      // (the actions' min(M, ta) - 1 included: M_n <= M)
          }
          const int64_t off = (first + vr / kBlock) * per_traj + (int64_t)min(t, tlast) * stride;
          const T x1 = hi[off], x0 = lo[off];
          T x = kind == kDiff ? x1 - x0 : x1;
          x = kind == kTau ? (T)t * tau_r : x;
          v[u] = (kind == kZero || t >= steps) ? (T)0 : x;
        }
#pragma unroll
        for (int u = 0; u < kStageBatch; ++u)
          if (i0 + u < iters) X[(row0 + (i0 + u) * rpp) * pitch + k] = v[u];
      }
    }
  };
  // (`scale`: a / M of the trajectory; `valid`: its length was inside the range, else the row is NaN)
  auto store = [&](int64_t traj, int tile, T cs, T sn, T scale, bool valid) {
    const int j = tile * kTile + (lane & 31);
    if (lane < 32 && j < m) {
      const T c = valid ? cs * scale : (T)NAN, s = valid ? sn * scale : (T)NAN;
      T* o = out + traj * ld_out;
      o[j] = c;
      o[m + j] = s;
      bad |= !isfinite(c) || !isfinite(s);
    }
  };

  for (int64_t base = (int64_t)blockIdx.x * G; base < n; base += (int64_t)gridDim.x * G) {
    if (p.n_blocks == 1) {
      const int ng = (int)min((int64_t)G, n - base);
      __syncthreads();                            // the items before are done with the LDS
      stage(base, 0, ng * kBlock, -1);
      __syncthreads();
      for (int item = wave; item < ng * p.tiles; item += kWaves) {
        const int gi = item / p.tiles, tile = item - gi * p.tiles;
        int steps = g.steps;
        T scale = a_over_m;
        bool valid = true;
        if constexpr (kRagged) {
          const ragged::Steps own = ragged::steps_of(lengths, base + gi, g.ts, g.diff);
          steps = own.steps;
          valid = own.valid;
          scale = (T)(a_root / (double)steps);
        }
        T cs, sn;
        tile_sums(X + gi * p.block_elems, coeff, ld_coeff, vec_ok, tile, m, g.d, dpad, pitch, steps, &cs, &sn);
        store(base + gi, tile, cs, sn, scale, valid);
      }
    } else {
      // (one trajectory a workgroup here: its length is the same for every thread, and so are the barriers)
      int steps = g.steps, n_blocks = p.n_blocks;
      T scale = a_over_m;
      bool valid = true;
      if constexpr (kRagged) {
        const ragged::Steps own = ragged::steps_of(lengths, base, g.ts, g.diff);
        steps = own.steps;
        valid = own.valid;
        n_blocks = ceil_div(steps, kBlock);
        scale = (T)(a_root / (double)steps);
      }
      for (int tile0 = 0; tile0 < p.tiles; tile0 += kWaves) {
        const int tile = tile0 + wave;
        T cs = (T)0, sn = (T)0;
        for (int b = 0; b < n_blocks; ++b) {
          __syncthreads();
          stage(base, b * kBlock, kBlock, steps);
          __syncthreads();
          if (tile < p.tiles) {
            T c1, s1;
            tile_sums(X, coeff, ld_coeff, vec_ok, tile, m, g.d, dpad, pitch, min(kBlock, steps - b * kBlock),
                      &c1, &s1);
            cs += c1;
            sn += s1;
          }
        }
        if (tile < p.tiles) store(base, tile, cs, sn, scale, valid);
      }
    }
  }
  if (bad && nonfinite) atomicOr(nonfinite, 1);
}

template <typename T>
inline Shape<T> shape_of(int ts, int ta, int sd, int ad, int diff, int time, int steps, int d) {
  Shape<T> g;
  g.ts = ts; g.ta = ta; g.sd = sd; g.ad = ad; g.diff = diff ? 1 : 0; g.time = time ? 1 : 0;
  g.steps = steps;
  g.d = d;
  g.tau_r = (T)1 / (T)std::max(steps - 1, 1);
  return g;
}

// bsig_kme / bsig_kme_f64 and, with lengths, bsig_kme_ragged / bsig_kme_ragged_f64: the argument checks, the
// plan, the constants, the launch.  `max_grid`: the precision's workgroup cap.
template <typename T, bool kRagged>
int run_any(const char* what, int64_t max_grid, const T* states, const T* actions, const int32_t* lengths,
            const T* coeff, int64_t ld_coeff, T* out, int64_t n, int ts, int ta, int sd, int ad, int m, int diff,
            int time, int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "%s: bad n=%lld", what, (long long)n);
  Plan p;
  BSIG_TRY(plan(what, ts, ta, sd, ad, m, diff, time, (int)sizeof(T), &p));
  BSIG_REQUIRE(ld_out >= 2 * (int64_t)m, "%s: ld_out %lld below the width %lld (2 m)", what, (long long)ld_out,
               2 * (long long)m);
  BSIG_REQUIRE(ld_coeff >= p.d, "%s: ld_coeff %lld below the row width %d", what, (long long)ld_coeff, p.d);
  BSIG_REQUIRE(states && actions && coeff && out, "%s: null pointer", what);
  if (kRagged) BSIG_REQUIRE(lengths, "%s: null lengths", what);
  static LdsRaised raised;
  if (p.lds > kLdsUnraised) BSIG_TRY(raise_lds_limit(kme_kernel<T, kRagged>, kLdsBytes, &raised));
  const int vec_ok = ld_coeff % 4 == 0 && aligned(coeff, 16);
  const double a_root = std::sqrt(1.0 / (double)m);
  const T a_over_m = (T)(a_root / (double)p.steps);
  hipLaunchKernelGGL((kme_kernel<T, kRagged>), dim3(capped_grid(ceil_div<int64_t>(n, p.group), max_grid)),
                     dim3(kThreads), p.lds, as_stream(stream), states, actions, lengths, coeff, ld_coeff, vec_ok, out,
                     n, m, ld_out, a_over_m, a_root, nonfinite,
                     shape_of<T>(ts, ta, sd, ad, diff, time, p.steps, p.d), p);
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

template <typename T>
int run(const char* what, int64_t max_grid, const T* states, const T* actions, const T* coeff, int64_t ld_coeff,
        T* out, int64_t n, int ts, int ta, int sd, int ad, int m, int diff, int time, int64_t ld_out,
        int32_t* nonfinite, bsig_stream_t stream) {
  return run_any<T, false>(what, max_grid, states, actions, nullptr, coeff, ld_coeff, out, n, ts, ta, sd, ad, m, diff,
                           time, ld_out, nonfinite, stream);
}

template <typename T>
int run_rows(const char* what, const T* states, const T* actions, T* rows, int64_t n, int ts, int ta, int sd,
             int ad, int diff, int time, int64_t ld_rows, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "%s: bad n=%lld", what, (long long)n);
  int steps = 0, d = 0;
  BSIG_TRY(dims(what, ts, ta, sd, ad, diff, time, &steps, &d));
  BSIG_REQUIRE(ld_rows >= d, "%s: ld_rows %lld below the row width %d", what, (long long)ld_rows, d);
  BSIG_REQUIRE(states && actions && rows, "%s: null pointer", what);
  BSIG_REQUIRE(n <= INT64_MAX / ((int64_t)steps * d), "%s: n=%lld rows of %d x %d elements are past 2^63", what,
               (long long)n, steps, d);
  const int64_t total = n * steps * d;
  hipLaunchKernelGGL((kme_rows_kernel<T>), dim3(capped_grid(ceil_div<int64_t>(total, kThreads), kSummaryGridCap)),
                     dim3(kThreads), 0, as_stream(stream), states, actions, rows, total, ld_rows,
                     shape_of<T>(ts, ta, sd, ad, diff, time, steps, d));
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

template <typename T>
int run_rows_ragged(const char* what, const T* states, const T* actions, const int32_t* lengths,
                    const int64_t* offsets, T* rows, int64_t n, int ts, int ta, int sd, int ad, int diff, int time,
                    int64_t ld_rows, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "%s: bad n=%lld", what, (long long)n);
  int steps = 0, d = 0;
  BSIG_TRY(dims(what, ts, ta, sd, ad, diff, time, &steps, &d));
  BSIG_REQUIRE(ld_rows >= d, "%s: ld_rows %lld below the row width %d", what, (long long)ld_rows, d);
  BSIG_REQUIRE(states && actions && rows, "%s: null pointer", what);
  BSIG_REQUIRE(lengths, "%s: null lengths", what);
  BSIG_REQUIRE(offsets, "%s: null offsets", what);
  BSIG_REQUIRE(n <= INT64_MAX / ((int64_t)steps * d), "%s: n=%lld rows of %d x %d elements are past 2^63", what,
               (long long)n, steps, d);
  BSIG_REQUIRE((int64_t)steps * d <= INT32_MAX, "%s: a trajectory of %d x %d elements is past 2^31 - 1", what, steps,
               d);
  hipLaunchKernelGGL((kme_rows_ragged_kernel<T>), dim3(capped_grid(n, kSummaryGridCap)), dim3(kThreads), 0,
                     as_stream(stream), states, actions, lengths, offsets, rows, n, ld_rows,
                     shape_of<T>(ts, ta, sd, ad, diff, time, steps, d));
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

template <typename T>
int run_coeff(const char* what, const float* freqs, int64_t ld_freqs, const double* inv_std, double kappa, T* coeff,
              int64_t ld_coeff, int64_t m, int64_t d, bsig_stream_t stream) {
  BSIG_REQUIRE(m >= 1 && d >= 1, "%s: bad shape m=%lld d=%lld", what, (long long)m, (long long)d);
  BSIG_REQUIRE(ld_freqs >= d, "%s: ld_freqs %lld below d=%lld", what, (long long)ld_freqs, (long long)d);
  BSIG_REQUIRE(ld_coeff >= d, "%s: ld_coeff %lld below d=%lld", what, (long long)ld_coeff, (long long)d);
  BSIG_REQUIRE(m <= INT64_MAX / ld_coeff, "%s: m=%lld rows of pitch %lld are past 2^63", what, (long long)m,
               (long long)ld_coeff);
  BSIG_REQUIRE(freqs && inv_std && coeff, "%s: null pointer", what);
  hipLaunchKernelGGL((kme_coeff_kernel<T>), dim3(capped_grid(ceil_div<int64_t>(m * ld_coeff, kThreads), kSummaryGridCap)),
                     dim3(kThreads), 0, as_stream(stream), freqs, ld_freqs, inv_std, kappa, coeff, ld_coeff, m, d);
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

}  // namespace kme
}  // namespace bsig
