// The start, cross-correlation and signature summaries (bsig_summary_start, bsig_crosscorr, bsig_signature) in fp32
// (csrc/summarizers.hip) and in double (csrc/f64/summarizers_f64.hip, include/bsig_f64.h: what the reference's torch
// ops give under torch.set_default_dtype(torch.float64)) from this one template. Replaces the PyTorch op sequences of
// bayes_sim_ig/utils/summarizers.py (reference file:line cited per kernel).  One workgroup per trajectory; all global
// traffic is lane-contiguous.
// T is the element type and kVec<T> the elements of a 16-byte word (4 | 2): the width of every vector read and store,
// of the padding of the increments' rows and of the stage's alignment phase.  What only fp32 has -- the wave and
// quads kernels of the cross-correlation and its factor rows -- sits behind `if constexpr (kF32<T>)` in the kernels
// and behind Precision::f32_paths in the plans.  The plans (start_path, crosscorr_path, signature_path) take
// everything else that differs from a Precision.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "../../include/bsig_f64.h"

namespace bsig {
namespace summaries {

template <typename T> constexpr bool kF32 = std::is_same<T, float>::value;
template <typename T> constexpr int kVec = 16 / (int)sizeof(T);
template <typename T> constexpr int kVecLog = kF32<T> ? 2 : 1;          // (shifts: the operands are signed)
template <typename T> using Vec = T __attribute__((ext_vector_type(kVec<T>)));

using bsig::wave_max;
__device__ inline double wave_max(double v) {
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
  return v;
}

// HipVec, all_finite, pack and scaled are spelled as they are because the fp32 kernels' instruction streams are compared
// with their predecessors' (profiles/summaries_template_NOTES.md a): a generic rewrite changes them.
template <typename T> using HipVec = typename std::conditional<kF32<T>, float4, double2>::type;   // (.x .y ..)
template <typename T, typename W>
__device__ __forceinline__ bool all_finite(const W& v) {
  if constexpr (kF32<T>) return isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w);
  else return isfinite(v.x) && isfinite(v.y);
}
// A store of the cross-correlation's products.  fp32 streams them past the caches (nontemporal: 4.4 against 4.1 TB/s
// of cached stores, profiles/r03_fill_bench.txt); double stores plainly, as it always has: Ant's rows of doubles
// took 1.2 times as long streamed (profiles/summaries_template_NOTES.md; the signature's did not).
template <typename T, typename W>
__device__ __forceinline__ void product_store(const W& v, W* p) {
  if constexpr (kF32<T>) __builtin_nontemporal_store(v, p);
  else *p = v;
}
// the 16-byte word a vector store takes
template <typename T>
__device__ __forceinline__ Vec<T> pack(const HipVec<T>& a) {
  if constexpr (kF32<T>) return Vec<T>{a.x, a.y, a.z, a.w};
  else return Vec<T>{a.x, a.y};
}
// sv * a, one multiply per element
template <typename T>
__device__ __forceinline__ Vec<T> scaled(T sv, const HipVec<T>& a) {
  if constexpr (kF32<T>) return Vec<T>{sv * a.x, sv * a.y, sv * a.z, sv * a.w};
  else return Vec<T>{sv * a.x, sv * a.y};
}

// ------------------------------------------------------------------ K1
// summary_start / summary_waypts: summarizers.py:65-87 after the crop/pad of :20-62.  2 sizeof(T) W (sd+ad) B / trajectory.
//   out[n, t*(sd+ad)+c] = c<sd ? s[n,min(t,Ts-1),c] : a[n,min(t,Ta-1),c-sd]
template <typename T, int UNROLL_T>
__global__ __launch_bounds__(256) void summary_start_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, T* __restrict__ out, int64_t n, int ts, int ta,
    int sd, int ad, int w, int64_t ld_out) {
  const int width = sd + ad;
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const T* s = states + traj * (int64_t)ts * sd;
    const T* a = actions + traj * (int64_t)ta * ad;
    T* o = out + traj * ld_out;
    for (int t0 = 0; t0 < w; t0 += UNROLL_T) {
      for (int c = threadIdx.x; c < width; c += blockDim.x) {
        T v[UNROLL_T];
#pragma unroll
        for (int u = 0; u < UNROLL_T; ++u) {
          const int t = t0 + u;
          if (t < w) {
            v[u] = (c < sd) ? s[(int64_t)min(t, ts - 1) * sd + c]
                            : a[(int64_t)min(t, ta - 1) * ad + (c - sd)];
          }
        }
#pragma unroll
        for (int u = 0; u < UNROLL_T; ++u) {
          const int t = t0 + u;
          if (t < w) o[(int64_t)t * width + c] = v[u];
        }
      }
    }
  }
}

// mean and unbiased std of a feature row (summarizers.py:114-119: torch.mean / torch.std, two passes), taken by one
// wavefront from LDS.  Accumulated in fp64 and rounded once: for fp32 the value every fp32 summation order approximates
// (the reference's own order is a property of the torch build), at 5 elements per lane.  Same value in every lane.
template <typename T>
__device__ __forceinline__ void row_mean_std(const T* sf, int S, int ln, T& mean, T& sdev) {
  double part = 0.0;
  for (int i = ln; i < S; i += 64) part += (double)sf[i];
  const double m = wave_sum_f64(part) / (double)S;
  part = 0.0;
  for (int i = ln; i < S; i += 64) {
    const double d = (double)sf[i] - m;
    part += d * d;
  }
  mean = (T)m;
  sdev = (S < 2) ? (T)0 : (T)sqrt(wave_sum_f64(part) / (double)(S - 1));
}

// ------------------------------------------------------------------ K2
// cross_correlation: summarizers.py:90-122.
//   sf[t*(sd-1)+c] = s[t,c+1]-s[t,c]  (corrdiff, :105-106: ONE subtraction)  or  s[t,c] (:108)
//   af[t*ad+c]     = a[t,c]
//   out[i*A + j]   = sf[i]*af[j]      (bmm outer product, :112-113: ONE multiply, stored as it is)
//   out[S*A]       = mean(sf), out[S*A+1] = unbiased std(sf)   (:114-119)
// Algorithmic bytes / trajectory: sizeof(T)*(W*(sd+ad) + S*A + 2); write-bound.
// `fac` (fp32, optional): the row's FACTORS [sf S | af A | mean | std | 1 | 0..] -- everything the summary is made of,
// 1/35 of its size for Ant; `out` may then be null (no outer product): the fit engine's first layer forms
// sf[i]*af[j] itself (bsig_crosscorr_factors).
// kLean (double, rows of at most kSmallRow products: crosscorr_path): without the register prefetch, the max
// reduction and the word stores, which such a row is over too soon to repay (8 workgroups a CU against 4).
template <typename T, bool kLean = false>
__global__ __launch_bounds__(256) void crosscorr_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, T* __restrict__ out, int64_t n, int ts, int ta,
    int sd, int ad, int w, int use_diff, int64_t ld_out, int vec, int32_t* __restrict__ nonfinite,
    T* __restrict__ fac, int64_t ld_fac) {
  extern __shared__ __attribute__((aligned(16))) unsigned char summaries_smem[];
  constexpr int V = kVec<T>, VL = kVecLog<T>;
  const int sfeat = sd - 1;
  const int S = w * sfeat, A = w * ad;
  T* sf = reinterpret_cast<T*>(summaries_smem);   // [S]
  T* af = sf + S;                                  // [A]
  const int tid = threadIdx.x, nt = blockDim.x;
  // A workgroup that stops storing while it fetches and reduces its next trajectory leaves the chip's write path
  // idle for that time: with the fetch -> LDS -> mean -> std -> max chain of six workgroup barriers per trajectory
  // the kernel ran at 0.8 of what the same store loop does alone (tools/micro/fill_bench.hip).  So the NEXT
  // trajectory's features are fetched into registers before this one's store loop (their latency hides behind it),
  // and the statistics are taken by every wavefront for itself (same values, same order in each: no barrier) --
  // two barriers per trajectory.
  constexpr int kPfW = 10;                 // window <= 10 (crosscorr_window)
  const bool pf_ok = !kLean && sfeat <= nt && ad <= nt && w <= kPfW;   // (else: fetched in place, below)
  T pf_s0[kPfW], pf_s1[kPfW], pf_a[kPfW];
  auto prefetch = [&](int64_t traj) {
    const T* s = states + traj * (int64_t)ts * sd;
    const T* a = actions + traj * (int64_t)ta * ad;
#pragma unroll
    for (int t = 0; t < kPfW; ++t) {
      if (t < w) {
        const T* srow = s + (int64_t)t * sd;
        const T* arow = a + (int64_t)min(t, ta - 1) * ad;   // pad: repeat the last step (:52-58)
        if (tid < sfeat) { pf_s0[t] = srow[tid]; pf_s1[t] = use_diff ? srow[tid + 1] : (T)0; }
        if (tid < ad) pf_a[t] = arow[tid];
      }
    }
  };
  if (pf_ok && (int64_t)blockIdx.x < n) prefetch(blockIdx.x);
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const T* s = states + traj * (int64_t)ts * sd;
    const T* a = actions + traj * (int64_t)ta * ad;
    T* o = out ? out + traj * ld_out : nullptr;
    __syncthreads();
    if (pf_ok) {
#pragma unroll
      for (int t = 0; t < kPfW; ++t) {
        if (t < w) {
          if (tid < sfeat) sf[t * sfeat + tid] = use_diff ? pf_s1[t] - pf_s0[t] : pf_s0[t];
          if (tid < ad) af[t * ad + tid] = pf_a[t];
        }
      }
    } else {
      // state features: iterate (t, c) without integer division
      for (int t = 0; t < w; ++t) {
        const T* srow = s + (int64_t)t * sd;
        for (int c = tid; c < sfeat; c += nt)
          sf[t * sfeat + c] = use_diff ? (srow[c + 1] - srow[c]) : srow[c];
        // actions beyond their own length repeat the last step (pad, :52-58)
        const T* arow = a + (int64_t)min(t, ta - 1) * ad;
        for (int c = tid; c < ad; c += nt) af[t * ad + c] = arow[c];
      }
    }
    __syncthreads();
    if (pf_ok && traj + gridDim.x < n) prefetch(traj + gridDim.x);
    // mean and unbiased std (two passes, like torch.std), per wavefront
    const int ln = tid & 63;
    T mean, sdev;
    row_mean_std(sf, S, ln, mean, sdev);
    // isfinite(feats) (summarizers.py:120) without touching every product: all
    // inputs finite and max|sf| * max|af| far from overflow => every product is
    // finite; otherwise fall back to checking each product.
    T ms = (T)0, ma = (T)0;
    bool in_bad = false;
    if constexpr (!kLean) {
      for (int i = ln; i < S; i += 64) { ms = fmax(ms, fabs(sf[i])); in_bad |= !isfinite(sf[i]); }
      for (int i = ln; i < A; i += 64) { ma = fmax(ma, fabs(af[i])); in_bad |= !isfinite(af[i]); }
      ms = wave_max(ms); ma = wave_max(ma);
    }
    const bool check_each = kLean || !(ms < (T)1e18f && ma < (T)1e18f);
    if constexpr (kF32<T>) {
      if (fac) {
        T* f = fac + traj * ld_fac;
        for (int i = tid; i < S; i += nt) f[i] = sf[i];
        for (int i = tid; i < A; i += nt) f[S + i] = af[i];
        for (int i = S + A + tid; i < ld_fac; i += nt)
          f[i] = i == S + A ? mean : (i == S + A + 1 ? sdev : (i == S + A + 2 ? 1.0f : 0.f));
      }
      if (!o) {   // factors only: |sf[i] af[j]| <= max|sf| max|af|
        if (nonfinite && (in_bad || (tid == 0 && !(isfinite(ms * ma) && isfinite(mean) && isfinite(sdev)))))
          atomicOr(nonfinite, 1);
        continue;
      }
    }
    // streaming outer product
    const int64_t total = (int64_t)S * A;
    bool bad = in_bad;
    if (!kLean && vec && (A & (V - 1)) == 0 && A <= V * nt) {
      // A thread keeps ONE word of action features (columns V jq .. V jq + V - 1; fp32: a quad) in registers
      // and walks down the state features: per 16-byte store one LDS broadcast read and V multiplies
      // (the generic loop below spends ~30 instructions per store on index arithmetic and eight
      // LDS reads).  Consecutive threads cover consecutive words of a row, then the next row: the
      // stores of a wavefront are one contiguous run.
      const int qpr = A >> VL, rstep = nt / qpr;
      const int jq = tid % qpr, r0 = tid / qpr;
      if (r0 < rstep) {
        const HipVec<T> a4 = *reinterpret_cast<const HipVec<T>*>(af + V * jq);
        Vec<T>* orow = reinterpret_cast<Vec<T>*>(o) + jq;
        for (int i = r0; i < S; i += rstep) {
          const Vec<T> pk = scaled<T>(sf[i], a4);
          if (check_each) bad |= !all_finite<T>(pk);
          product_store<T>(pk, orow + (int64_t)i * qpr);
        }
      }
    } else if (!kLean && vec) {
      // rows are 16-B aligned (ld_out % V == 0): one 16-byte word per lane
      const int64_t nvec = total >> VL;
      const int step_i = (V * nt) / A, step_j = (V * nt) % A;
      int64_t e = V * (int64_t)tid;
      int i = (int)(e / A), j = (int)(e % A);
      for (int64_t q = tid; q < nvec; q += nt) {
        HipVec<T> v;
        int ii = i, jj = j;
        auto next = [&]() { if (++jj == A) { jj = 0; ++ii; } };
        v.x = sf[ii] * af[jj]; next();
        if constexpr (V == 4) {
          v.y = sf[ii] * af[jj]; next();
          v.z = sf[ii] * af[jj]; next();
          v.w = sf[ii] * af[jj];
        } else {
          v.y = sf[ii] * af[jj];
        }
        if constexpr (V == 4) {   // (all_finite, spelled out: through the call the fp32 loop's instructions reorder)
          if (check_each) bad |= !(isfinite(v.x) && isfinite(v.y) && isfinite(v.z) && isfinite(v.w));
        } else {
          if (check_each) bad |= !(isfinite(v.x) && isfinite(v.y));
        }
        const Vec<T> pk = pack<T>(v);
        // (one 16-byte streaming store; four 4-byte ones run at the same 4.4 TB/s, cached stores at 4.1)
        product_store<T>(pk, reinterpret_cast<Vec<T>*>(o + V * q));
        i += step_i; j += step_j;
        if (j >= A) { j -= A; ++i; }
      }
      for (int64_t e2 = (nvec << VL) + tid; e2 < total; e2 += nt) {
        const T v = sf[e2 / A] * af[e2 % A];
        bad |= !isfinite(v);
        o[e2] = v;
      }
    } else {
      const int step_i = nt / A, step_j = nt % A;
      int i = tid / A, j = tid % A;
      for (int64_t e = tid; e < total; e += nt) {
        const T v = sf[i] * af[j];
        bad |= !isfinite(v);
        product_store<T>(v, o + e);
        i += step_i; j += step_j;
        if (j >= A) { j -= A; ++i; }
      }
    }
    if (tid == 0) {
      o[total] = mean;
      o[total + 1] = sdev;
      bad |= !(isfinite(mean) && isfinite(sdev));
    }
    if (bad && nonfinite) atomicOr(nonfinite, 1);
  }
}

// fp32 only.  The materialised summary alone (bsig_crosscorr, vector-width rows, A % 4 == 0): the same arithmetic as
// crosscorr_kernel's quad path in a kernel small enough for 8 workgroups per CU, with every wavefront's 1 KB run of
// stores starting on a 128-byte line.  The kernel is write-bound and its rows (4 (S A + 2) bytes, padded to 16)
// start at arbitrary 16-byte offsets: streaming stores that straddle lines ran at 4.0-4.4 TB/s where the same bytes
// in line-aligned runs take 5.2 (tools/micro/fill_bench.hip, profiles/r03_fill_bench.txt).  So the thread <-> quad
// map is rotated per trajectory by the row's offset within a line: thread t owns quads shift + t + k * act of the
// row (act = rstep * A/4 threads store per sweep, a multiple of 8 quads = 128 bytes); the up to seven quads in
// front of the first line boundary are stored by threads 0..shift-1 on the side.
template <typename T>
__global__ __launch_bounds__(256) void crosscorr_quads_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, T* __restrict__ out,
    int64_t n, int ts, int ta, int sd, int ad, int w, int use_diff, int64_t ld_out, int rstep,
    int32_t* __restrict__ nonfinite) {
  static_assert(kF32<T>, "the quads, their lines and the rotation are counted in floats");
  extern __shared__ __attribute__((aligned(16))) unsigned char summaries_smem[];
  const int sfeat = sd - 1;
  const int S = w * sfeat, A = w * ad;
  T* sf = reinterpret_cast<T*>(summaries_smem);   // [S]
  T* af = sf + S;                                  // [A]
  const int tid = threadIdx.x, ln = tid & 63;
  const int qpr = A >> 2, act = rstep * qpr;
  constexpr int kPfW = 10;
  T pf_s0[kPfW], pf_s1[kPfW], pf_a[kPfW];
  auto prefetch = [&](int64_t traj) {     // (see crosscorr_kernel)
    const T* s = states + traj * (int64_t)ts * sd;
    const T* a = actions + traj * (int64_t)ta * ad;
#pragma unroll
    for (int t = 0; t < kPfW; ++t) {
      if (t < w) {
        const T* srow = s + (int64_t)t * sd;
        const T* arow = a + (int64_t)min(t, ta - 1) * ad;
        if (tid < sfeat) { pf_s0[t] = srow[tid]; pf_s1[t] = use_diff ? srow[tid + 1] : 0.f; }
        if (tid < ad) pf_a[t] = arow[tid];
      }
    }
  };
  if ((int64_t)blockIdx.x < n) prefetch(blockIdx.x);
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    __syncthreads();
#pragma unroll
    for (int t = 0; t < kPfW; ++t) {
      if (t < w) {
        if (tid < sfeat) sf[t * sfeat + tid] = use_diff ? pf_s1[t] - pf_s0[t] : pf_s0[t];
        if (tid < ad) af[t * ad + tid] = pf_a[t];
      }
    }
    __syncthreads();
    if (traj + gridDim.x < n) prefetch(traj + gridDim.x);
    T mean, sdev;
    row_mean_std(sf, S, ln, mean, sdev);
    T ms = 0.f, ma = 0.f;
    bool bad = false;
    for (int i = ln; i < S; i += 64) { ms = fmaxf(ms, fabsf(sf[i])); bad |= !isfinite(sf[i]); }
    for (int i = ln; i < A; i += 64) { ma = fmaxf(ma, fabsf(af[i])); bad |= !isfinite(af[i]); }
    ms = wave_max(ms); ma = wave_max(ma);
    const bool check_each = !(ms < 1e18f && ma < 1e18f);   // (see crosscorr_kernel)
    const int64_t base_q = (traj * ld_out) >> 2;
    Vec<T>* o4 = reinterpret_cast<Vec<T>*>(out) + base_q;
    const int shift = (int)((8 - (base_q & 7)) & 7);
    if (tid < shift) {                       // quads in front of the first line boundary
      const int i = tid / qpr, jq = tid - i * qpr;
      const Vec<T> pk = scaled<T>(sf[i], *reinterpret_cast<const HipVec<T>*>(af + 4 * jq));
      if (check_each) bad |= !all_finite<T>(pk);
      o4[tid] = pk;
    }
    if (tid < act) {
      const int q0 = shift + tid;
      const int i0 = q0 / qpr, jq = q0 - i0 * qpr;
      const HipVec<T> a4 = *reinterpret_cast<const HipVec<T>*>(af + 4 * jq);
      Vec<T>* orow = o4 + jq;
      for (int i = i0; i < S; i += rstep) {
        const Vec<T> pk = scaled<T>(sf[i], a4);
        if (check_each) bad |= !all_finite<T>(pk);
        __builtin_nontemporal_store(pk, orow + (int64_t)i * qpr);
      }
    }
    if (tid == 0) {
      T* o = out + traj * ld_out;
      o[(int64_t)S * A] = mean;
      o[(int64_t)S * A + 1] = sdev;
      bad |= !(isfinite(mean) && isfinite(sdev));
    }
    if (bad && nonfinite) atomicOr(nonfinite, 1);
  }
}

// fp32 only.  Small summaries (Cartpole: 302 floats): one wavefront per trajectory, four
// per workgroup, so a launch still covers the chip with lane-contiguous stores.
template <typename T>
__global__ __launch_bounds__(256) void crosscorr_wave_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, T* __restrict__ out, int64_t n, int ts, int ta,
    int sd, int ad, int w, int use_diff, int64_t ld_out, int32_t* __restrict__ nonfinite,
    T* __restrict__ fac, int64_t ld_fac) {
  static_assert(kF32<T>, "launched with the LDS of four trajectories of floats");
  extern __shared__ __attribute__((aligned(16))) unsigned char summaries_smem[];
  const int sfeat = sd - 1;
  const int S = w * sfeat, A = w * ad;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  T* sf = reinterpret_cast<T*>(summaries_smem) + wid * (S + A);
  T* af = sf + S;
  for (int64_t base = (int64_t)blockIdx.x * 4; base < n; base += (int64_t)gridDim.x * 4) {
    const int64_t traj = base + wid;
    const bool active = traj < n;
    __syncthreads();
    if (active) {
      const T* s = states + traj * (int64_t)ts * sd;
      const T* a = actions + traj * (int64_t)ta * ad;
      for (int e = lane; e < S; e += 64) {
        const int t = e / sfeat, c = e - t * sfeat;
        const T* srow = s + (int64_t)t * sd;
        sf[e] = use_diff ? (srow[c + 1] - srow[c]) : srow[c];
      }
      for (int e = lane; e < A; e += 64) {
        const int t = e / ad, c = e - t * ad;
        af[e] = a[(int64_t)min(t, ta - 1) * ad + c];
      }
    }
    __syncthreads();
    if (!active) continue;
    // (the statistics of every other path: an fp32 sum of squares overflows from |sf| ~ 1e19)
    T mean, sdev;
    row_mean_std(sf, S, lane, mean, sdev);
    if (fac) {
      T* f = fac + traj * ld_fac;
      for (int i = lane; i < S + A; i += 64) f[i] = sf[i];     // af follows sf in LDS
      for (int i = S + A + lane; i < ld_fac; i += 64)
        f[i] = i == S + A ? mean : (i == S + A + 1 ? sdev : (i == S + A + 2 ? 1.0f : 0.f));
    }
    if (!out) {   // factors only: a non-finite product needs a non-finite or overflowing pair
      T ms = 0.f, ma = 0.f;
      bool in_bad = false;
      for (int i = lane; i < S; i += 64) { ms = fmaxf(ms, fabsf(sf[i])); in_bad |= !isfinite(sf[i]); }
      for (int i = lane; i < A; i += 64) { ma = fmaxf(ma, fabsf(af[i])); in_bad |= !isfinite(af[i]); }
      ms = wave_max(ms); ma = wave_max(ma);
      if (nonfinite && (in_bad || !(isfinite(ms * ma) && isfinite(mean) && isfinite(sdev))))
        atomicOr(nonfinite, 1);
      continue;
    }
    T* o = out + traj * ld_out;
    const int total = S * A;
    bool bad = false;
    const int step_i = 64 / A, step_j = 64 % A;
    int i = lane / A, j = lane % A;
    for (int e = lane; e < total; e += 64) {
      const T v = sf[i] * af[j];
      bad |= !isfinite(v);
      o[e] = v;
      i += step_i; j += step_j;
      if (j >= A) { j -= A; ++i; }
    }
    if (lane == 0) {
      o[total] = mean;
      o[total + 1] = sdev;
      bad |= !(isfinite(mean) && isfinite(sdev));
    }
    if (bad && nonfinite) atomicOr(nonfinite, 1);
  }
}

// ------------------------------------------------------------------ K3
// summary_signatory: summarizers.py:144-168.  Path X_l = [l+1 | s_l | a_l] (:152-155), signature levels 1..depth in
// signatory's layout.  Chen's identity per segment, Horner form:
//   S3[i,j,k] += (S2[i,j] + (S1[i] + D[i]/3) * D[j]/2) * D[k]
//   S2[i,j]   += (S1[i] + D[i]/2) * D[j]
//   S1[i]      = X_l[i] - X_0[i]
// One thread per (i,j) pair keeps S2[i,j] and the S3[i,j,:] row in registers for the whole path (every index a
// compile-time constant, so the row never goes to scratch); the result is staged in LDS and stored lane-contiguous
// (straight from the registers -- 16 bytes per lane at a stride of 4 d bytes -- the same stores ran at 2.4 instead
// of 4.0 TB/s: a wavefront's store instruction wants one contiguous run).
// LDS: path [L d] | increments [(L-1) dp], rows zero-padded to dp = d rounded up to kVec | stage [d^3].
// sizeof(T)*(L*d + d + d^2 + d^3) B / trajectory.  (double: d <= 22, one pair per thread of at most 512)
template <typename T, int DMAX>
__global__ __launch_bounds__(kF32<T> ? 1024 : 512) void signature3_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, T* __restrict__ out, int64_t n,
    int length, int sd, int ad, int64_t ld_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char summaries_smem[];
  constexpr int V = kVec<T>, VL = kVecLog<T>;
  const int d = 1 + sd + ad;
  const int dp = (d + V - 1) & ~(V - 1);       // increment rows padded to a 16-byte word
  T* path = reinterpret_cast<T*>(summaries_smem);              // [length * d]
  T* delta = path + ((length * d + V - 1) & ~(V - 1));         // [(length-1) * dp], zero padded
  // level-3 terms are staged at the same offset modulo a 16-byte word as they have in the output row
  // (o + d + d*d): 16-byte chunks are then aligned on both sides.  (double: d (d + 1) is even, no offset)
  const int mis = (d + d * d) & (V - 1);
  T* stage = delta + (length - 1) * dp + mis;    // [d*d*d]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int npairs = d * d;
  const int i = tid / d, j = tid % d;
  const bool active = tid < npairs;
  // the next trajectory's samples are fetched into registers before this one's store phase
  // (one element per thread: their latency hides behind it instead of opening every trajectory)
  const bool pf_ok = length * sd <= nt && length * ad <= nt;
  T pf_s = (T)0, pf_a = (T)0;
  auto prefetch = [&](int64_t traj) {
    if (tid < length * sd) pf_s = states[traj * (int64_t)length * sd + tid];
    if (tid < length * ad) pf_a = actions[traj * (int64_t)length * ad + tid];
  };
  if (pf_ok && (int64_t)blockIdx.x < n) prefetch(blockIdx.x);
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const T* s = states + traj * (int64_t)length * sd;
    const T* a = actions + traj * (int64_t)length * ad;
    T* o = out + traj * ld_out;
    __syncthreads();
    if (pf_ok) {
      if (tid < length * sd) { const int l = tid / sd, c = tid - l * sd; path[l * d + 1 + c] = pf_s; }
      if (tid < length * ad) { const int l = tid / ad, c = tid - l * ad; path[l * d + 1 + sd + c] = pf_a; }
    } else {
      for (int e = tid; e < length * sd; e += nt) {
        const int l = e / sd, c = e - l * sd;
        path[l * d + 1 + c] = s[e];
      }
      for (int e = tid; e < length * ad; e += nt) {
        const int l = e / ad, c = e - l * ad;
        path[l * d + 1 + sd + c] = a[e];
      }
    }
    for (int l = tid; l < length; l += nt) path[l * d] = (T)(l + 1);
    __syncthreads();
    if (pf_ok && traj + gridDim.x < n) prefetch(traj + gridDim.x);
    for (int e = tid; e < (length - 1) * dp; e += nt) {
      const int l = e / dp, c = e - l * dp;
      delta[e] = c < d ? path[(l + 1) * d + c] - path[l * d + c] : (T)0;
    }
    __syncthreads();
    T s2 = (T)0;
    T s3[DMAX];
#pragma unroll
    for (int k = 0; k < DMAX; ++k) s3[k] = (T)0;
    if (active) {
      const T x0i = path[i];
      for (int l = 0; l + 1 < length; ++l) {
        const T* dl = delta + l * dp;
        const T di = dl[i], dj = dl[j];
        const T s1i = path[l * d + i] - x0i;
        const T coef = s2 + (s1i + di * ((T)1 / (T)3)) * dj * (T)0.5;
#pragma unroll
        for (int kv = 0; kv < DMAX / V; ++kv) {        // 16-byte broadcast reads
          if (V * kv < d) {
            const Vec<T> q = *reinterpret_cast<const Vec<T>*>(dl + V * kv);
#pragma unroll
            for (int k = 0; k < V; ++k) s3[V * kv + k] = fma(coef, q[k], s3[V * kv + k]);
          }
        }
        s2 = fma(s1i + di * (T)0.5, dj, s2);
      }
      bool staged = false;
      if constexpr (kF32<T>) {
        if ((d & 1) == 0) {   // 8-byte aligned row of the stage: ds_write_b64
#pragma unroll
          for (int k = 0; k < DMAX; k += 2)
            if (k < d)
              *reinterpret_cast<float2*>(stage + tid * d + k) = make_float2(s3[k], s3[k + 1]);
          staged = true;
        }
      }
      if (!staged) {
#pragma unroll
        for (int k = 0; k < DMAX; ++k)
          if (k < d) stage[tid * d + k] = s3[k];
      }
      o[d + tid] = s2;                                   // level 2
    }
    for (int c = tid; c < d; c += nt)                    // level 1
      o[c] = path[(length - 1) * d + c] - path[c];
    __syncthreads();
    T* o3 = o + d + npairs;
    const int n3 = npairs * d;
    if ((ld_out & (V - 1)) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
      // head up to the first 128-byte LINE of the output row (a wavefront's 64 words are then whole
      // lines: streaming stores that straddle lines run at 4.0-4.4 TB/s, line-aligned runs at 5.2,
      // tools/micro/fill_bench.hip), aligned words, tail.  (head = (V - mis) mod V: the stage has
      // the row's 16-byte phase)
      constexpr int kLine = 128 / (int)sizeof(T);
      const int head =
          min((int)((kLine - ((reinterpret_cast<uintptr_t>(o3) / sizeof(T)) & (kLine - 1))) & (kLine - 1)), n3);
      const int nq = (n3 - head) >> VL;
      if (tid < head) __builtin_nontemporal_store(stage[tid], o3 + tid);
      const Vec<T>* sq = reinterpret_cast<const Vec<T>*>(stage + head);
      Vec<T>* oq = reinterpret_cast<Vec<T>*>(o3 + head);
      for (int q = tid; q < nq; q += nt) __builtin_nontemporal_store(sq[q], oq + q);
      for (int e = head + V * nq + tid; e < n3; e += nt) __builtin_nontemporal_store(stage[e], o3 + e);
    } else {
      for (int e = tid; e < n3; e += nt) __builtin_nontemporal_store(stage[e], o3 + e);
    }
  }
}

// depth <= 2 for wider paths: S2[i,j] = sum_l (X_l[i]-X_0[i] + D_l[i]/2) D_l[j]
template <typename T>
__global__ __launch_bounds__(256) void signature12_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, T* __restrict__ out, int64_t n, int length,
    int sd, int ad, int depth, int64_t ld_out) {
  extern __shared__ __attribute__((aligned(16))) unsigned char summaries_smem[];
  const int d = 1 + sd + ad;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const T* s = states + traj * (int64_t)length * sd;
    const T* a = actions + traj * (int64_t)length * ad;
    T* o = out + traj * ld_out;
    if (depth == 1) {  // last - first row (time channel: L-1)
      for (int c = tid; c < d; c += nt) {
        T v;
        if (c == 0) v = (T)(length - 1);
        else if (c <= sd) v = s[(int64_t)(length - 1) * sd + c - 1] - s[c - 1];
        else v = a[(int64_t)(length - 1) * ad + c - 1 - sd] - a[c - 1 - sd];
        o[c] = v;
      }
      continue;
    }
    T* path = reinterpret_cast<T*>(summaries_smem);  // [length * d]
    __syncthreads();
    for (int l = 0; l < length; ++l) {
      T* row = path + l * d;
      if (tid == 0) row[0] = (T)(l + 1);
      for (int c = tid; c < sd; c += nt) row[1 + c] = s[(int64_t)l * sd + c];
      for (int c = tid; c < ad; c += nt) row[1 + sd + c] = a[(int64_t)l * ad + c];
    }
    __syncthreads();
    for (int c = tid; c < d; c += nt) o[c] = path[(length - 1) * d + c] - path[c];
    const int n2 = d * d;
    const int step_i = nt / d, step_j = nt % d;
    int i = tid / d, j = tid % d;
    for (int e = tid; e < n2; e += nt) {
      const T x0i = path[i];
      T acc = (T)0;
      for (int l = 0; l + 1 < length; ++l) {
        const T* p0 = path + l * d;
        const T* p1 = p0 + d;
        acc = fma((p0[i] - x0i) + (p1[i] - p0[i]) * (T)0.5, p1[j] - p0[j], acc);
      }
      o[d + e] = acc;
      i += step_i; j += step_j;
      if (j >= d) { j -= d; ++i; }
    }
  }
}

// ------------------------------------------------------------------ the plans
// What a plan takes from the element type.  fp32 launches with up to 150 KB of dynamic LDS as it is, without
// raising the kernels' limit (common.h: raise_lds_limit); double asks for the workgroup's whole LDS, from
// the launches that need it.
struct Precision {
  const char* start; const char* crosscorr; const char* signature;   // the messages' prefixes
  int itemsize;
  int64_t grid_cap;       // workgroups of a launch at most
  size_t lds_cap;         // dynamic LDS of a launch at most,
  bool raise_lds;         // reached by raising the kernel's limit
  bool f32_paths;         // the wave and quads kernels, the factor rows
  int cc_slack;           // elements of LDS a cross-correlation launch asks for beyond S + A
  int sig3_slack;         // ... a depth-3 launch beyond path, increments and stage (fp32: the stage's phase)
  int sig3_dim;           // widest path at depth 3 (fp32: 1024 threads; double: every d of the reference's rule)
};
template <typename T>
constexpr Precision kPrecision =
    kF32<T> ? Precision{"summary_start", "crosscorr", "signature", 4, kSummaryGridCap, 150 * 1024, false, true, 8,
                        4, 32}
            : Precision{"summary_start_f64", "crosscorr_f64", "signature_f64", 8, BSIG_F64_SUMMARY_GRID_CAP,
                        kLdsBytes, true, false, 0, 0, 22};

constexpr int64_t kSmallRow = 2048;   // products of a row the wave kernel (fp32) / the lean kernel (double) takes
inline int crosscorr_window(int t_states, int sd) {
  int w = sd > 50 ? 5 : 10;                       // summarizers.py:96-98
  if (t_states <= w) w = t_states;                // :99 (only crop when longer)
  return w;
}

// The device path of a summarizer launch: the launchers take their kernel, store loop and launch
// shape from these helpers, and bsig_debug_summary_path reports what they pick.
enum SumKernel { kKStart = 0, kKCcWave = 1, kKCcQuads = 2, kKCc = 3, kKSig3 = 4, kKSig12 = 5 };
enum SumStore { kStElem = 0, kStQuad = 1, kStVec4 = 2, kStVec4Tail = 3, kStLine = 4, kStFactors = 5 };
struct SumPath {
  int kernel = 0, store = 0, prefetch = 0, threads = 0;
  size_t lds = 0;
  int grid = 0, rstep = 0, dmax = 0, steps = 0, depth = 0;
  int vec = 0, lean = 0;        // crosscorr_kernel's vec argument and kLean
};

inline int lds_refused(const Precision& P, const char* what, size_t lds) {
  if (P.raise_lds) set_error("%s: %zu B of LDS needed (%zu in a workgroup)", what, lds, P.lds_cap);
  else set_error("%s: %zu B of LDS needed", what, lds);
  return BSIG_EUNSUPPORTED;
}

inline int start_path(const Precision& P, int64_t n, int t_states, int t_actions, int sd, int ad, int max_t,
                      int64_t ld_out, SumPath* p) {
  BSIG_REQUIRE(n >= 0 && t_states >= 1 && t_actions >= 1 && sd >= 1 && ad >= 1 && max_t >= 1,
               "%s: bad dims n=%lld ts=%d ta=%d sd=%d ad=%d max_t=%d", P.start,
               (long long)n, t_states, t_actions, sd, ad, max_t);
  BSIG_REQUIRE(ld_out >= (int64_t)max_t * (sd + ad), "%s: ld_out too small", P.start);
  const int width = sd + ad;
  p->kernel = kKStart;
  p->store = kStElem;
  p->threads = width >= 192 ? 256 : (width >= 96 ? 128 : 64);
  p->grid = capped_grid(n, P.grid_cap);
  p->steps = max_t;
  return BSIG_OK;
}

// the materialised summary (has_out), its factors (has_fac), or both
inline int crosscorr_path(const Precision& P, int64_t n, int t_states, int t_actions, int sd, int ad,
                          bool has_out, int64_t ld_out, bool out_align16, bool has_fac, int64_t ld_fac,
                          SumPath* p) {
  const char* what = P.crosscorr;
  BSIG_REQUIRE(n >= 0 && sd >= 2 && ad >= 1, "%s: bad dims sd=%d ad=%d", what, sd, ad);
  BSIG_REQUIRE(t_states > 1, "%s: traj_len must be > 1 (summarizers.py:94)", what);
  BSIG_REQUIRE(t_actions >= 1, "%s: no actions", what);
  const int w = crosscorr_window(t_states, sd);
  const int64_t S = (int64_t)w * (sd - 1), A = (int64_t)w * ad;
  BSIG_REQUIRE(!has_out || ld_out >= S * A + 2, "%s: ld_out too small", what);
  BSIG_REQUIRE(!has_fac || ld_fac >= S + A + 3, "%s: ld_factors too small (need S + A + 3 = %lld)", what,
               (long long)(S + A + 3));
  const int V = 16 / P.itemsize;
  const size_t lds = (size_t)(S + A + P.cc_slack) * P.itemsize;
  if (lds > P.lds_cap) {
    set_error("%s: %zu B of LDS needed", what, lds);
    return BSIG_EUNSUPPORTED;
  }
  p->steps = w;
  p->threads = 256;
  const bool small = S * A <= kSmallRow;
  if (P.f32_paths && small && (S + A) * 4 * sizeof(float) <= 32 * 1024) {
    p->kernel = kKCcWave;
    p->store = has_out ? kStElem : kStFactors;
    p->lds = (size_t)(S + A) * 4 * sizeof(float);
    p->grid = (int)std::min<int64_t>(ceil_div<int64_t>(n, 4), 65536);
    return BSIG_OK;
  }
  p->lds = lds;
  p->grid = capped_grid(n, P.grid_cap);
  p->vec = has_out && (ld_out % V == 0) && out_align16;
  const int qpr = (int)(A / V);
  // the materialised summary alone, quads of action features: the lean streaming kernel
  if (P.f32_paths && has_out && !has_fac && p->vec && (A & 3) == 0 && sd - 1 <= 256 && ad <= 256 && w <= 10 &&
      getenv("BSIG_CC_GENERAL") == nullptr) {
    int m8 = 8; for (int g = qpr; (g & 1) == 0 && m8 > 1; g >>= 1) m8 >>= 1;   // 8 / gcd(qpr, 8)
    const int rstep = (256 / qpr) / m8 * m8;
    if (rstep >= 1 && S * qpr >= 512) {
      p->kernel = kKCcQuads;
      p->store = kStQuad;
      p->prefetch = 1;
      p->rstep = rstep;
      return BSIG_OK;
    }
  }
  // crosscorr_kernel at 256 threads: its pf_ok and the store loop its arguments select
  p->kernel = kKCc;
  p->lean = !P.f32_paths && small;     // (double has no wave kernel: its small rows take the element loop, as ever)
  if (p->lean) p->vec = 0;
  p->prefetch = !p->lean && sd - 1 <= 256 && ad <= 256 && w <= 10;
  if (!has_out) {
    p->store = kStFactors;
  } else if (p->vec && A % V == 0 && A <= V * 256) {
    p->store = kStQuad;
    p->rstep = 256 / qpr;
  } else if (p->vec) {
    p->store = (S * A) % V ? kStVec4Tail : kStVec4;
  } else {
    p->store = kStElem;
  }
  return BSIG_OK;
}

inline int signature_path(const Precision& P, int64_t n, int length, int sd, int ad, int depth,
                          int64_t ld_out, bool out_align16, SumPath* p) {
  const char* what = P.signature;
  BSIG_REQUIRE(n >= 0 && length >= 2 && sd >= 1 && ad >= 1, "%s: bad dims length=%d sd=%d ad=%d", what,
               length, sd, ad);
  const int d = 1 + sd + ad;
  if (depth <= 0) depth = ref_signature_depth(d);
  BSIG_REQUIRE(depth >= 1 && depth <= 3, "%s: depth %d not in 1..3", what, depth);
  BSIG_REQUIRE(ld_out >= bsig_summary_dim(3, length, sd, ad, depth), "%s: ld_out too small", what);
  p->depth = depth;
  p->steps = length;
  p->grid = capped_grid(n, P.grid_cap);
  if (depth == 3) {
    if (d > P.sig3_dim) {
      set_error("%s: depth 3 needs path dim <= %d (got %d)", what, P.sig3_dim, d);
      return BSIG_EUNSUPPORTED;
    }
    const int64_t V = 16 / P.itemsize;
    const size_t lds = (size_t)(round_up<int64_t>((int64_t)length * d, V) + (length - 1) * round_up<int64_t>(d, V) +
                                (int64_t)d * d * d + P.sig3_slack) * P.itemsize;
    if (lds > P.lds_cap) return lds_refused(P, what, lds);
    p->kernel = kKSig3;
    p->lds = lds;
    p->threads = (int)round_up<int64_t>((int64_t)d * d, 64);
    p->dmax = d <= 8 ? 8 : (d <= 16 ? 16 : (d <= 24 ? 24 : 32));
    p->prefetch = length * sd <= p->threads && length * ad <= p->threads;   // signature3_kernel's pf_ok
    p->store = ld_out % V == 0 && out_align16 ? kStLine : kStElem;
    return BSIG_OK;
  }
  size_t lds = 0;
  if (depth == 2) {
    lds = (size_t)length * d * P.itemsize;
    if (lds > P.lds_cap) return lds_refused(P, what, lds);
  }
  p->kernel = kKSig12;
  p->store = kStElem;
  p->lds = lds;
  p->threads = 256;
  return BSIG_OK;
}

// ------------------------------------------------------------------ the launches
// (raise_lds_limit; `raised` is the kernel's own, static next to its launch)
template <typename T, typename K>
inline int allow_lds(K kernel, size_t lds, LdsRaised* raised) {
  return kPrecision<T>.raise_lds && lds > kLdsUnraised ? raise_lds_limit(kernel, (int)kLdsBytes, raised) : BSIG_OK;
}

template <typename T>
int run_start(const T* states, const T* actions, T* out, int64_t n, int t_states, int t_actions, int sd,
              int ad, int max_t, int64_t ld_out, bsig_stream_t stream) {
  constexpr Precision P = kPrecision<T>;
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(states && actions && out, "%s: null pointer", P.start);
  SumPath p;
  BSIG_TRY(start_path(P, n, t_states, t_actions, sd, ad, max_t, ld_out, &p));
  hipLaunchKernelGGL((summary_start_kernel<T, 10>), dim3(p.grid), dim3(p.threads), 0, as_stream(stream), states,
                     actions, out, n, t_states, t_actions, sd, ad, max_t, ld_out);
  BSIG_CHECK_LAUNCH(P.start);
  return BSIG_OK;
}

// the materialised summary (`out`), its factors (`fac`: fp32), or both
template <typename T>
int run_crosscorr(const T* states, const T* actions, T* out, int64_t ld_out, T* fac, int64_t ld_fac,
                  int64_t n, int t_states, int t_actions, int sd, int ad, int use_state_diff,
                  int32_t* nonfinite, bsig_stream_t stream) {
  constexpr Precision P = kPrecision<T>;
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(states && actions && (out || fac), "%s: null pointer", P.crosscorr);
  SumPath p;
  BSIG_TRY(crosscorr_path(P, n, t_states, t_actions, sd, ad, out != nullptr, ld_out, aligned(out, 16),
                          fac != nullptr, ld_fac, &p));
  const hipStream_t st = as_stream(stream);
  const int w = p.steps;
  if constexpr (kF32<T>) {
    if (p.kernel == kKCcWave) {
      hipLaunchKernelGGL(crosscorr_wave_kernel<T>, dim3(p.grid), dim3(p.threads), p.lds, st, states, actions, out,
                         n, t_states, t_actions, sd, ad, w, use_state_diff, ld_out, nonfinite, fac, ld_fac);
      BSIG_CHECK_LAUNCH("crosscorr_wave");
      return BSIG_OK;
    }
    if (p.kernel == kKCcQuads) {
      hipLaunchKernelGGL(crosscorr_quads_kernel<T>, dim3(p.grid), dim3(p.threads), p.lds, st, states, actions, out,
                         n, t_states, t_actions, sd, ad, w, use_state_diff, ld_out, p.rstep, nonfinite);
      BSIG_CHECK_LAUNCH("crosscorr_quads");
      return BSIG_OK;
    }
  }
  const auto kernel = p.lean ? crosscorr_kernel<T, !kF32<T>> : crosscorr_kernel<T, false>;   // (fp32: one kernel)
  static LdsRaised raised[2];
  BSIG_TRY(allow_lds<T>(kernel, p.lds, &raised[p.lean]));
  hipLaunchKernelGGL(kernel, dim3(p.grid), dim3(p.threads), p.lds, st, states, actions, out, n, t_states,
                     t_actions, sd, ad, w, use_state_diff, ld_out, p.vec, nonfinite, fac, ld_fac);
  BSIG_CHECK_LAUNCH(P.crosscorr);
  return BSIG_OK;
}

template <typename T, int DMAX>
int launch_sig3(const SumPath& p, hipStream_t st, const T* states, const T* actions, T* out, int64_t n,
                int length, int sd, int ad, int64_t ld_out) {
  static LdsRaised raised;
  BSIG_TRY(allow_lds<T>(signature3_kernel<T, DMAX>, p.lds, &raised));
  hipLaunchKernelGGL((signature3_kernel<T, DMAX>), dim3(p.grid), dim3(p.threads), p.lds, st, states, actions,
                     out, n, length, sd, ad, ld_out);
  BSIG_CHECK_LAUNCH(kPrecision<T>.signature);
  return BSIG_OK;
}

template <typename T>
int run_signature(const T* states, const T* actions, T* out, int64_t n, int length, int sd, int ad,
                  int depth, int64_t ld_out, bsig_stream_t stream) {
  constexpr Precision P = kPrecision<T>;
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(states && actions && out, "%s: null pointer", P.signature);
  SumPath p;
  BSIG_TRY(signature_path(P, n, length, sd, ad, depth, ld_out, aligned(out, 16), &p));
  const hipStream_t st = as_stream(stream);
  if (p.kernel == kKSig12) {
    static LdsRaised raised;
    BSIG_TRY(allow_lds<T>(signature12_kernel<T>, p.lds, &raised));
    hipLaunchKernelGGL(signature12_kernel<T>, dim3(p.grid), dim3(p.threads), p.lds, st, states, actions, out,
                       n, length, sd, ad, p.depth, ld_out);
    BSIG_CHECK_LAUNCH(P.signature);
    return BSIG_OK;
  }
  if (p.dmax == 8) return launch_sig3<T, 8>(p, st, states, actions, out, n, length, sd, ad, ld_out);
  if (p.dmax == 16) return launch_sig3<T, 16>(p, st, states, actions, out, n, length, sd, ad, ld_out);
  if constexpr (kF32<T>) {          // (double: sig3_dim is below 24)
    if (p.dmax == 32) return launch_sig3<T, 32>(p, st, states, actions, out, n, length, sd, ad, ld_out);
  }
  return launch_sig3<T, 24>(p, st, states, actions, out, n, length, sd, ad, ld_out);
}

}  // namespace summaries
}  // namespace bsig
