// The time-lagged cross-correlation summary (include/bsig_xcorr.h) in fp32 (csrc/xcorr.hip) and in
// double (csrc/f64/xcorr_f64.hip) from this one template.
//
// A workgroup of kThreads threads holds G trajectories at a time, P = kThreads / G threads each (both
// powers of two, picked on the host from the shape: Plan), and grid-strides over the rest; a trajectory
// that takes more than half a CU's LDS gets kMaxThreads threads.  Per
// trajectory its slot of LDS holds
//   raw / f [ts * sd]   the states as they lie in memory, row t at t * sd; under state_diff the
//                       differences f_t = s_(t+1) - s_t are formed IN PLACE (rows 0..M-1), so a state
//                       is read from memory once and differenced once;
//   a       [M * ad]    the actions, padded with their last step.
// and the workgroup the reciprocals 1/(M - tau), tau = 0..max_lag, then 1/M: made on the host, they
// arrive with the launch arguments (Rcp).
// Threads own outputs.  Output e < C = (max_lag + 1) sd ad is c_tau[i, j] with e = (tau sd + i) ad + j:
// at step t its thread reads f[t sd + (tau sd + i)] and a[t ad + j].  The lanes of a wavefront hold
// consecutive e: consecutive j (consecutive words of a: no conflict), and e / ad = tau sd + i
// consecutive too, every value shared by ad lanes (consecutive words of f, the shared ones broadcast).
// So row-major [t][channel] is conflict-free for both arrays and neither is padded.  From two outputs a
// thread on (Plan::vec) a thread owns kVec consecutive outputs, a 16-byte word of the row: it runs their
// chains in one loop over t, kVec of them in flight (one after the other each step waited for its two
// LDS reads with nothing else to do: cross_terms), and stores them at once.  e in [C, C + sd) is mu_i, [C + sd, C + 2 sd) sigma_i (whose thread
// runs mu's chain again: the same bits), read from the same staged f down a column.
// The in-place differences: a thread owns a (column, run of steps) item and walks down it with the
// state before in a register.  With sd < P a column is cut into P / sd runs so that the threads of the
// trajectory all work; a run's last difference needs the first state of the next run, which that run's
// owner overwrites -- every thread takes its first and that state into registers before a barrier.
// As in crosscorr_kernel a workgroup that fetched its next trajectories only after its stores would
// idle the memory path meanwhile: where a thread's share is at most kPfS states and kPfA actions
// (Plan::prefetch: Pendulum, Ant; not ShadowHand's 42 states a thread) the NEXT trajectories'
// elements are fetched into registers before this one's differences, chains and stores.
// With lengths (include/bsig_ragged.h, kRagged) the same kernel takes M per trajectory: the launch shape and
// the staging are those of ts (the rows beyond a length are in bounds, staged and never read again), the run
// length of the in-place differences and every chain's trip count follow the trajectory's own M, whose
// reciprocals its threads make in LDS, one set per trajectory of the workgroup (Plan: per_traj_rcp); a lag
// with no term gets the reciprocal 0.  The barriers do not depend on a length.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"
#include "ragged.h"
#include "../../include/bsig_ragged.h"

namespace bsig {
namespace xcorr {

constexpr int kThreads = 256;         // of a workgroup that trajectories share, and of most others
constexpr int kMaxThreads = 512;      // of one whose trajectory leaves the CU's LDS to no second workgroup
constexpr int kMinPerTraj = 16;       // threads a trajectory gets at least
constexpr int kPfS = 16, kPfA = 4;    // elements a thread prefetches into registers at most

template <typename T>
struct Rcp {                          // host-made: lag[tau] = 1 / (M - tau), all = 1 / M
  T lag[BSIG_XCORR_MAX_LAG + 1];
  T all;
};

struct Plan {
  int m = 0;               // M: steps of the feature series
  int64_t width = 0;       // outputs of a row
  int per_traj = 0;        // P
  int group = 0;           // G; the workgroup has G * P threads
  int vec = 1;             // outputs a thread stores at once
  int prefetch = 0;
  int slot = 0;            // bytes of LDS of one trajectory; the actions start at off_a
  int off_a = 0;
  size_t lds = 0;          // the workgroup's: the reciprocals (with lengths: of each of the G), then G slots
  int off_slots = 0;
};

inline int64_t row_width(int64_t sd, int64_t ad, int64_t max_lag) {
  if (sd < 1 || ad < 1 || max_lag < 0) return -1;
  if (sd > INT32_MAX || ad > INT32_MAX || max_lag >= INT32_MAX) return -1;
  if (sd * ad > INT32_MAX) return -1;
  const int64_t w = (max_lag + 1) * (sd * ad) + 2 * sd;      // below 2^62
  return w > INT32_MAX ? -1 : w;
}

// The launch shape, or why there is none (the checks every entry point and bsig_xcorr_fits share).
// `per_traj_rcp`: every trajectory of a workgroup has reciprocals of its own (what is covered does not change:
// one trajectory, one set).
inline int plan(const char* what, int ts, int ta, int sd, int ad, int max_lag, int state_diff,
                int itemsize, Plan* p, bool per_traj_rcp = false) {
  BSIG_REQUIRE(ts >= 1, "%s: ts %d below 1", what, ts);
  BSIG_REQUIRE(ta >= 1, "%s: ta %d below 1", what, ta);
  BSIG_REQUIRE(sd >= 1 && ad >= 1, "%s: bad dims sd=%d ad=%d", what, sd, ad);
  const int m = state_diff ? ts - 1 : ts;
  BSIG_REQUIRE(m >= 1, "%s: ts %d leaves no state difference (M = %d)", what, ts, m);
  BSIG_REQUIRE(max_lag >= 0 && max_lag <= m - 1, "%s: max_lag %d outside 0..%d (M - 1)", what, max_lag,
               m - 1);
  const int64_t width = row_width(sd, ad, max_lag);
  BSIG_REQUIRE(width > 0, "%s: the width for sd=%d ad=%d max_lag=%d is past 2^31 - 1", what, sd, ad,
               max_lag);
  if (max_lag > BSIG_XCORR_MAX_LAG) {
    set_error("%s: max_lag %d above %d (the reciprocals of the counts travel with the launch)", what,
              max_lag, BSIG_XCORR_MAX_LAG);
    return BSIG_EUNSUPPORTED;
  }
  auto r16 = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
  const int64_t off_a = r16((int64_t)ts * sd * itemsize);
  const int64_t slot = off_a + r16((int64_t)m * ad * itemsize);
  auto rcp_bytes = [&](int group) { return r16((int64_t)(per_traj_rcp ? group : 1) * (max_lag + 2) * itemsize); };
  int64_t off_slots = rcp_bytes(1);
  if (off_slots + slot > (int64_t)kLdsBytes) {
    set_error("%s: %lld B of LDS needed for one trajectory of %d steps, sd=%d ad=%d (%zu in a workgroup)",
              what, (long long)(off_slots + slot), ts, sd, ad, kLdsBytes);
    return BSIG_EUNSUPPORTED;
  }
  int per_traj = kMinPerTraj;
  while (per_traj < kThreads && per_traj < width) per_traj *= 2;
  int group = kThreads / per_traj;
  while (group > 1 && rcp_bytes(group) + group * slot > (int64_t)kLdsUnraised) group /= 2;
  off_slots = rcp_bytes(group);
  per_traj = kThreads / group;
  // a trajectory beyond half the LDS has the CU to itself: twice the wavefronts to hide its LDS reads behind
  if (group == 1 && 2 * (off_slots + slot) > (int64_t)kLdsBytes) per_traj = kMaxThreads;
  const int vec = 16 / itemsize;
  p->m = m;
  p->width = width;
  p->per_traj = per_traj;
  p->group = group;
  p->vec = width >= 2 * (int64_t)per_traj ? vec : 1;      // (one output a thread or less: nothing to interleave)
  p->prefetch = ceil_div<int64_t>((int64_t)ts * sd, per_traj) <= kPfS &&
                ceil_div<int64_t>((int64_t)m * ad, per_traj) <= kPfA;
  p->slot = (int)slot;
  p->off_a = (int)off_a;
  p->off_slots = (int)off_slots;
  p->lds = (size_t)(off_slots + group * slot);
  return BSIG_OK;
}

template <typename T, int kVec>
struct Pack;
template <typename T>
struct Pack<T, 1> { typedef T type; };
template <>
struct Pack<float, 4> { typedef float type __attribute__((ext_vector_type(4))); };
template <>
struct Pack<double, 2> { typedef double type __attribute__((ext_vector_type(2))); };

// Output e of a trajectory from its staged features (see the head of this file).
template <typename T>
__device__ __forceinline__ T output(const T* f, const T* a, const T* rcp, int e, int sd, int ad, int m,
                                    int max_lag, int n_cross) {
  if (e < n_cross) {
    const int q = e / ad, j = e - q * ad;       // q = tau * sd + i
    const int tau = q / sd;
    const T* fp = f + q;                        // f[(t + tau) sd + i]
    const T* ap = a + j;
    const int cnt = m - tau;
    T acc = (T)0;
    for (int t = 0; t < cnt; ++t) acc = fma(fp[t * sd], ap[t * ad], acc);
    return acc * rcp[tau];
  }
  const int r = e - n_cross;
  const int i = r < sd ? r : r - sd;
  const T* fp = f + i;
  const T rm = rcp[max_lag + 1];
  T acc = (T)0;
  for (int t = 0; t < m; ++t) acc += fp[t * sd];
  const T mu = acc * rm;
  if (r < sd) return mu;
  acc = (T)0;
  for (int t = 0; t < m; ++t) {
    const T d = fp[t * sd] - mu;
    acc = fma(d, d, acc);
  }
  return sqrt(acc * rm);
}

// kVec consecutive cross terms e0 .. e0 + kVec - 1 (all below n_cross) in ONE loop over t: kVec independent
// chains in flight, each the chain `output` runs.  Where they share their (tau, i) -- ad a multiple of kVec:
// e0 is one, so they are kVec consecutive j -- a step reads f once and the kVec actions as one 16-byte word.
template <typename T, int kVec>
__device__ __forceinline__ void cross_terms(const T* f, const T* a, const T* rcp, int e0, int sd, int ad, int m,
                                            T (&r)[kVec]) {
  T acc[kVec];
#pragma unroll
  for (int v = 0; v < kVec; ++v) acc[v] = (T)0;
  if constexpr (kVec > 1) {
    if (ad % kVec == 0) {
      const int q = e0 / ad, j = e0 - q * ad;
      const int tau = q / sd, cnt = m - tau;
      const T* fp = f + q;
      const T* ap = a + j;
#pragma unroll 4
      for (int t = 0; t < cnt; ++t) {
        const T fv = fp[t * sd];
        const typename Pack<T, kVec>::type av = *reinterpret_cast<const typename Pack<T, kVec>::type*>(ap + t * ad);
#pragma unroll
        for (int v = 0; v < kVec; ++v) acc[v] = fma(fv, av[v], acc[v]);
      }
      const T rt = rcp[tau];
#pragma unroll
      for (int v = 0; v < kVec; ++v) r[v] = acc[v] * rt;
      return;
    }
  }
  const T* fp[kVec];
  const T* ap[kVec];
  int cnt[kVec], most = 0;
#pragma unroll
  for (int v = 0; v < kVec; ++v) {
    const int q = (e0 + v) / ad, j = e0 + v - q * ad;
    fp[v] = f + q;
    ap[v] = a + j;
    cnt[v] = m - q / sd;
    most = max(most, cnt[v]);
  }
#pragma unroll 4
  for (int t = 0; t < most; ++t) {
#pragma unroll
    for (int v = 0; v < kVec; ++v)
      if (t < cnt[v]) acc[v] = fma(fp[v][t * sd], ap[v][t * ad], acc[v]);
  }
#pragma unroll
  for (int v = 0; v < kVec; ++v) r[v] = acc[v] * rcp[m - cnt[v]];
}

// kVec consecutive statistics r0 .. r0 + kVec - 1 of [mu (sd) | sigma (sd)] in one loop over t per pass (those
// beyond 2 sd - 1 repeat the last one; the caller drops them).
template <typename T, int kVec>
__device__ __forceinline__ void statistics(const T* f, T rm, int r0, int sd, int m, T (&r)[kVec]) {
  const T* fp[kVec];
  bool sig[kVec], any = false;
  T acc[kVec], mu[kVec];
#pragma unroll
  for (int v = 0; v < kVec; ++v) {
    const int rr = min(r0 + v, 2 * sd - 1);
    sig[v] = rr >= sd;
    any |= sig[v];
    fp[v] = f + (sig[v] ? rr - sd : rr);
    acc[v] = (T)0;
  }
#pragma unroll 4
  for (int t = 0; t < m; ++t) {
#pragma unroll
    for (int v = 0; v < kVec; ++v) acc[v] += fp[v][t * sd];
  }
#pragma unroll
  for (int v = 0; v < kVec; ++v) {
    r[v] = mu[v] = acc[v] * rm;
    acc[v] = (T)0;
  }
  if (!any) return;
#pragma unroll 4
  for (int t = 0; t < m; ++t) {
#pragma unroll
    for (int v = 0; v < kVec; ++v) {
      const T d = fp[v][t * sd] - mu[v];
      acc[v] = fma(d, d, acc[v]);
    }
  }
#pragma unroll
  for (int v = 0; v < kVec; ++v)
    if (sig[v]) r[v] = sqrt(acc[v] * rm);
}

// (kBound, the workgroup's size, is a template argument because the bound decides the code: compiled for up to
// kMaxThreads threads the workgroups of kThreads ran Ant 1.1 to 2.1 times as long, profiles/xcorr_NOTES.md)
// (kRagged: `lengths` holds every trajectory's own length and `rc` is not read; else `lengths` is not read)
template <typename T, int kVec, int kBound, bool kRagged>
__global__ __launch_bounds__(kBound) void xcorr_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, const int32_t* __restrict__ lengths,
    T* __restrict__ out, int64_t n, int ts, int ta, int sd, int ad, int max_lag, int state_diff,
    int64_t ld_out, int vec_ok, int32_t* __restrict__ nonfinite, Plan g, Rcp<T> rc) {
  extern __shared__ __attribute__((aligned(16))) unsigned char xcorr_smem[];
  const int tid = threadIdx.x;
  const int P = g.per_traj, G = g.group;
  const int grp = tid / P, lt = tid - grp * P;
  T* rcp = reinterpret_cast<T*>(xcorr_smem) + (kRagged ? grp * (max_lag + 2) : 0);
  T* f = reinterpret_cast<T*>(xcorr_smem + g.off_slots + grp * g.slot);
  T* a = reinterpret_cast<T*>(xcorr_smem + g.off_slots + grp * g.slot + g.off_a);
  // what is staged: the steps of ts, whatever a trajectory's own length
  const int n_s = ts * sd, n_a = g.m * ad, n_a_own = min(ta, g.m) * ad;
  const int n_cross = (max_lag + 1) * sd * ad, width = (int)g.width;
  // the in-place differences: runs per column, steps per run
  const int nseg = sd >= P ? 1 : P / sd;
  // M, and what follows from it: the trajectory's own under kRagged
  int m = g.m, seg_len = ceil_div(m, nseg);
  bool valid = true;

  if constexpr (!kRagged) {
    for (int k = tid; k <= max_lag; k += blockDim.x) rcp[k] = rc.lag[k];
    if (tid == 0) rcp[max_lag + 1] = rc.all;
  }

  // element e of the padded actions of a trajectory: beyond its own steps the last one again
  auto action_at = [&](const T* arow, int e) { return arow[e < n_a_own ? e : (ta - 1) * ad + e % ad]; };
  T pf_s[kPfS], pf_a[kPfA];
  auto prefetch = [&](int64_t traj) {
    const T* s = states + traj * (int64_t)n_s;
    const T* arow = actions + traj * (int64_t)ta * ad;
#pragma unroll
    for (int k = 0; k < kPfS; ++k) {
      const int e = lt + k * P;
      if (e < n_s) pf_s[k] = s[e];
    }
#pragma unroll
    for (int k = 0; k < kPfA; ++k) {
      const int e = lt + k * P;
      if (e < n_a) pf_a[k] = action_at(arow, e);
    }
  };
  const int64_t first = (int64_t)blockIdx.x * G, step = (int64_t)gridDim.x * G;
  if (g.prefetch && first + grp < n) prefetch(first + grp);
  for (int64_t base = first; base < n; base += step) {
    const int64_t traj = base + grp;
    const bool active = traj < n;
    if constexpr (kRagged) {
      // the length is clamped before it indexes anything; one outside the range makes the row NaN below
      const ragged::Steps own = active ? ragged::steps_of(lengths, traj, ts, state_diff) : ragged::Steps{g.m, true};
      m = own.steps;
      valid = own.valid;
      seg_len = ceil_div(m, nseg);
    }
    __syncthreads();          // the reciprocals above / the trajectories before are done with the LDS
    if constexpr (kRagged) {
      // the host's (T)1 / (T)(M - tau) and (T)1 / (T)M, here by the same correctly rounded division; a lag with
      // no term: 0, times its empty chain's 0
      for (int k = lt; k <= max_lag; k += P) rcp[k] = k < m ? (T)1 / (T)(m - k) : (T)0;
      if (lt == 0) rcp[max_lag + 1] = (T)1 / (T)m;
    }
    if (active) {
      if (g.prefetch) {
#pragma unroll
        for (int k = 0; k < kPfS; ++k) {
          const int e = lt + k * P;
          if (e < n_s) f[e] = pf_s[k];
        }
#pragma unroll
        for (int k = 0; k < kPfA; ++k) {
          const int e = lt + k * P;
          if (e < n_a) a[e] = pf_a[k];
        }
      } else {
        const T* s = states + traj * (int64_t)n_s;
        const T* arow = actions + traj * (int64_t)ta * ad;
        for (int e = lt; e < n_s; e += P) f[e] = s[e];
        for (int e = lt; e < n_a; e += P) a[e] = action_at(arow, e);
      }
    }
    __syncthreads();
    if (g.prefetch && traj + step < n) prefetch(traj + step);
    if (state_diff) {
      if (nseg == 1) {        // a thread walks whole columns: nobody else touches them
        if (active) {
          for (int c = lt; c < sd; c += P) {
            T prev = f[c];
            for (int t = 0; t < m; ++t) {
              const T nx = f[(t + 1) * sd + c];
              f[t * sd + c] = nx - prev;
              prev = nx;
            }
          }
        }
      } else {                // one (column, run) a thread; the state behind the run before the barrier
        const int seg = lt / sd, c = lt - seg * sd;
        const int t0 = min(seg * seg_len, m), t1 = min(t0 + seg_len, m);
        const bool own = active && seg < nseg && t0 < t1;
        T prev = (T)0, last = (T)0;
        if (own) {
          prev = f[t0 * sd + c];
          last = f[t1 * sd + c];
        }
        __syncthreads();
        if (own) {
          for (int t = t0; t < t1; ++t) {
            const T nx = t + 1 < t1 ? f[(t + 1) * sd + c] : last;
            f[t * sd + c] = nx - prev;
            prev = nx;
          }
        }
      }
      __syncthreads();
    }
    if (!active) continue;
    T* o = out + traj * ld_out;
    bool bad = false;
    for (int e0 = lt * kVec; e0 < width; e0 += P * kVec) {
      T r[kVec];
      if (e0 + kVec <= n_cross) {
        cross_terms<T, kVec>(f, a, rcp, e0, sd, ad, m, r);
      } else if (e0 >= n_cross) {
        statistics<T, kVec>(f, rcp[max_lag + 1], e0 - n_cross, sd, m, r);
      } else {                // the word that holds the last cross terms and the first means
#pragma unroll
        for (int v = 0; v < kVec; ++v)
          r[v] = e0 + v < width ? output<T>(f, a, rcp, e0 + v, sd, ad, m, max_lag, n_cross) : (T)0;
      }
      if constexpr (kRagged) {
        if (!valid) {
#pragma unroll
          for (int v = 0; v < kVec; ++v) r[v] = (T)NAN;
        }
      }
#pragma unroll
      for (int v = 0; v < kVec; ++v)
        if (e0 + v < width) bad |= !isfinite(r[v]);
      bool stored = false;
      if constexpr (kVec > 1) {
        if (vec_ok && e0 + kVec <= width) {      // one 16-byte store
          typename Pack<T, kVec>::type pk;
#pragma unroll
          for (int v = 0; v < kVec; ++v) pk[v] = r[v];
          *reinterpret_cast<typename Pack<T, kVec>::type*>(o + e0) = pk;
          stored = true;
        }
      }
      if (!stored) {
#pragma unroll
        for (int v = 0; v < kVec; ++v)
          if (e0 + v < width) o[e0 + v] = r[v];
      }
    }
    if (bad && nonfinite) atomicOr(nonfinite, 1);
  }
}

template <typename T, int kVec, int kBound, bool kRagged>
inline int launch(const char* what, int64_t max_grid, const T* states, const T* actions, const int32_t* lengths,
                  T* out, int64_t n, int ts, int ta, int sd, int ad, int max_lag, int state_diff, int64_t ld_out,
                  int32_t* nonfinite, const Plan& g, const Rcp<T>& rc, bsig_stream_t stream) {
  static LdsRaised raised;
  if (g.lds > kLdsUnraised)
    BSIG_TRY(raise_lds_limit(xcorr_kernel<T, kVec, kBound, kRagged>, kLdsBytes, &raised));
  const int vec_ok = ld_out % kVec == 0 && aligned(out, 16);
  hipLaunchKernelGGL((xcorr_kernel<T, kVec, kBound, kRagged>),
                     dim3(capped_grid(ceil_div<int64_t>(n, g.group), max_grid)), dim3(kBound), g.lds,
                     as_stream(stream), states, actions, lengths, out, n, ts, ta, sd, ad, max_lag, state_diff,
                     ld_out, vec_ok, nonfinite, g, rc);
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

// The entry point of either precision, without lengths (bsig_xcorr.h) and with (bsig_ragged.h): the argument
// checks, the plan, the reciprocals (with lengths the kernel makes them per trajectory), the launch.
// `max_grid`: the precision's workgroup cap.
template <typename T, bool kRagged>
int run_any(const char* what, int64_t max_grid, const T* states, const T* actions, const int32_t* lengths, T* out,
            int64_t n, int ts, int ta, int sd, int ad, int max_lag, int state_diff, int64_t ld_out,
            int32_t* nonfinite, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "%s: bad n=%lld", what, (long long)n);
  Plan g;
  BSIG_TRY(plan(what, ts, ta, sd, ad, max_lag, state_diff, (int)sizeof(T), &g, kRagged));
  BSIG_REQUIRE(ld_out >= g.width, "%s: ld_out %lld below the width %lld", what, (long long)ld_out,
               (long long)g.width);
  BSIG_REQUIRE(states && actions && out, "%s: null pointer", what);
  if (kRagged) BSIG_REQUIRE(lengths, "%s: null lengths", what);
  Rcp<T> rc = {};
  if (!kRagged) {
    for (int tau = 0; tau <= BSIG_XCORR_MAX_LAG; ++tau)
      rc.lag[tau] = tau <= max_lag ? (T)1 / (T)(g.m - tau) : (T)0;
    rc.all = (T)1 / (T)g.m;
  }
  constexpr int kWide = 16 / (int)sizeof(T);
#define BSIG_XCORR_LAUNCH(vec, bound)                                                                    \
  launch<T, vec, bound, kRagged>(what, max_grid, states, actions, lengths, out, n, ts, ta, sd, ad, max_lag, \
                                 state_diff, ld_out, nonfinite, g, rc, stream)
  const bool big = g.group * g.per_traj == kMaxThreads;
  if (g.vec == 1) return big ? BSIG_XCORR_LAUNCH(1, kMaxThreads) : BSIG_XCORR_LAUNCH(1, kThreads);
  return big ? BSIG_XCORR_LAUNCH(kWide, kMaxThreads) : BSIG_XCORR_LAUNCH(kWide, kThreads);
#undef BSIG_XCORR_LAUNCH
}

template <typename T>
int run(const char* what, int64_t max_grid, const T* states, const T* actions, T* out, int64_t n, int ts,
        int ta, int sd, int ad, int max_lag, int state_diff, int64_t ld_out, int32_t* nonfinite,
        bsig_stream_t stream) {
  return run_any<T, false>(what, max_grid, states, actions, nullptr, out, n, ts, ta, sd, ad, max_lag, state_diff,
                           ld_out, nonfinite, stream);
}

}  // namespace xcorr
}  // namespace bsig
