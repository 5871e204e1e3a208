// The least-squares dynamics summary (include/bsig_sysid.h) in fp32 (csrc/sysid.hip) and in double
// (csrc/f64/sysid_f64.hip) from this one template.
//
// A workgroup of kThreads threads holds G trajectories at a time, P = kThreads / G threads each (both powers
// of two, picked on the host from the shape: Plan), and grid-strides over the rest.  Per trajectory its slot
// of LDS holds
//   X [ts][ldx]   the rows [1 | s_t | a_t], staged from memory once (ldx = p | 1: odd, so that the dual's walk
//                 down two rows at once and the primal's walk down two columns are both free of bank
//                 conflicts); row M = ts - 1 holds the last state only.  phi_t is row t, and
//                 y_tj = X[t + 1][1 + j] - X[t][1 + j] is formed where it is used, always by that one
//                 subtraction: the same bits every time, and no second copy of the states;
//   K [k][ldk]    k = min(p, M), ldk = k | 1: the lower triangle of G (primal, p <= M) or of Phi Phi^T / M
//                 (dual), then of its Cholesky factor, in place;
//   R [k][sd]     the right-hand sides: B (primal) or Y (dual), then the solution W or alpha, in place;
//   part [nseg][sd]  the primal's sums of squared residuals over runs of steps, added up in ascending order.
// The phases, a barrier between each: stage; the products (a P = tw x th tile of threads over the lower
// triangle, one fma chain an element; a thread an element of R); rho from the trace, on to the diagonal; the
// factorisation, right-looking, column j scaled by threads down it and the trailing triangle updated by the
// tile (two barriers a column); the two triangular solves, a thread a right-hand side, forward then backward
// with no barrier (it owns its column of R; the factor is only read); the stores.
// Primal: W is R; the residuals e_tj = y_tj - phi_t . W_:j are formed from X and R by (run, j) items.
// Dual: W_cj = 1/M sum_t X[t][c] alpha_tj straight to memory, and e_tj = rho alpha_tj.
// A trajectory with a non-finite staged value or a pivot that is not positive and finite stores NaN in every
// element; its arithmetic runs on all the same (no index depends on a value), so the barriers do not depend
// on the data.  Slots beyond n run the phases on what the LDS holds and neither load nor store.
#pragma once
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.h"

namespace bsig {
namespace sysid {

constexpr int kThreads = 256;
constexpr int kMinPerTraj = 16;       // threads a trajectory gets at least

struct Plan {
  int m = 0, p = 0, k = 0;  // steps, regressors, the order of the factorised system
  int dual = 0;
  int64_t width = 0;
  int per_traj = 0, p_log = 0;      // P and its logarithm
  int group = 0;                    // G
  int tw_log = 0;                   // the tile of threads: tw = 1 << tw_log columns, P / tw rows
  int ldx = 0, ldk = 0;
  int nseg = 0, seg_len = 0;        // the primal's runs of steps a column of residuals is cut into
  int off_x = 0, off_k = 0, off_r = 0, off_part = 0, slot = 0;      // bytes; a slot starts with rho
  size_t lds = 0;
};

inline int64_t row_width(int64_t sd, int64_t ad) {
  if (sd < 1 || ad < 1 || sd > INT32_MAX || ad > INT32_MAX) return -1;
  const int64_t w = (1 + sd + ad) * sd + sd;      // below 2^63
  return w > INT32_MAX ? -1 : w;
}

// The launch shape, or why there is none (the checks both entry points and bsig_sysid_fits share).
inline int plan(const char* what, int ts, int ta, int sd, int ad, int itemsize, Plan* g) {
  BSIG_REQUIRE(ts >= 2, "%s: ts %d leaves no step (M = ts - 1 >= 1)", what, ts);
  BSIG_REQUIRE(ta >= 1, "%s: ta %d below 1", what, ta);
  BSIG_REQUIRE(sd >= 1 && ad >= 1, "%s: bad dims sd=%d ad=%d", what, sd, ad);
  const int64_t width = row_width(sd, ad);
  BSIG_REQUIRE(width > 0, "%s: the width for sd=%d ad=%d is past 2^31 - 1", what, sd, ad);
  const int64_t m = ts - 1, p = 1 + (int64_t)sd + ad;
  const int dual = m < p;
  const int64_t k = dual ? m : p;
  const int64_t ldx = p | 1, ldk = k | 1;
  auto r16 = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
  auto slot_bytes = [&](int per_traj, int64_t* off) {
    const int64_t nseg = dual ? 0 : std::max<int64_t>(1, std::min<int64_t>(per_traj / sd, m));
    off[0] = 16;
    off[1] = off[0] + r16(ts * ldx * itemsize);
    off[2] = off[1] + r16(k * ldk * itemsize);
    off[3] = off[2] + r16(k * sd * itemsize);
    return off[3] + r16(nseg * sd * itemsize);
  };
  int64_t off[4];
  const int64_t alone = slot_bytes(kThreads, off);
  if (alone > (int64_t)kLdsBytes) {
    set_error("%s: %lld B of LDS needed for one trajectory of %d states, sd=%d ad=%d (%zu in a workgroup)", what,
              (long long)alone, ts, sd, ad, kLdsBytes);
    return BSIG_EUNSUPPORTED;
  }
  int per_traj = kMinPerTraj;
  while (per_traj < kThreads && 2 * per_traj <= width) per_traj *= 2;
  int group = kThreads / per_traj;
  while (group > 1 && group * slot_bytes(kThreads / group, off) > (int64_t)kLdsUnraised) group /= 2;
  per_traj = kThreads / group;
  const int64_t slot = slot_bytes(per_traj, off);
  g->m = (int)m;
  g->p = (int)p;
  g->k = (int)k;
  g->dual = dual;
  g->width = width;
  g->per_traj = per_traj;
  g->p_log = 0;
  while ((1 << g->p_log) < per_traj) ++g->p_log;
  g->group = group;
  g->tw_log = g->p_log / 2;
  g->ldx = (int)ldx;
  g->ldk = (int)ldk;
  g->nseg = dual ? 0 : (int)std::max<int64_t>(1, std::min<int64_t>(per_traj / sd, m));
  g->seg_len = dual ? 0 : (int)ceil_div<int64_t>(m, g->nseg);
  g->off_x = (int)off[0];
  g->off_k = (int)off[1];
  g->off_r = (int)off[2];
  g->off_part = (int)off[3];
  g->slot = (int)slot;
  g->lds = (size_t)(group * slot);
  return BSIG_OK;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void sysid_kernel(const T* __restrict__ states,
                                                         const T* __restrict__ actions, T* __restrict__ out,
                                                         int64_t n, int ts, int ta, int sd, int ad, T ridge,
                                                         int64_t ld_out, int32_t* __restrict__ nonfinite,
                                                         Plan g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sysid_smem[];
  const int tid = threadIdx.x;
  const int P = g.per_traj, G = g.group;
  const int grp = tid >> g.p_log, lt = tid & (P - 1);
  unsigned char* slot = sysid_smem + (size_t)grp * g.slot;
  T* rho_at = reinterpret_cast<T*>(slot);
  int* flag = reinterpret_cast<int*>(slot + 8);
  T* X = reinterpret_cast<T*>(slot + g.off_x);
  T* K = reinterpret_cast<T*>(slot + g.off_k);
  T* R = reinterpret_cast<T*>(slot + g.off_r);
  T* part = reinterpret_cast<T*>(slot + g.off_part);
  const int M = g.m, p = g.p, k = g.k, ldx = g.ldx, ldk = g.ldk, dual = g.dual;
  const int tw = 1 << g.tw_log, th = P >> g.tw_log;
  const int tc = lt & (tw - 1), ti = lt >> g.tw_log;
  const int n_x = ts * p, n_w = p * sd;
  const T rcp_m = (T)1 / (T)M;

  if (lt == 0) *flag = 0;
  for (int64_t base = (int64_t)blockIdx.x * G; base < n; base += (int64_t)gridDim.x * G) {
    const int64_t traj = base + grp;
    const bool active = traj < n;
    __syncthreads();          // the trajectories before are done with the LDS; the flag is down
    if (active) {
      const T* s = states + traj * ((int64_t)ts * sd);
      const T* a = actions + traj * ((int64_t)ta * ad);
      bool nf = false;
      for (int e = lt; e < n_x; e += P) {
        const int t = e / p, c = e - t * p;
        T v;
        if (c == 0) v = (T)1;
        else if (c <= sd) v = s[t * sd + (c - 1)];
        else if (t < M) v = a[min(t, ta - 1) * ad + (c - 1 - sd)];
        else v = (T)0;        // (the action of the last state enters nothing)
        nf |= !isfinite(v);
        X[t * ldx + c] = v;
      }
      if (nf) *flag = 1;
    }
    __syncthreads();
    bool bad = *flag != 0;

    // ---- the products: the lower triangle of K, then R
    {
      const int len = dual ? p : M, step = dual ? 1 : ldx, lead = dual ? ldx : 1;
      for (int i = ti; i < k; i += th) {
        const T* xi = X + i * lead;
        for (int c = tc; c <= i; c += tw) {
          const T* xc = X + c * lead;
          T acc = (T)0;
#pragma unroll 4
          for (int q = 0; q < len; ++q) acc = fma(xi[q * step], xc[q * step], acc);
          K[i * ldk + c] = acc * rcp_m;
        }
      }
    }
    if (dual) {
      for (int e = lt; e < M * sd; e += P) {
        const int t = e / sd, j = e - t * sd;
        R[e] = X[(t + 1) * ldx + 1 + j] - X[t * ldx + 1 + j];
      }
    } else {
      for (int e = lt; e < n_w; e += P) {
        const int i = e / sd, j = e - i * sd;
        const T* xi = X + i;
        const T* xj = X + 1 + j;
        T acc = (T)0;
#pragma unroll 4
        for (int t = 0; t < M; ++t) acc = fma(xi[t * ldx], xj[(t + 1) * ldx] - xj[t * ldx], acc);
        R[e] = acc * rcp_m;
      }
    }
    __syncthreads();
    if (lt == 0) {
      T trace = (T)0;
      for (int i = 0; i < k; ++i) trace += K[i * ldk + i];
      *rho_at = ridge * trace / (T)p;
      *flag = 0;              // (every thread has read it; the next trajectory's threads raise it after a barrier)
    }
    __syncthreads();
    const T rho = *rho_at;
    for (int i = lt; i < k; i += P) K[i * ldk + i] += rho;

    // ---- K + rho I = L L^T in place; the diagonal keeps the pivots until the end
    for (int j = 0; j < k; ++j) {
      __syncthreads();
      const T d = K[j * ldk + j];
      if (!(d > (T)0) || !isfinite(d)) bad = true;
      const T ljj = sqrt(d);
      for (int i = j + 1 + lt; i < k; i += P) K[i * ldk + j] = K[i * ldk + j] / ljj;
      __syncthreads();
      for (int i = j + 1 + ti; i < k; i += th) {
        const T lij = K[i * ldk + j];
        for (int c = j + 1 + tc; c <= i; c += tw) K[i * ldk + c] = fma(-lij, K[c * ldk + j], K[i * ldk + c]);
      }
    }
    __syncthreads();
    for (int i = lt; i < k; i += P) K[i * ldk + i] = sqrt(K[i * ldk + i]);
    __syncthreads();

    // ---- L z = b, L^T x = z for every right-hand side: a thread owns a column of R
    for (int j = lt; j < sd; j += P) {
      T* rj = R + j;
      for (int i = 0; i < k; ++i) {
        T acc = rj[i * sd];
#pragma unroll 4
        for (int c = 0; c < i; ++c) acc = fma(-K[i * ldk + c], rj[c * sd], acc);
        rj[i * sd] = acc / K[i * ldk + i];
      }
      for (int i = k - 1; i >= 0; --i) {
        T acc = rj[i * sd];
#pragma unroll 4
        for (int c = i + 1; c < k; ++c) acc = fma(-K[c * ldk + i], rj[c * sd], acc);
        rj[i * sd] = acc / K[i * ldk + i];
      }
    }
    __syncthreads();

    // ---- the row
    T* o = out + traj * ld_out;       // (dereferenced by active slots only)
    bool overflow = false;
    if (dual) {
      for (int e = lt; e < n_w; e += P) {
        const int c = e / sd, j = e - c * sd;
        const T* xc = X + c;
        const T* rj = R + j;
        T acc = (T)0;
#pragma unroll 4
        for (int t = 0; t < M; ++t) acc = fma(xc[t * ldx], rj[t * sd], acc);
        const T v = bad ? (T)NAN : acc * rcp_m;
        overflow |= !isfinite(v);
        if (active) o[e] = v;
      }
      for (int j = lt; j < sd; j += P) {
        T acc = (T)0;
        for (int t = 0; t < M; ++t) {
          const T e = rho * R[t * sd + j];
          acc = fma(e, e, acc);
        }
        const T v = bad ? (T)NAN : sqrt(acc * rcp_m);
        overflow |= !isfinite(v);
        if (active) o[n_w + j] = v;
      }
    } else {
      for (int e = lt; e < n_w; e += P) {
        const T v = bad ? (T)NAN : R[e];
        overflow |= !isfinite(v);
        if (active) o[e] = v;
      }
      for (int item = lt; item < g.nseg * sd; item += P) {
        const int seg = item / sd, j = item - seg * sd;
        const int t0 = min(seg * g.seg_len, M), t1 = min(t0 + g.seg_len, M);
        const T* wj = R + j;
        const T* xj = X + 1 + j;
        T acc = (T)0;
        for (int t = t0; t < t1; ++t) {
          const T* xt = X + t * ldx;
          T fit = (T)0;
#pragma unroll 4
          for (int c = 0; c < p; ++c) fit = fma(xt[c], wj[c * sd], fit);
          const T e = (xj[(t + 1) * ldx] - xj[t * ldx]) - fit;
          acc = fma(e, e, acc);
        }
        part[item] = acc;
      }
      __syncthreads();
      for (int j = lt; j < sd; j += P) {
        T acc = (T)0;
        for (int seg = 0; seg < g.nseg; ++seg) acc += part[seg * sd + j];
        const T v = bad ? (T)NAN : sqrt(acc * rcp_m);
        overflow |= !isfinite(v);
        if (active) o[n_w + j] = v;
      }
    }
    if (active && overflow && nonfinite) atomicOr(nonfinite, 1);
  }
}

// The entry point of either precision: the argument checks, the plan, the launch.  `max_grid`: the
// precision's workgroup cap.
template <typename T>
int run(const char* what, int64_t max_grid, const T* states, const T* actions, T* out, int64_t n, int ts, int ta,
        int sd, int ad, double ridge, int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "%s: bad n=%lld", what, (long long)n);
  Plan g;
  BSIG_TRY(plan(what, ts, ta, sd, ad, (int)sizeof(T), &g));
  const T ridge_t = (T)ridge;
  BSIG_REQUIRE(ridge_t > (T)0 && std::isfinite(ridge_t), "%s: ridge %g is not a positive finite number", what,
               ridge);
  BSIG_REQUIRE(ld_out >= g.width, "%s: ld_out %lld below the width %lld", what, (long long)ld_out,
               (long long)g.width);
  BSIG_REQUIRE(states && actions && out, "%s: null pointer", what);
  static LdsRaised raised;
  if (g.lds > kLdsUnraised) BSIG_TRY(raise_lds_limit(sysid_kernel<T>, kLdsBytes, &raised));
  hipLaunchKernelGGL((sysid_kernel<T>), dim3(capped_grid(ceil_div<int64_t>(n, g.group), max_grid)),
                     dim3(kThreads), g.lds, as_stream(stream), states, actions, out, n, ts, ta, sd, ad, ridge_t,
                     ld_out, nonfinite, g);
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

}  // namespace sysid
}  // namespace bsig
