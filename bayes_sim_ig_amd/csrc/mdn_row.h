// The mixture-density head's component row, once, for fp32 and double: "a thread runs component k of a row" -- mixture
// weights, forward substitution with T_k = diag(sigma_k) + strict lower (mdnn.py:152-158), log-density and its clamps,
// the row's logsumexp, back substitution and every gradient (closed forms: SURVEY.md Appendix A.1-A.3, from
// mdnn.py:108-178).  Its callers: mdn_nll_kernel<FULL> (mdn_head.hip: thread (r, k), row in an LDS tile),
// full_row (head_device.h: lane k of a persistent owner's wavefront) and mdn_nll_f64_kernel<FULL>
// (f64/mdn_head_f64.hip: lane k, row in global memory).  The forward() tuple kernel sits here too, for both precisions.
//
// The body comes in four phases, because a wait or a cross-lane step of the caller's sits between them: comp_weights,
// comp_elements, row_lse, comp_backward.  They see the row through a RowView; which of its optional scratch planes a
// caller has (VP: v, E0: exp(pre)) is a template argument of the phases, so that no lane tests a pointer per element.
//
// Contraction of multiplies and adds is OFF in every function here and the fused operations are written out
// (fma_): the bits of a row must not depend on which kernel the body is inlined into.  The choices are those the
// compiler made for the per-phase kernels before the body was shared (profiles/head_body_NOTES.md).
#pragma once
#include <type_traits>

#include "common.h"
#include "fit_protocol.h"

namespace bsig {
namespace mdn {

template <typename T> constexpr bool kF32 = std::is_same<T, float>::value;
template <typename T> constexpr T kHalfLog2Pi = kF32<T> ? (T)0.91893853320467274178f : (T)0.91893853320467274178;

__device__ __forceinline__ float fma_(float a, float b, float c) { return __builtin_fmaf(a, b, c); }
__device__ __forceinline__ double fma_(double a, double b, double c) { return __builtin_fma(a, b, c); }
template <typename T>
__device__ __forceinline__ T clamp(T v, T lo, T hi) { return fmin(fmax(v, lo), hi); }

// the jitter draw u ~ U[0, 1) (mdnn.py:116) of the flat element e = (row * D + d) * K + k: injected, or 24 bits of
// word 0 of Philox at counter e (exact in fp32, widened for double)
template <typename T>
__device__ __forceinline__ T jitter_u(const T* noise, uint64_t seed, uint64_t sid, int64_t e) {
  if (noise) return noise[e];
  return (T)u01(philox4x32_10(seed, sid, (uint64_t)e).v[0]);
}

// ---- mixture weights: softmax -> clamp -> renormalise (mdnn.py:109-111) ------------------------------------
template <typename T>
struct MixNorm { T mx, den, csum; };   // max logit, sum exp(logit - mx), sum of the clamped softmax
template <typename T>
__device__ __forceinline__ MixNorm<T> mix_norm(const T* lg, int K, T min_w) {
#pragma clang fp contract(off)
  MixNorm<T> m;
  m.mx = lg[0];
  for (int j = 1; j < K; ++j) m.mx = fmax(m.mx, lg[j]);
  m.den = (T)0;
  for (int j = 0; j < K; ++j) m.den += exp(lg[j] - m.mx);
  m.csum = (T)0;
  for (int j = 0; j < K; ++j) m.csum += clamp(exp(lg[j] - m.mx) / m.den, min_w, (T)1);
  return m;
}
template <typename T>
__device__ __forceinline__ T mix_softmax(const MixNorm<T>& m, T logit) { return exp(logit - m.mx) / m.den; }
template <typename T>
__device__ __forceinline__ T mix_weight(const MixNorm<T>& m, T s, T min_w) { return clamp(s, min_w, (T)1) / m.csum; }

// ---- the row as a component sees it -------------------------------------------------------------------------
template <typename T>
struct RowView {
  const T* lg;              // the row's K logits (or the tuple's weights)
  const T *mu, *sg, *lo;    // this component at d = 0: mean, pre-activation (tuple: sigma), first strict-lower entry
  T *d_mu, *d_sg, *d_lo;    // where the gradients go, laid out like the inputs (an LDS tile: the inputs themselves)
  int es;                   // elements between consecutive d of a component (lower entry (d, j): (d (d-1) / 2 + j) es)
  const T* y;               // the D targets
  T *v, *q; int vs;         // scratch planes at stride vs: T v = y - mu (VP; a diagonal row may have one too: it
                            // saves the backward a division), T^T q = v (FULL)
  T* e0;                    // plane of exp(pre) at stride vs, left for the caller (E0; without: recomputed)
  int64_t je;               // flat jitter element of (row, d = 0, k)
};
template <typename T>
struct RowHyper {
  int D, K; bool tuple;     // tuple: weights and sigma are final (no softmax, no exp, no jitter)
  T min_w, ll_limit, inv_norm;
  const T* noise; uint64_t seed, sid;
};
// what a component carries from one phase to the next
template <typename T>
struct CompState { T w, s; MixNorm<T> m; T logp; bool bad; };

// phase 1: the component's mixture weight
template <typename T>
__device__ __forceinline__ void comp_weights(const RowView<T>& r, const RowHyper<T>& h, int k, CompState<T>& c) {
  c.s = (T)0; c.m = MixNorm<T>{(T)0, (T)1, (T)1}; c.logp = (T)0;
  if (h.tuple) {
    c.w = r.lg[k];
  } else {
    c.m = mix_norm(r.lg, h.K, h.min_w);
    c.s = mix_softmax(c.m, r.lg[k]);
    c.w = mix_weight(c.m, c.s, h.min_w);
  }
  c.bad = !isfinite(c.w);
}

// sigma of element d again (backward): exp(pre) from the caller's plane or recomputed, the same jitter draw
template <typename T, bool E0>
__device__ __forceinline__ T sigma_again(const RowView<T>& r, const RowHyper<T>& h, T eps, int d, T& sg0, T& u) {
#pragma clang fp contract(off)
  u = (T)0;
  if (h.tuple) { sg0 = (T)1; return r.sg[d * r.es]; }
  if constexpr (E0) sg0 = r.e0[d * r.vs];
  else sg0 = exp(r.sg[d * r.es]);
  T sg = sg0;
  if (eps != (T)0) { u = jitter_u(h.noise, h.seed, h.sid, r.je + (int64_t)d * h.K); sg = fma_(u, eps, sg); }
  return sg;
}

// phase 2: sigma with jitter (scale `eps`), substitution, quad, logdet, logp; returns rv = clamp(logp) + log clamp(w)
template <typename T, bool FULL, bool VP = FULL, bool E0 = false>
__device__ __forceinline__ T comp_elements(const RowView<T>& r, const RowHyper<T>& h, T eps, CompState<T>& c) {
#pragma clang fp contract(off)
  T quad = (T)0, logdet = (T)0;
  for (int d = 0; d < h.D; ++d) {
    const T mu = r.mu[d * r.es];
    T sg = r.sg[d * r.es];
    if (!h.tuple) {
      sg = exp(sg);
      if constexpr (E0) r.e0[d * r.vs] = sg;
      if (eps != (T)0) sg = fma_(jitter_u(h.noise, h.seed, h.sid, r.je + (int64_t)d * h.K), eps, sg);
    }
    c.bad |= !(isfinite(mu) && isfinite(sg));
    T res = r.y[d] - mu;
    if (FULL) {   // forward substitution with T = diag(sigma) + strict lower
      const T* lrow = r.lo + (d * (d - 1) / 2) * r.es;
      for (int j = 0; j < d; ++j) {
        const T lij = lrow[j * r.es];
        c.bad |= !isfinite(lij);
        res = fma_(-lij, r.v[j * r.vs], res);
      }
    }
    const T vi = res / sg;
    if constexpr (VP) r.v[d * r.vs] = vi;
    // (the one operation the precisions' compiles disagreed on: fp32 added the rounded square, double fused)
    if constexpr (kF32<T>) quad += vi * vi;
    else quad = fma_(vi, vi, quad);
    logdet += log(sg);
  }
  c.logp = fma_(-(T)h.D, kHalfLog2Pi<T>, fma_((T)-0.5, quad, -logdet));
  const T lp = clamp(c.logp, -h.ll_limit, h.ll_limit);   // mdnn.py:159
  const T wc = clamp(c.w, h.min_w, (T)1);                // mdnn.py:160
  const T rv = lp + log(wc);
  c.bad |= !(isfinite(c.logp) && isfinite(rv));
  return rv;
}

// phase 3: the row's logsumexp over rk[0..K), mdnn.py:163-178
template <typename T>
__device__ __forceinline__ T row_lse(const T* rk, int K) {
#pragma clang fp contract(off)
  T m2 = rk[0];
  for (int j = 1; j < K; ++j) m2 = fmax(m2, rk[j]);
  T se = (T)0;
  for (int j = 0; j < K; ++j) se += exp(rk[j] - m2);
  return m2 + log(se);
}

// phase 4: back substitution, d mu / d sigma / d lower stores (d pre without the jitter-scale term), the lane's
// sum(u * dL/dsigma) added to `uds`; returns the component's logit gradient (tuple: d / d weight), which the caller
// stores once every lane of the row has read the logits
template <typename T, bool FULL, bool VP = FULL, bool E0 = false>
__device__ __forceinline__ T comp_backward(const RowView<T>& r, const RowHyper<T>& h, int k, T eps,
                                           const CompState<T>& c, const T* rk, T lse, T& uds) {
#pragma clang fp contract(off)
  const int D = h.D, K = h.K;
  const T sc = -exp(rk[k] - lse) * h.inv_norm;
  const T g_lp = (c.logp >= -h.ll_limit && c.logp <= h.ll_limit) ? sc : (T)0;
  T sg0, u;
  if (FULL) {   // q = T^{-T} v by back substitution
    for (int i = D - 1; i >= 0; --i) {
      T acc = r.v[i * r.vs];
      for (int j = i + 1; j < D; ++j) acc = fma_(-r.lo[(j * (j - 1) / 2 + i) * r.es], r.q[j * r.vs], acc);
      r.q[i * r.vs] = acc / sigma_again<T, E0>(r, h, eps, i, sg0, u);
    }
  }
  for (int d = 0; d < D; ++d) {
    const T sg = sigma_again<T, E0>(r, h, eps, d, sg0, u);
    T dmu, dsg;
    if (FULL) {
      const T qi = r.q[d * r.vs], vi = r.v[d * r.vs];
      dmu = g_lp * qi;
      dsg = g_lp * fma_(qi, vi, (T)-1 / sg);
      T* drow = r.d_lo + (d * (d - 1) / 2) * r.es;
      for (int j = 0; j < d; ++j) drow[j * r.es] = g_lp * qi * r.v[j * r.vs];
    } else {
      T z;   // (the same bits either way)
      if constexpr (VP) z = r.v[d * r.vs];
      else z = (r.y[d] - r.mu[d * r.es]) / sg;
      dmu = g_lp * z / sg;
      dsg = g_lp * fma_(z, z, (T)-1) / sg;
    }
    uds = fma_(u, dsg, uds);
    r.d_mu[d * r.es] = dmu;
    r.d_sg[d * r.es] = dsg * sg0;
  }
  // mixture-weight path: second clamp, renormalisation, first clamp, softmax
  if (h.tuple) return (c.w >= h.min_w && c.w <= (T)1) ? sc / clamp(c.w, h.min_w, (T)1) : (T)0;
  auto g_w = [&](int j, T& sj, T& wj) {   // d loss / d w_j
    sj = mix_softmax(c.m, r.lg[j]);
    wj = mix_weight(c.m, sj, h.min_w);
    const T scj = -exp(rk[j] - lse) * h.inv_norm;
    return (wj >= h.min_w && wj <= (T)1) ? scj / clamp(wj, h.min_w, (T)1) : (T)0;
  };
  T s1 = (T)0, sj, wj;   // sum_j g_w[j] * w[j]
  for (int j = 0; j < K; ++j) {
    const T gwj = g_w(j, sj, wj);
    s1 = fma_(gwj, wj, s1);
  }
  T s2 = (T)0, gs_k = (T)0;   // sum_j g_s[j] * s[j]
  for (int j = 0; j < K; ++j) {
    const T gcj = (g_w(j, sj, wj) - s1) / c.m.csum;
    const T gsj = (sj >= h.min_w && sj <= (T)1) ? gcj : (T)0;
    s2 = fma_(gsj, sj, s2);
    if (j == k) gs_k = gsj;
  }
  return c.s * (gs_k - s2);
}

// ---- forward() tuple, mdnn.py:109-119 ---------------------------------------------------------------------
// the sum of the exp(pre) partials, each precision in the order it always had: fp32 through the block, double
// serially in every thread
__device__ inline float sig_partials_sum(const float* p, int n) {
  __shared__ float red[8];
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += blockDim.x) s += p[i];
  return block_sum(s, red);
}
__device__ inline double sig_partials_sum(const double* p, int n) {
  double s = 0.0;
  for (int i = 0; i < n; ++i) s += p[i];
  return s;
}

template <typename T>
__global__ __launch_bounds__(256) void mdn_outputs_kernel(
    const T* __restrict__ o, int64_t ld, int batch, int D, int K, int Ls, const T* __restrict__ noise, uint64_t seed,
    uint64_t stream_id, T eps_noise, T min_w, const T* __restrict__ sig_partials, int n_sig, T* __restrict__ weights,
    T* __restrict__ mu, T* __restrict__ l_d, T* __restrict__ lower, int32_t* __restrict__ nonfinite) {
#pragma clang fp contract(off)
  const int DK = D * K, Nh = K + 2 * DK + Ls * K;
  T eps = (T)0;
  if (eps_noise != (T)0) eps = eps_noise * (sig_partials_sum(sig_partials, n_sig) / ((T)batch * (T)DK));
  bool bad = false;
  for (int row = blockIdx.x; row < batch; row += gridDim.x) {
    const T* t = o + (int64_t)row * ld;
    for (int j = threadIdx.x; j < Nh; j += blockDim.x) {
      T v;
      if (j < K) {
        const MixNorm<T> m = mix_norm(t, K, min_w);
        v = mix_weight(m, mix_softmax(m, t[j]), min_w);
        weights[(int64_t)row * K + j] = v;
      } else if (j < K + DK) {
        v = t[j];
        mu[(int64_t)row * DK + (j - K)] = v;
      } else if (j < K + 2 * DK) {
        const int64_t ne = (int64_t)row * DK + (j - K - DK);   // [B, D, K] flat == d*K+k
        v = exp(t[j]);
        if (eps != (T)0) v = fma_(jitter_u(noise, seed, stream_id, ne), eps, v);
        l_d[(int64_t)row * DK + (j - K - DK)] = v;
      } else {
        v = t[j];
        lower[(int64_t)row * Ls * K + (j - K - 2 * DK)] = v;
      }
      bad |= !isfinite(v);
    }
  }
  if (bad && nonfinite) atomicOr(nonfinite, kFlagNonfinite);
}

}  // namespace mdn
}  // namespace bsig
