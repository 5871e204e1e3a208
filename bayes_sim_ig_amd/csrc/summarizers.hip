// The fp32 entry points of the start, cross-correlation and signature summaries (csrc/summaries.h), the
// cross-correlation's factor rows and the report of the device path a launch takes.
#include "summaries.h"

using namespace bsig;
using namespace bsig::summaries;

extern "C" int64_t bsig_summary_dim(int kind, int traj_len, int sd, int ad, int depth) {
  if (kind == 0) return 10 * (int64_t)(sd + ad);
  if (kind == 1 || kind == 2) {
    const int w = crosscorr_window(traj_len, sd);
    return (int64_t)w * (sd - 1) * w * ad + 2;
  }
  if (kind == 3) {
    const int64_t d = 1 + sd + ad;
    if (depth <= 0) depth = ref_signature_depth(d);
    int64_t tot = 0, p = 1;
    for (int q = 1; q <= depth; ++q) { p *= d; tot += p; }
    return tot;
  }
  return -1;
}

extern "C" int bsig_summary_start(const float* states, const float* actions, float* out, int64_t n, int t_states,
                                  int t_actions, int sd, int ad, int max_t, int64_t ld_out, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_summary_start");
  return run_start<float>(states, actions, out, n, t_states, t_actions, sd, ad, max_t, ld_out, stream);
}

extern "C" int bsig_crosscorr(const float* states, const float* actions, float* out, int64_t n, int t_states,
                              int t_actions, int sd, int ad, int use_state_diff, int64_t ld_out,
                              int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_crosscorr");
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(out, "crosscorr: null pointer");
  return run_crosscorr<float>(states, actions, out, ld_out, nullptr, 0, n, t_states, t_actions, sd, ad,
                              use_state_diff, nonfinite, stream);
}

extern "C" int bsig_crosscorr_factor_dims(int traj_len, int sd, int ad, int32_t* s_out, int32_t* a_out) {
  BSIG_REQUIRE(traj_len > 1 && sd >= 2 && ad >= 1 && s_out && a_out, "crosscorr_factor_dims: bad args");
  const int w = crosscorr_window(traj_len, sd);
  *s_out = w * (sd - 1);
  *a_out = w * ad;
  return BSIG_OK;
}

extern "C" int bsig_crosscorr_factors(const float* states, const float* actions, float* factors, int64_t n,
                                      int t_states, int t_actions, int sd, int ad, int use_state_diff,
                                      int64_t ld_factors, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_crosscorr_factors");
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(factors, "crosscorr_factors: null pointer");
  return run_crosscorr<float>(states, actions, nullptr, 0, factors, ld_factors, n, t_states, t_actions,
                              sd, ad, use_state_diff, nonfinite, stream);
}

namespace bsig {
// out[r, i*A + j] = sf[i] * af[j], out[r, S*A] = mean, out[r, S*A + 1] = std  from factor rows
__global__ __launch_bounds__(256) void crosscorr_expand_kernel(const float* __restrict__ fac, int64_t ld_fac,
                                                               int64_t n, int S, int A, float* __restrict__ out,
                                                               int64_t ld_out) {
  const int total = S * A;
  for (int64_t r = blockIdx.y; r < n; r += gridDim.y) {
    const float* f = fac + r * ld_fac;
    float* o = out + r * ld_out;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total + 2; e += gridDim.x * blockDim.x) {
      const int i = e / A, j = e - i * A;
      o[e] = e < total ? f[i] * f[S + j] : f[S + A + (e - total)];
    }
  }
}

// bsig_crosscorr_expand's grid for rows of `total` floats
static dim3 expand_grid(int total, int64_t n) {
  return dim3(std::min(ceil_div(total, 256), 64), (unsigned)std::min<int64_t>(n, 16384));
}
}  // namespace bsig

extern "C" int bsig_crosscorr_expand(const float* factors, int64_t ld_factors, int64_t n, int s_dim,
                                     int a_dim, float* out, int64_t ld_out, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(factors && out && n >= 0 && s_dim >= 1 && a_dim >= 1, "crosscorr_expand: bad args");
  BSIG_REQUIRE(ld_factors >= s_dim + a_dim + 3 && ld_out >= (int64_t)s_dim * a_dim + 2,
               "crosscorr_expand: leading dims too small");
  hipLaunchKernelGGL(crosscorr_expand_kernel, expand_grid(s_dim * a_dim + 2, n), dim3(256), 0,
                     as_stream(stream), factors, ld_factors, n, s_dim, a_dim, out, ld_out);
  BSIG_CHECK_LAUNCH("crosscorr_expand");
  return BSIG_OK;
}

extern "C" int bsig_signature(const float* states, const float* actions, float* out, int64_t n, int length,
                              int sd, int ad, int depth, int64_t ld_out, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_signature");
  return run_signature<float>(states, actions, out, n, length, sd, ad, depth, ld_out, stream);
}

extern "C" int bsig_debug_summary_path(int kind, int64_t n, int t_states, int t_actions, int sd,
                                       int ad, int depth, int max_t, int64_t ld_out, int out_align16,
                                       int factors, int32_t* out) {
  BSIG_REQUIRE(out, "summary path: null pointer");
  for (int i = 0; i < 16; ++i) out[i] = 0;
  BSIG_REQUIRE(n >= 1, "summary path: bad n=%lld", (long long)n);
  constexpr Precision P = kPrecision<float>;
  SumPath p;
  dim3 ex(0, 0);
  if (kind == 0) {
    BSIG_TRY(start_path(P, n, t_states, t_actions, sd, ad, max_t, ld_out, &p));
  } else if (kind == 1 || kind == 2) {
    BSIG_TRY(crosscorr_path(P, n, t_states, t_actions, sd, ad, !factors, factors ? 0 : ld_out,
                            out_align16 != 0, factors != 0, factors ? ld_out : 0, &p));
    ex = expand_grid(p.steps * (sd - 1) * p.steps * ad + 2, n);
  } else if (kind == 3) {
    BSIG_TRY(signature_path(P, n, t_states, sd, ad, depth, ld_out, out_align16 != 0, &p));
  } else {
    BSIG_REQUIRE(false, "summary path: bad kind %d", kind);
  }
  out[0] = p.kernel; out[1] = p.store; out[2] = p.prefetch; out[3] = p.threads;
  out[4] = (int32_t)p.lds; out[5] = p.grid; out[6] = p.rstep; out[7] = p.dmax;
  out[8] = p.steps; out[9] = p.depth; out[10] = (int32_t)ex.x; out[11] = (int32_t)ex.y;
  return BSIG_OK;
}
