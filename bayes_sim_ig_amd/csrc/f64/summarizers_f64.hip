// Trajectory summarizers of the fp64 mode (include/bsig_f64.h): bayes_sim_ig/utils/summarizers.py on
// double trajectories, every value a double -- what the reference's torch ops give under
// torch.set_default_dtype(torch.float64).  One straightforward kernel per summarizer, one workgroup
// per trajectory, grid-strided; none of the store variants of csrc/summarizers.hip (nothing here is
// tuned).  Reference file:line cited per kernel.
#include "f64.h"

#include <algorithm>

namespace bsig {
namespace f64 {

// ------------------------------------------------------------------ K1
// summary_start / summary_waypts: summarizers.py:65-87 after the crop/pad of :20-62.
//   out[n, t*(sd+ad)+c] = c<sd ? s[n,min(t,Ts-1),c] : a[n,min(t,Ta-1),c-sd]
__global__ __launch_bounds__(256) void summary_start_f64_kernel(
    const double* __restrict__ states, const double* __restrict__ actions, double* __restrict__ out,
    int64_t n, int ts, int ta, int sd, int ad, int w, int64_t ld_out) {
  const int width = sd + ad;
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const double* s = states + traj * (int64_t)ts * sd;
    const double* a = actions + traj * (int64_t)ta * ad;
    double* o = out + traj * ld_out;
    for (int t = 0; t < w; ++t) {
      const double* srow = s + (int64_t)min(t, ts - 1) * sd;
      const double* arow = a + (int64_t)min(t, ta - 1) * ad;
      for (int c = threadIdx.x; c < width; c += blockDim.x)
        o[(int64_t)t * width + c] = c < sd ? srow[c] : arow[c - sd];
    }
  }
}

// ------------------------------------------------------------------ K2
// cross_correlation: summarizers.py:90-122, the waypoints of csrc/summarizers.hip (the first w steps).
//   sf[t*(sd-1)+c] = s[t,c+1]-s[t,c]  (corrdiff, :105-106: ONE subtraction)  or  s[t,c] (:108)
//   af[t*ad+c]     = a[min(t,Ta-1),c]
//   out[i*A + j]   = sf[i]*af[j]      (:112-113: ONE multiply, stored as it is -- there is no sum
//                                      next to it that a contraction could fold it into)
//   out[S*A]       = mean(sf), out[S*A+1] = unbiased std(sf), two passes (:114-119), 0 for S < 2
// `nonfinite` is OR-ed with 1 where the reference asserts isfinite(feats) (:120): every product,
// the mean and the std are looked at.
// LDS: sf and af as doubles.  The product loop reads sf[i] (a few distinct addresses per wavefront:
// broadcast) and af[j] at consecutive j: ds_read_b64 takes 32 lanes per cycle over 64 4-byte banks,
// so 32 consecutive doubles are conflict free.
__global__ __launch_bounds__(256) void crosscorr_f64_kernel(
    const double* __restrict__ states, const double* __restrict__ actions, double* __restrict__ out,
    int64_t n, int ts, int ta, int sd, int ad, int w, int use_diff, int64_t ld_out,
    int32_t* __restrict__ nonfinite) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int sfeat = sd - 1;
  const int S = w * sfeat, A = w * ad;
  double* sf = smem;         // [S]
  double* af = smem + S;     // [A]
  const int tid = threadIdx.x, nt = blockDim.x, ln = tid & 63;
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const double* s = states + traj * (int64_t)ts * sd;
    const double* a = actions + traj * (int64_t)ta * ad;
    double* o = out + traj * ld_out;
    __syncthreads();                               // the trajectory before is done with sf / af
    for (int t = 0; t < w; ++t) {                  // (w <= ts: crosscorr_window)
      const double* srow = s + (int64_t)t * sd;
      for (int c = tid; c < sfeat; c += nt)
        sf[t * sfeat + c] = use_diff ? (srow[c + 1] - srow[c]) : srow[c];
      const double* arow = a + (int64_t)min(t, ta - 1) * ad;   // pad: repeat the last step (:52-58)
      for (int c = tid; c < ad; c += nt) af[t * ad + c] = arow[c];
    }
    __syncthreads();
    // mean, then the squared deviations from it (torch.mean / torch.std): by every wavefront for
    // itself, same values in the same order in each
    double part = 0.0;
    for (int i = ln; i < S; i += 64) part += sf[i];
    const double mean = wave_sum_f64(part) / (double)S;
    part = 0.0;
    for (int i = ln; i < S; i += 64) {
      const double dv = sf[i] - mean;
      part += dv * dv;
    }
    const double sdev = S < 2 ? 0.0 : sqrt(wave_sum_f64(part) / (double)(S - 1));
    const int64_t total = (int64_t)S * A;
    bool bad = false;
    const int step_i = nt / A, step_j = nt % A;
    int i = tid / A, j = tid % A;
    for (int64_t e = tid; e < total; e += nt) {
      const double v = sf[i] * af[j];
      bad |= !isfinite(v);
      o[e] = v;
      i += step_i; j += step_j;
      if (j >= A) { j -= A; ++i; }
    }
    if (tid == 0) {
      o[total] = mean;
      o[total + 1] = sdev;
      bad |= !(isfinite(mean) && isfinite(sdev));
    }
    if (bad && nonfinite) atomicOr(nonfinite, 1);
  }
}

// ------------------------------------------------------------------ K3
// summary_signatory: summarizers.py:144-168.  Path X_l = [l+1 | s_l | a_l] (:152-155), signature
// levels 1..3 in signatory's layout; the Chen / Horner recurrences of signature3_kernel
// (csrc/summarizers.hip), in double:
//   S3[i,j,k] += (S2[i,j] + (S1[i] + D[i]/3) * D[j]/2) * D[k]
//   S2[i,j]   += (S1[i] + D[i]/2) * D[j]
//   S1[i]      = X_l[i] - X_0[i]
// One thread per (i,j) pair keeps S2[i,j] and the S3[i,j,:] row in registers for the whole path
// (2 DMAX VGPRs: 48 at DMAX = 24, every index a compile-time constant, so the row never goes to
// scratch); the level-3 terms are staged in LDS and stored lane-contiguous, 8 bytes per lane.
// LDS in doubles: path [L d] | increments [(L-1) dp], rows zero-padded to dp = d rounded up to 2 |
// stage [d^3]; 86 KB at d = 22, L = 3.  Access patterns: the loop reads D[i], D[j], X_l[i] with
// ds_read_b64 (32 lanes per cycle, 64 banks of 4 bytes: consecutive j are consecutive doubles,
// conflict free; equal addresses broadcast) and the D[k] pairs as 16-byte broadcasts.  The stage is
// written with ds_write_b64 at a lane stride of d doubles (16 lanes per cycle over 32 banks):
// conflict free for odd d, a gcd(2 d, 32) / 2-way conflict for even d -- left as it is.
template <int DMAX>
__global__ __launch_bounds__(512) void signature3_f64_kernel(
    const double* __restrict__ states, const double* __restrict__ actions, double* __restrict__ out,
    int64_t n, int length, int sd, int ad, int64_t ld_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int d = 1 + sd + ad;
  const int dp = (d + 1) & ~1;
  double* path = smem;                                  // [length * d]
  double* delta = smem + ((length * d + 1) & ~1);       // [(length-1) * dp]
  double* stage = delta + (length - 1) * dp;            // [d*d*d]
  const int tid = threadIdx.x, nt = blockDim.x;
  const int npairs = d * d;
  const int i = tid / d, j = tid % d;
  const bool active = tid < npairs;
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const double* s = states + traj * (int64_t)length * sd;
    const double* a = actions + traj * (int64_t)length * ad;
    double* o = out + traj * ld_out;
    __syncthreads();                                    // the trajectory before is done with the stage
    for (int e = tid; e < length * sd; e += nt) {
      const int l = e / sd, c = e - l * sd;
      path[l * d + 1 + c] = s[e];
    }
    for (int e = tid; e < length * ad; e += nt) {
      const int l = e / ad, c = e - l * ad;
      path[l * d + 1 + sd + c] = a[e];
    }
    for (int l = tid; l < length; l += nt) path[l * d] = (double)(l + 1);
    __syncthreads();
    for (int e = tid; e < (length - 1) * dp; e += nt) {
      const int l = e / dp, c = e - l * dp;
      delta[e] = c < d ? path[(l + 1) * d + c] - path[l * d + c] : 0.0;
    }
    __syncthreads();
    if (active) {
      double s2 = 0.0;
      double s3[DMAX];
#pragma unroll
      for (int k = 0; k < DMAX; ++k) s3[k] = 0.0;
      const double x0i = path[i];
      for (int l = 0; l + 1 < length; ++l) {
        const double* dl = delta + l * dp;
        const double di = dl[i], dj = dl[j];
        const double s1i = path[l * d + i] - x0i;
        const double coef = s2 + (s1i + di * (1.0 / 3.0)) * dj * 0.5;
#pragma unroll
        for (int k2 = 0; k2 < DMAX / 2; ++k2) {
          if (2 * k2 < d) {
            const double2 q = *reinterpret_cast<const double2*>(dl + 2 * k2);
            s3[2 * k2 + 0] = fma(coef, q.x, s3[2 * k2 + 0]);
            s3[2 * k2 + 1] = fma(coef, q.y, s3[2 * k2 + 1]);
          }
        }
        s2 = fma(s1i + di * 0.5, dj, s2);
      }
#pragma unroll
      for (int k = 0; k < DMAX; ++k)
        if (k < d) stage[tid * d + k] = s3[k];
      o[d + tid] = s2;                                   // level 2
    }
    for (int c = tid; c < d; c += nt)                    // level 1
      o[c] = path[(length - 1) * d + c] - path[c];
    __syncthreads();
    double* o3 = o + d + npairs;
    const int n3 = npairs * d;
    for (int e = tid; e < n3; e += nt) o3[e] = stage[e];
  }
}

// depth <= 2 for wider paths (signature12_kernel): S2[i,j] = sum_l (X_l[i]-X_0[i] + D_l[i]/2) D_l[j]
__global__ __launch_bounds__(256) void signature12_f64_kernel(
    const double* __restrict__ states, const double* __restrict__ actions, double* __restrict__ out,
    int64_t n, int length, int sd, int ad, int depth, int64_t ld_out) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int d = 1 + sd + ad;
  const int tid = threadIdx.x, nt = blockDim.x;
  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const double* s = states + traj * (int64_t)length * sd;
    const double* a = actions + traj * (int64_t)length * ad;
    double* o = out + traj * ld_out;
    if (depth == 1) {  // last - first row (time channel: L-1)
      for (int c = tid; c < d; c += nt) {
        double v;
        if (c == 0) v = (double)(length - 1);
        else if (c <= sd) v = s[(int64_t)(length - 1) * sd + c - 1] - s[c - 1];
        else v = a[(int64_t)(length - 1) * ad + c - 1 - sd] - a[c - 1 - sd];
        o[c] = v;
      }
      continue;
    }
    double* path = smem;  // [length * d]
    __syncthreads();
    for (int l = 0; l < length; ++l) {
      double* row = path + l * d;
      if (tid == 0) row[0] = (double)(l + 1);
      for (int c = tid; c < sd; c += nt) row[1 + c] = s[(int64_t)l * sd + c];
      for (int c = tid; c < ad; c += nt) row[1 + sd + c] = a[(int64_t)l * ad + c];
    }
    __syncthreads();
    for (int c = tid; c < d; c += nt) o[c] = path[(length - 1) * d + c] - path[c];
    const int n2 = d * d;
    const int step_i = nt / d, step_j = nt % d;
    int i = tid / d, j = tid % d;
    for (int e = tid; e < n2; e += nt) {
      const double x0i = path[i];
      double acc = 0.0;
      for (int l = 0; l + 1 < length; ++l) {
        const double* p0 = path + l * d;
        const double* p1 = p0 + d;
        acc = fma((p0[i] - x0i) + (p1[i] - p0[i]) * 0.5, p1[j] - p0[j], acc);
      }
      o[d + e] = acc;
      i += step_i; j += step_j;
      if (j >= d) { j -= d; ++i; }
    }
  }
}

static int grid_for(int64_t n) { return capped_grid(n, BSIG_F64_SUMMARY_GRID_CAP); }

// (common.h: raise_lds_limit) only the launches that need it ask
template <typename K>
static int allow_lds(K kernel, size_t lds, LdsRaised* raised) {
  return lds > kLdsUnraised ? raise_lds_limit(kernel, kLdsBytes, raised) : BSIG_OK;
}

template <int DMAX>
static int launch_sig3(const double* states, const double* actions, double* out, int64_t n, int length,
                       int sd, int ad, int64_t ld_out, int threads, size_t lds, hipStream_t st) {
  static LdsRaised raised;
  BSIG_TRY(allow_lds(signature3_f64_kernel<DMAX>, lds, &raised));
  hipLaunchKernelGGL((signature3_f64_kernel<DMAX>), dim3(grid_for(n)), dim3(threads), lds, st, states,
                     actions, out, n, length, sd, ad, ld_out);
  BSIG_CHECK_LAUNCH("signature_f64");
  return BSIG_OK;
}

}  // namespace f64
}  // namespace bsig

using namespace bsig;

extern "C" int bsig_summary_start_f64(const double* states, const double* actions, double* out,
                                      int64_t n, int t_states, int t_actions, int sd, int ad,
                                      int max_t, int64_t ld_out, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_summary_start_f64");
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(states && actions && out, "summary_start_f64: null pointer");
  BSIG_REQUIRE(n >= 0 && t_states >= 1 && t_actions >= 1 && sd >= 1 && ad >= 1 && max_t >= 1,
               "summary_start_f64: bad dims n=%lld ts=%d ta=%d sd=%d ad=%d max_t=%d",
               (long long)n, t_states, t_actions, sd, ad, max_t);
  BSIG_REQUIRE(ld_out >= (int64_t)max_t * (sd + ad), "summary_start_f64: ld_out too small");
  const int width = sd + ad;
  hipLaunchKernelGGL(f64::summary_start_f64_kernel, dim3(f64::grid_for(n)),
                     dim3(width >= 192 ? 256 : (width >= 96 ? 128 : 64)), 0, as_stream(stream), states,
                     actions, out, n, t_states, t_actions, sd, ad, max_t, ld_out);
  BSIG_CHECK_LAUNCH("summary_start_f64");
  return BSIG_OK;
}

extern "C" int bsig_crosscorr_f64(const double* states, const double* actions, double* out, int64_t n,
                                  int t_states, int t_actions, int sd, int ad, int use_state_diff,
                                  int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_crosscorr_f64");
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(states && actions && out, "crosscorr_f64: null pointer");
  BSIG_REQUIRE(n >= 0 && sd >= 2 && ad >= 1, "crosscorr_f64: bad dims sd=%d ad=%d", sd, ad);
  BSIG_REQUIRE(t_states > 1, "crosscorr_f64: traj_len must be > 1 (summarizers.py:94)");
  BSIG_REQUIRE(t_actions >= 1, "crosscorr_f64: no actions");
  int w = sd > 50 ? 5 : 10;                       // summarizers.py:96-98
  if (t_states <= w) w = t_states;                // :99 (only crop when longer)
  const int64_t S = (int64_t)w * (sd - 1), A = (int64_t)w * ad;
  BSIG_REQUIRE(ld_out >= S * A + 2, "crosscorr_f64: ld_out too small");
  const size_t lds = (size_t)(S + A) * sizeof(double);
  if (lds > kLdsBytes) {
    set_error("crosscorr_f64: %zu B of LDS needed", lds);
    return BSIG_EUNSUPPORTED;
  }
  static LdsRaised raised;
  BSIG_TRY(f64::allow_lds(f64::crosscorr_f64_kernel, lds, &raised));
  hipLaunchKernelGGL(f64::crosscorr_f64_kernel, dim3(f64::grid_for(n)), dim3(256), lds, as_stream(stream),
                     states, actions, out, n, t_states, t_actions, sd, ad, w, use_state_diff, ld_out,
                     nonfinite);
  BSIG_CHECK_LAUNCH("crosscorr_f64");
  return BSIG_OK;
}

extern "C" int bsig_signature_f64(const double* states, const double* actions, double* out, int64_t n,
                                  int length, int sd, int ad, int depth, int64_t ld_out,
                                  bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_signature_f64");
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(states && actions && out, "signature_f64: null pointer");
  BSIG_REQUIRE(n >= 0 && length >= 2 && sd >= 1 && ad >= 1,
               "signature_f64: bad dims length=%d sd=%d ad=%d", length, sd, ad);
  const int d = 1 + sd + ad;
  if (depth <= 0) depth = ref_signature_depth(d);
  BSIG_REQUIRE(depth >= 1 && depth <= 3, "signature_f64: depth %d not in 1..3", depth);
  BSIG_REQUIRE(ld_out >= bsig_summary_dim(3, length, sd, ad, depth), "signature_f64: ld_out too small");
  const hipStream_t st = as_stream(stream);
  if (depth == 3) {
    // every d the reference takes at depth 3 (d^3 <= 110^2): one (i,j) pair per thread of a
    // 512-thread workgroup
    if (d > 22) {
      set_error("signature_f64: depth 3 needs path dim <= 22 (got %d)", d);
      return BSIG_EUNSUPPORTED;
    }
    const size_t lds = ((size_t)((length * (int64_t)d + 1) & ~(int64_t)1) +
                        (size_t)(length - 1) * ((d + 1) & ~1) + (size_t)d * d * d) * sizeof(double);
    if (lds > kLdsBytes) {
      set_error("signature_f64: %zu B of LDS needed (%zu in a workgroup)", lds, kLdsBytes);
      return BSIG_EUNSUPPORTED;
    }
    const int threads = (int)round_up<int64_t>((int64_t)d * d, 64);
    if (d <= 8) return f64::launch_sig3<8>(states, actions, out, n, length, sd, ad, ld_out, threads, lds, st);
    if (d <= 16) return f64::launch_sig3<16>(states, actions, out, n, length, sd, ad, ld_out, threads, lds, st);
    return f64::launch_sig3<24>(states, actions, out, n, length, sd, ad, ld_out, threads, lds, st);
  }
  size_t lds = 0;
  if (depth == 2) {
    lds = (size_t)length * d * sizeof(double);
    if (lds > kLdsBytes) {
      set_error("signature_f64: %zu B of LDS needed (%zu in a workgroup)", lds, kLdsBytes);
      return BSIG_EUNSUPPORTED;
    }
    static LdsRaised raised;
    BSIG_TRY(f64::allow_lds(f64::signature12_f64_kernel, lds, &raised));
  }
  hipLaunchKernelGGL(f64::signature12_f64_kernel, dim3(f64::grid_for(n)), dim3(256), lds, st, states,
                     actions, out, n, length, sd, ad, depth, ld_out);
  BSIG_CHECK_LAUNCH("signature_f64");
  return BSIG_OK;
}
