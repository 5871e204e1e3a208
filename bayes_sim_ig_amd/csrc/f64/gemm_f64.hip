// fp64 GEMM on v_mfma_f64_16x16x4_f64 with the fused epilogues of the fp32 GEMM (include/bsig_f64.h).
//
// One tile shape: a 64 x 64 workgroup tile, 4 wavefronts (2 x 2, a 32 x 32 block of four MFMA
// tiles each), k in steps of 16 through a double-buffered LDS image.  K is never split: every
// output is one accumulation chain in ascending k, so a result does not depend on the launch.
//
// MFMA operand maps of the f64 16x16x4 form: lane l feeds A[row = l & 15][k = l >> 4] and
// B[k = l >> 4][col = l & 15], one double each; result register r of lane l is
// D[row = (l >> 4) + 4 r][col = l & 15] -- NOT the (l >> 4) * 4 + r rows of the f32 forms.
//
// LDS image of an operand: S[kk][r], r = row (A) / column (B) inside the tile, pitch kPitch = 81
// doubles.  The odd pitch was chosen on paper, not measured: it is meant to spread the 16 lanes
// of a k-contiguous tile store (16 values of kk at one r) and the two k values a ds_read_b64 half
// covers over different banks.  Nothing in this kernel has been profiled or tuned.
#include "f64.h"

#include <cmath>

namespace bsig {
namespace f64 {

typedef double double4_t __attribute__((ext_vector_type(4)));

constexpr int kTile = 64, kTk = 16, kPitch = 81, kThreads = 256;
constexpr int kPerThread = kTile * kTk / kThreads;   // 4 elements of each operand per thread and k-step

struct GemmArgs {
  const double* a; int64_t lda; int a_kmajor; const int32_t* a_rows;
  const double* b; int64_t ldb; int b_kmajor; const int32_t* b_rows;
  double* c; int64_t ldc;
  int m, n, k;
  int epilogue, act;
  const double* bias; const double* aux; int64_t ldaux;
  double alpha;
};

__device__ inline double act_fwd(double v, int act) {
  switch (act) {
    case BSIG_ACT_TANH: return tanh(v);
    case BSIG_ACT_RELU: return v > 0.0 ? v : 0.0;
    case BSIG_ACT_LEAKY_RELU: return v > 0.0 ? v : 0.01 * v;
    case BSIG_ACT_SIGMOID: return 1.0 / (1.0 + exp(-v));
    default: return v;
  }
}
// derivative expressed through the activation OUTPUT h
__device__ inline double act_bwd_from_out(double h, int act) {
  switch (act) {
    case BSIG_ACT_TANH: return 1.0 - h * h;
    case BSIG_ACT_RELU: return h > 0.0 ? 1.0 : 0.0;
    case BSIG_ACT_LEAKY_RELU: return h > 0.0 ? 1.0 : 0.01;
    case BSIG_ACT_SIGMOID: return h * (1.0 - h);
    default: return 1.0;
  }
}

// The thread's 4 elements of the [kTk][64] image of one operand at k-step k0: element e = tid +
// 256 i sits at (kk, r) = (e % 16, e / 16) of a k-contiguous operand (consecutive lanes read
// consecutive k of one row) and at (e / 64, e % 64) of a k-major one (consecutive lanes read
// consecutive rows at one k).  Rows past `extent` and k past K read as zero.
__device__ __forceinline__ void fetch(const double* __restrict__ src, int64_t ld, int kmajor,
                                      const int32_t* __restrict__ rows, int r0, int extent, int k0,
                                      int K, int tid, double (&q)[kPerThread]) {
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int e = tid + kThreads * i;
    const int kk = kmajor ? e >> 6 : e & 15, r = kmajor ? e & 63 : e >> 4;
    const int gr = r0 + r, gk = k0 + kk;
    double v = 0.0;
    if (gr < extent && gk < K) {
      if (kmajor) v = src[(int64_t)(rows ? rows[gk] : gk) * ld + gr];
      else v = src[(int64_t)(rows ? rows[gr] : gr) * ld + gk];
    }
    q[i] = v;
  }
}
__device__ __forceinline__ void stash(double* __restrict__ s, int kmajor, int tid,
                                      const double (&q)[kPerThread]) {
#pragma unroll
  for (int i = 0; i < kPerThread; ++i) {
    const int e = tid + kThreads * i;
    const int kk = kmajor ? e >> 6 : e & 15, r = kmajor ? e & 63 : e >> 4;
    s[kk * kPitch + r] = q[i];
  }
}

__global__ __launch_bounds__(kThreads) void gemm_f64_kernel(GemmArgs g) {
  __shared__ double sa[2][kTk * kPitch];
  __shared__ double sb[2][kTk * kPitch];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int m0 = blockIdx.y * kTile, n0 = blockIdx.x * kTile;
  const int lr = lane & 15, lk = lane >> 4;

  double4_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = double4_t{0.0, 0.0, 0.0, 0.0};

  double qa[kPerThread], qb[kPerThread];
  const int nt = (g.k + kTk - 1) / kTk;
  fetch(g.a, g.lda, g.a_kmajor, g.a_rows, m0, g.m, 0, g.k, tid, qa);
  fetch(g.b, g.ldb, g.b_kmajor, g.b_rows, n0, g.n, 0, g.k, tid, qb);
  stash(sa[0], g.a_kmajor, tid, qa);
  stash(sb[0], g.b_kmajor, tid, qb);
  __syncthreads();
  for (int t = 0; t < nt; ++t) {
    const int cur = t & 1;
    if (t + 1 < nt) {   // the next k-step's global loads fly under this one's MFMAs
      fetch(g.a, g.lda, g.a_kmajor, g.a_rows, m0, g.m, (t + 1) * kTk, g.k, tid, qa);
      fetch(g.b, g.ldb, g.b_kmajor, g.b_rows, n0, g.n, (t + 1) * kTk, g.k, tid, qb);
    }
#pragma unroll
    for (int ks = 0; ks < kTk / 4; ++ks) {
      const double* pa = sa[cur] + (ks * 4 + lk) * kPitch + wm + lr;
      const double* pb = sb[cur] + (ks * 4 + lk) * kPitch + wn + lr;
      const double a0 = pa[0], a1 = pa[16], b0 = pb[0], b1 = pb[16];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    if (t + 1 < nt) {   // (the other buffer: last read before the barrier that ended step t - 1)
      stash(sa[cur ^ 1], g.a_kmajor, tid, qa);
      stash(sb[cur ^ 1], g.b_kmajor, tid, qb);
    }
    __syncthreads();
  }

  // epilogue: register r of tile (i, j) is row wm + 16 i + lk + 4 r, column wn + 16 j + lr
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int gm = m0 + wm + 16 * i + lk + 4 * r, gn = n0 + wn + 16 * j + lr;
        if (gm >= g.m || gn >= g.n) continue;
        double v = acc[i][j][r];
        double* out = g.c + (int64_t)gm * g.ldc + gn;
        switch (g.epilogue) {
          case BSIG_EPI_BIAS: v += g.bias[gn]; break;
          case BSIG_EPI_BIAS_ACT: v = act_fwd(v + g.bias[gn], g.act); break;
          case BSIG_EPI_COS_SIN: {
            double s, c;
            sincos(v, &s, &c);
            out[g.n] = g.alpha * s;
            v = g.alpha * c;
            break;
          }
          case BSIG_EPI_COS_OFF: v = g.alpha * cos(v + g.bias[gn]); break;
          case BSIG_EPI_MUL_DACT: v *= act_bwd_from_out(g.aux[(int64_t)gm * g.ldaux + gn], g.act); break;
          default: break;
        }
        *out = v;
      }
}

int gemm_run(const Gemm& p, hipStream_t st) {
  BSIG_REQUIRE(p.a && p.b && p.c, "gemm_f64: null operand");
  BSIG_REQUIRE(p.m >= 1 && p.n >= 1 && p.k >= 1, "gemm_f64: empty product");
  BSIG_REQUIRE(p.m < (1ll << 30) && p.n < (1ll << 30) && p.k < (1ll << 30), "gemm_f64: dimension too large");
  BSIG_REQUIRE(p.epilogue >= BSIG_EPI_NONE && p.epilogue <= BSIG_EPI_MUL_DACT, "gemm_f64: bad epilogue");
  BSIG_REQUIRE(p.act >= BSIG_ACT_TANH && p.act <= BSIG_ACT_IDENTITY, "gemm_f64: bad activation");
  BSIG_REQUIRE(p.lda >= (p.a_kmajor ? p.m : p.k) && p.ldb >= (p.b_kmajor ? p.n : p.k),
               "gemm_f64: operand pitch below the row width");
  BSIG_REQUIRE(p.ldc >= (p.epilogue == BSIG_EPI_COS_SIN ? 2 * p.n : p.n), "gemm_f64: ldc too small");
  const bool needs_bias = p.epilogue == BSIG_EPI_BIAS || p.epilogue == BSIG_EPI_BIAS_ACT ||
                          p.epilogue == BSIG_EPI_COS_OFF;
  BSIG_REQUIRE(!needs_bias || p.bias, "gemm_f64: epilogue needs bias");
  BSIG_REQUIRE(p.epilogue != BSIG_EPI_MUL_DACT || (p.aux && p.ldaux >= p.n), "gemm_f64: epilogue needs aux");
  const int64_t gx = ceil_div<int64_t>(p.n, kTile), gy = ceil_div<int64_t>(p.m, kTile);
  BSIG_REQUIRE(gy <= 65535, "gemm_f64: more than 65535 row tiles");
  GemmArgs g;
  g.a = p.a; g.lda = p.lda; g.a_kmajor = p.a_kmajor; g.a_rows = p.a_rows;
  g.b = p.b; g.ldb = p.ldb; g.b_kmajor = p.b_kmajor; g.b_rows = p.b_rows;
  g.c = p.c; g.ldc = p.ldc; g.m = (int)p.m; g.n = (int)p.n; g.k = (int)p.k;
  g.epilogue = p.epilogue; g.act = p.act; g.bias = p.bias; g.aux = p.aux; g.ldaux = p.ldaux;
  g.alpha = p.alpha;
  hipLaunchKernelGGL(gemm_f64_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(kThreads), 0, st, g);
  BSIG_CHECK_LAUNCH("gemm_f64");
  return BSIG_OK;
}

}  // namespace f64
}  // namespace bsig

using namespace bsig;

extern "C" int bsig_gemm_f64(const double* a, int64_t lda, int a_kmajor, const int32_t* a_rows,
                             const double* b, int64_t ldb, int b_kmajor, const int32_t* b_rows,
                             double* c, int64_t ldc, int64_t m, int64_t n, int64_t k, int epilogue,
                             int act, const double* bias, const double* aux, int64_t ldaux,
                             double alpha, bsig_stream_t stream) {
  f64::Gemm g;
  g.a = a; g.lda = lda; g.a_kmajor = a_kmajor; g.a_rows = a_rows;
  g.b = b; g.ldb = ldb; g.b_kmajor = b_kmajor; g.b_rows = b_rows;
  g.c = c; g.ldc = ldc; g.m = m; g.n = n; g.k = k;
  g.epilogue = epilogue; g.act = act; g.bias = bias; g.aux = aux; g.ldaux = ldaux; g.alpha = alpha;
  return f64::gemm_run(g, as_stream(stream));
}

extern "C" int bsig_rff_project_f64(const double* x, int64_t ldx, const int32_t* x_rows,
                                    const double* coeff, int64_t ld_coeff, const double* offset,
                                    double* feats, int64_t ld_feats, int64_t batch, int64_t in_dim,
                                    int64_t m_feat, double a, int cos_only, bsig_stream_t stream) {
  BSIG_REQUIRE(!(cos_only && !offset), "rff_project_f64: cos-only RFF needs an offset");
  f64::Gemm g;
  g.a = x; g.lda = ldx; g.a_rows = x_rows;
  g.b = coeff; g.ldb = ld_coeff;
  g.c = feats; g.ldc = ld_feats; g.m = batch; g.n = m_feat; g.k = in_dim;
  g.epilogue = cos_only ? BSIG_EPI_COS_OFF : BSIG_EPI_COS_SIN;
  g.bias = offset; g.alpha = a;
  return f64::gemm_run(g, as_stream(stream));
}
