// Mixture-density head in double (include/bsig_f64.h): forward tuple, NLL and its backward --
// the closed forms of SURVEY.md Appendix A.1-A.3, derived from mdnn.py:108-178.
//
// mdn_nll_f64_kernel<FULL>: one wavefront per row, four rows per workgroup; lane k < K runs component k through the
// phases of the component row (../mdn_row.h, the body the fp32 kernels run), the row read from global memory, the
// gradients written to its d_out row, the logsumexp through the wavefront's LDS.  mdn_finish_f64_kernel: loss mean,
// the non-detached jitter-mean term sum(u dL/dsigma), head bias column sums, engine state advance.  The forward()
// tuple is mdn::mdn_outputs_kernel<double>.  Every sum has a fixed order: two runs are bitwise equal.
#include "f64.h"
#include "../mdn_row.h"

#include <algorithm>
#include <cmath>

namespace bsig {
namespace f64 {

constexpr int kRowsPerBlock = 4;   // wavefronts per workgroup
constexpr int kSigMax = 64;        // partial sums of exp(pre_diag)

struct HeadArgs {
  const double* seg_w; int64_t ld_w;
  const double* seg_mu; int64_t ld_mu;
  const double* seg_sg; int64_t ld_sg;
  const double* seg_lo; int64_t ld_lo;
  int from_tuple;
  const double* y; int64_t ldy; const int32_t* y_rows;
  int batch; double inv_norm;
  int D, K, Ls;
  const double* noise; uint64_t seed, stream_id;
  double eps_noise, min_w, ll_limit;
  const double* sig_partials; int n_sig;
  double* d_out; int64_t ld_dout;
  double* row_lse; double* row_uds;
  int32_t* nonfinite;
};

// every thread gets the block's sum; `scratch` holds blockDim.x / 64 doubles
__device__ inline double block_sum_f64(double v, double* scratch) {
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int nw = (blockDim.x + 63) >> 6;
  v = wave_sum_f64(v);
  __syncthreads();
  if (lane == 0) scratch[wid] = v;
  __syncthreads();
  double t = 0.0;
  for (int i = 0; i < nw; ++i) t += scratch[i];
  return t;
}

// partial sums of exp(pre_diag) over [batch, DK] for the jitter scale EPS_NOISE * mean(exp(pre))
__global__ __launch_bounds__(256) void sigma0_sum_f64_kernel(const double* __restrict__ pre, int64_t ld,
                                                             int batch, int DK, double* __restrict__ partials) {
  __shared__ double red[4];
  const int64_t total = (int64_t)batch * DK;
  double s = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x)
    s += exp(pre[(e / DK) * ld + (e % DK)]);
  s = block_sum_f64(s, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

template <bool FULL>
__global__ __launch_bounds__(64 * kRowsPerBlock) void mdn_nll_f64_kernel(HeadArgs a) {
  extern __shared__ double lds[];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const int D = a.D, K = a.K, DK = D * K;
  const int per_wave = (FULL ? 2 : 1) * DK + K;
  const int row = blockIdx.x * kRowsPerBlock + wid;
  if (row >= a.batch) return;   // (wavefront-uniform; nothing below crosses wavefronts)
  const int k = lane < K ? lane : 0;
  const bool comp = lane < K;
  double* v_ = lds + wid * per_wave + k;   // v_[i * K]: T v = y - mu
  double* q_ = v_ + DK;                    // q_[i * K]: T^T q = v   (FULL)
  double* rk = lds + wid * per_wave + (FULL ? 2 : 1) * DK;

  double eps = 0.0;
  if (a.eps_noise != 0.0) {
    double s = 0.0;
    for (int i = 0; i < a.n_sig; ++i) s += a.sig_partials[i];
    eps = a.eps_noise * (s / ((double)a.batch * (double)DK));   // mdnn.py:115, not detached
  }
  // the component row on the four pitched segments of the row; gradients go to the row of d_out
  const bool bwd = a.d_out != nullptr;
  double* dT = bwd ? a.d_out + (int64_t)row * a.ld_dout : nullptr;
  const mdn::RowHyper<double> h{D, K, a.from_tuple != 0, a.min_w, a.ll_limit, a.inv_norm, a.noise, a.seed, a.stream_id};
  mdn::RowView<double> view{};
  view.lg = a.seg_w + (int64_t)row * a.ld_w;
  view.mu = a.seg_mu + (int64_t)row * a.ld_mu + k;
  view.sg = a.seg_sg + (int64_t)row * a.ld_sg + k;
  view.lo = FULL ? a.seg_lo + (int64_t)row * a.ld_lo + k : nullptr;
  if (bwd) { view.d_mu = dT + K + k; view.d_sg = view.d_mu + DK; view.d_lo = view.d_sg + DK; }
  view.es = K;
  view.y = a.y + (int64_t)(a.y_rows ? a.y_rows[row] : row) * a.ldy;
  view.v = v_; view.q = q_; view.vs = K;
  view.je = (int64_t)row * DK + k;

  mdn::CompState<double> c{};
  if (comp) {
    mdn::comp_weights(view, h, k, c);
    rk[k] = mdn::comp_elements<double, FULL, true>(view, h, eps, c);   // (a v plane for diagonal rows too)
  }
  // (rk[] crosses LANES of this wavefront only -- a row never spans wavefronts, and the early
  // return above is row-uniform -- and a wavefront's LDS operations issue in order: a scheduling fence is
  // all that is needed, no __syncthreads().  A row spread over several wavefronts would break this.)
  __builtin_amdgcn_wave_barrier();
  const double lse = mdn::row_lse(rk, K);

  double uds = 0.0;
  if (bwd && comp) dT[k] = mdn::comp_backward<double, FULL, true>(view, h, k, eps, c, rk, lse, uds);
  uds = wave_sum_f64(comp ? uds : 0.0);
  if (lane == 0) {
    a.row_lse[row] = lse;
    if (a.row_uds) a.row_uds[row] = uds;
  }
  if (__any(c.bad) && lane == 0 && a.nonfinite) atomicOr(a.nonfinite, kFlagNonfinite);
}

// Fit-engine state advance (single writer; every reader of these words runs in a later kernel).
__device__ inline void run_finish_hook(const FinishHook& hook) {
  st64_finish_hook(hook.state, hook.kind == 1, hook.beta1, hook.beta2, hook.lr);
}

// loss = -(sum of the rows' logsumexp) / batch; d pre += (EPS / (B D K)) sum(u dL/dsigma) exp(pre)
// (the non-detached mean of mdnn.py:115); column sums of the corrected d_out (head bias gradients).
// Grid: 64-column groups of d_out; block = 64 columns x 4 row lanes, all rows.
__global__ __launch_bounds__(256) void mdn_finish_f64_kernel(
    const double* __restrict__ row_lse, const double* __restrict__ row_uds, int batch, int pre_begin,
    int dk, int nh, double eps_noise, const double* __restrict__ pre, int64_t ld_pre,
    double* __restrict__ d_out, int64_t ld_dout, double* __restrict__ colsum, double* __restrict__ loss,
    int32_t* __restrict__ nonfinite, FinishHook hook) {
  __shared__ double red[4];
  __shared__ double part[4][64];
  if (blockIdx.x == 0 && loss) {
    double s = 0.0;
    for (int i = threadIdx.x; i < batch; i += blockDim.x) s += row_lse[i];
    s = block_sum_f64(s, red);
    if (threadIdx.x == 0) {
      const double l = -s / (double)batch;
      loss[0] = l;
      if (!isfinite(l) && nonfinite) atomicOr(nonfinite, kFlagNonfinite);
    }
  }
  if (hook.state && blockIdx.x == 0 && threadIdx.x == 0) run_finish_hook(hook);
  if (!d_out) return;
  double c = 0.0;
  if (eps_noise != 0.0) {
    double s = 0.0;
    for (int i = threadIdx.x; i < batch; i += blockDim.x) s += row_uds[i];
    s = block_sum_f64(s, red);
    c = eps_noise / ((double)batch * (double)dk) * s;
  }
  const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
  const int col = blockIdx.x * 64 + cl;
  const bool fix = c != 0.0 && col >= pre_begin && col < pre_begin + dk;
  double acc = 0.0;
  if (col < nh)
    for (int row = rl; row < batch; row += 4) {
      double v = d_out[(int64_t)row * ld_dout + col];
      if (fix) {
        v += c * exp(pre[(int64_t)row * ld_pre + (col - pre_begin)]);
        d_out[(int64_t)row * ld_dout + col] = v;
      }
      acc += v;
    }
  if (!colsum) return;
  part[rl][cl] = acc;
  __syncthreads();
  if (rl == 0 && col < nh) colsum[col] = (part[0][cl] + part[1][cl]) + (part[2][cl] + part[3][cl]);
}

// ---------------------------------------------------------------- host side
struct HeadGeom { int D, K, Ls, Nh; size_t lds; };

static int head_geom(const bsig_head_dims* d, HeadGeom* g) {
  BSIG_REQUIRE(d && d->out_dim >= 1 && d->n_comp >= 1, "mdn head f64: bad dims");
  BSIG_REQUIRE(d->n_comp <= 64, "mdn head f64: at most 64 components");
  g->D = d->out_dim; g->K = d->n_comp;
  g->Ls = d->full_cov ? d->out_dim * (d->out_dim - 1) / 2 : 0;
  g->Nh = g->K + 2 * g->D * g->K + g->Ls * g->K;
  g->lds = (size_t)kRowsPerBlock * ((g->Ls ? 2 : 1) * (size_t)g->D * g->K + g->K) * sizeof(double);
  if (g->lds > kLdsUnraised) {
    set_error("mdn head f64: %zu B of LDS needed for one workgroup", g->lds);
    return BSIG_EUNSUPPORTED;
  }
  return BSIG_OK;
}

// workspace doubles: [sig partials kSigMax][row_lse B][row_uds B]
static size_t head_ws_doubles(int64_t batch) { return kSigMax + 2 * (size_t)batch; }

static int sigma0_sum(const double* pre, int64_t ld, int64_t batch, int DK, double* partials, hipStream_t st) {
  const int n_sig = (int)std::min<int64_t>(kSigMax, ceil_div<int64_t>(batch * DK, 2048));
  hipLaunchKernelGGL(sigma0_sum_f64_kernel, dim3(n_sig), dim3(256), 0, st, pre, ld, (int)batch, DK, partials);
  BSIG_CHECK_LAUNCH("sigma0_sum_f64");
  return n_sig;
}

int head_nll_launch(const bsig_head_dims* dims, const bsig_f64_hyper& hy, const double* seg_w, int64_t ld_w,
                    const double* seg_mu, int64_t ld_mu, const double* seg_sg, int64_t ld_sg,
                    const double* seg_lo, int64_t ld_lo, int from_tuple, const double* y, int64_t ldy,
                    const int32_t* y_rows, int64_t batch, int64_t norm_batch, const double* noise,
                    uint64_t seed, uint64_t stream_id, double* loss, double* d_out, int64_t ld_dout,
                    double* colsum_out, int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                    hipStream_t st, const FinishHook& hook) {
  HeadGeom g;
  BSIG_TRY(head_geom(dims, &g));
  BSIG_REQUIRE(batch >= 1 && batch < (1 << 30), "mdn head f64: bad batch");
  BSIG_REQUIRE(workspace && workspace_bytes >= head_ws_doubles(batch) * sizeof(double),
               "mdn head f64: workspace too small (%zu < %zu)", workspace_bytes,
               head_ws_doubles(batch) * sizeof(double));
  BSIG_REQUIRE(!(g.Ls > 0 && !seg_lo), "mdn head f64: full covariance needs lower entries");
  BSIG_REQUIRE(!(colsum_out && !d_out), "mdn head f64: bias gradients need d_head_out");
  BSIG_REQUIRE(!(from_tuple && d_out), "mdn head f64: no backward from a forward() tuple");
  double* ws = reinterpret_cast<double*>(workspace);
  double* sig_partials = ws;
  double* row_lse = ws + kSigMax;
  double* row_uds = row_lse + batch;
  const int DK = g.D * g.K;
  const bool jitter = !from_tuple && hy.eps_noise != 0.0;
  int n_sig = 0;
  if (jitter) {
    n_sig = sigma0_sum(seg_sg, ld_sg, batch, DK, sig_partials, st);
    if (n_sig < 0) return n_sig;
  }
  HeadArgs a{};
  a.seg_w = seg_w; a.ld_w = ld_w; a.seg_mu = seg_mu; a.ld_mu = ld_mu;
  a.seg_sg = seg_sg; a.ld_sg = ld_sg; a.seg_lo = seg_lo; a.ld_lo = ld_lo;
  a.from_tuple = from_tuple;
  a.y = y; a.ldy = ldy; a.y_rows = y_rows;
  a.batch = (int)batch; a.inv_norm = 1.0 / (double)norm_batch;
  a.D = g.D; a.K = g.K; a.Ls = g.Ls;
  a.noise = noise; a.seed = seed; a.stream_id = stream_id;
  a.eps_noise = jitter ? hy.eps_noise : 0.0; a.min_w = hy.min_weight; a.ll_limit = hy.ll_limit;
  a.sig_partials = sig_partials; a.n_sig = n_sig;
  a.d_out = d_out; a.ld_dout = ld_dout;
  a.row_lse = row_lse; a.row_uds = row_uds; a.nonfinite = nonfinite;
  const dim3 grid((unsigned)ceil_div<int64_t>(batch, kRowsPerBlock)), block(64 * kRowsPerBlock);
  if (g.Ls > 0) hipLaunchKernelGGL(mdn_nll_f64_kernel<true>, grid, block, g.lds, st, a);
  else hipLaunchKernelGGL(mdn_nll_f64_kernel<false>, grid, block, g.lds, st, a);
  BSIG_CHECK_LAUNCH("mdn_nll_f64");
  const bool sweep = d_out != nullptr && (jitter || colsum_out != nullptr);
  hipLaunchKernelGGL(mdn_finish_f64_kernel, dim3(sweep ? (unsigned)ceil_div(g.Nh, 64) : 1u), dim3(256), 0, st,
                     row_lse, row_uds, (int)batch, g.K + DK, DK, g.Nh, (jitter && d_out) ? hy.eps_noise : 0.0,
                     seg_sg, ld_sg, sweep ? d_out : nullptr, ld_dout, colsum_out, loss, nonfinite, hook);
  BSIG_CHECK_LAUNCH("mdn_finish_f64");
  return BSIG_OK;
}

}  // namespace f64
}  // namespace bsig

using namespace bsig;

extern "C" size_t bsig_head_workspace_bytes_f64(const bsig_head_dims* d, int64_t batch) {
  f64::HeadGeom g;
  if (f64::head_geom(d, &g) != BSIG_OK) return 0;
  return f64::head_ws_doubles(batch < 1 ? 1 : batch) * sizeof(double);
}

extern "C" int bsig_mdn_head_outputs_f64(const bsig_head_dims* dims, const bsig_f64_hyper* hyper,
                                         const double* head_out, int64_t ld, int64_t batch,
                                         const double* noise, uint64_t seed, uint64_t stream_id,
                                         double* weights, double* mu, double* l_d, double* lower,
                                         int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                                         bsig_stream_t stream) {
  BSIG_REQUIRE(dims && head_out && weights && mu && l_d, "head_outputs_f64: null pointer");
  BSIG_REQUIRE(batch >= 1 && batch < (1 << 30), "head_outputs_f64: bad batch");
  f64::HeadGeom g;
  BSIG_TRY(f64::head_geom(dims, &g));
  BSIG_REQUIRE(!(g.Ls > 0 && !lower), "head_outputs_f64: full covariance needs `lower`");
  BSIG_REQUIRE(ld >= g.Nh, "head_outputs_f64: ld too small");
  BSIG_REQUIRE(workspace && workspace_bytes >= f64::kSigMax * sizeof(double), "head_outputs_f64: workspace too small");
  const bsig_f64_hyper hy = f64::resolve_hyper(hyper, dims, nullptr);
  double* sig_partials = reinterpret_cast<double*>(workspace);
  hipStream_t st = as_stream(stream);
  int n_sig = 0;
  if (hy.eps_noise != 0.0) {
    n_sig = f64::sigma0_sum(head_out + g.K + g.D * g.K, ld, batch, g.D * g.K, sig_partials, st);
    if (n_sig < 0) return n_sig;
  }
  hipLaunchKernelGGL(mdn::mdn_outputs_kernel<double>, dim3((int)std::min<int64_t>(batch, 2048)), dim3(256), 0, st,
                     head_out, ld, (int)batch, g.D, g.K, g.Ls, noise, seed, stream_id, hy.eps_noise,
                     hy.min_weight, sig_partials, n_sig, weights, mu, l_d, lower, nonfinite);
  BSIG_CHECK_LAUNCH("mdn_outputs_f64");
  return BSIG_OK;
}

extern "C" int bsig_mdn_nll_from_tuple_f64(const bsig_head_dims* dims, const bsig_f64_hyper* hyper,
                                           const double* weights, const double* mu, const double* l_d,
                                           const double* lower, const double* y, int64_t ldy,
                                           int64_t batch, double* loss, int32_t* nonfinite,
                                           void* workspace, size_t workspace_bytes, bsig_stream_t stream) {
  BSIG_REQUIRE(dims && weights && mu && l_d && y && loss, "nll_from_tuple_f64: null pointer");
  const int64_t D = dims->out_dim, K = dims->n_comp;
  const int64_t Ls = dims->full_cov ? D * (D - 1) / 2 : 0;
  return f64::head_nll_launch(dims, f64::resolve_hyper(hyper, dims, nullptr), weights, K, mu, D * K, l_d, D * K,
                              lower, Ls * K, 1, y, ldy, nullptr, batch, batch, nullptr, 0, 0, loss, nullptr, 0,
                              nullptr, nonfinite, workspace, workspace_bytes, as_stream(stream), f64::FinishHook());
}

extern "C" int bsig_mdn_head_nll_f64(const bsig_head_dims* dims, const bsig_f64_hyper* hyper,
                                     const double* head_out, int64_t ld, const double* y, int64_t ldy,
                                     const int32_t* y_rows, int64_t batch, int64_t norm_batch,
                                     const double* noise, uint64_t seed, uint64_t stream_id, double* loss,
                                     double* d_head_out, int32_t* nonfinite, void* workspace,
                                     size_t workspace_bytes, bsig_stream_t stream) {
  BSIG_REQUIRE(dims && head_out && y, "head_nll_f64: null pointer");
  BSIG_REQUIRE(ld >= bsig_head_width(dims), "head_nll_f64: ld too small");
  BSIG_REQUIRE(norm_batch >= 1, "head_nll_f64: norm_batch must be >= 1");
  const int64_t D = dims->out_dim, K = dims->n_comp;
  return f64::head_nll_launch(dims, f64::resolve_hyper(hyper, dims, nullptr), head_out, ld, head_out + K, ld,
                              head_out + K + D * K, ld, dims->full_cov ? head_out + K + 2 * D * K : nullptr, ld,
                              0, y, ldy, y_rows, batch, norm_batch, noise, seed, stream_id, loss, d_head_out, ld,
                              nullptr, nonfinite, workspace, workspace_bytes, as_stream(stream),
                              f64::FinishHook());
}
