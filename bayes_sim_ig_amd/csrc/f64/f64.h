// Internal interfaces of the fp64 mode (include/bsig_f64.h): launchers shared between its files.
#pragma once
#include "../common.h"
#include "../fit_protocol.h"
#include "../../../include/bsig_f64.h"

namespace bsig {
namespace f64 {

struct Gemm {
  const double* a = nullptr; int64_t lda = 0; int a_kmajor = 0; const int32_t* a_rows = nullptr;
  const double* b = nullptr; int64_t ldb = 0; int b_kmajor = 0; const int32_t* b_rows = nullptr;
  double* c = nullptr; int64_t ldc = 0;
  int64_t m = 0, n = 0, k = 0;
  int epilogue = BSIG_EPI_NONE, act = BSIG_ACT_IDENTITY;
  const double* bias = nullptr; const double* aux = nullptr; int64_t ldaux = 0;
  double alpha = 1.0;
};
int gemm_run(const Gemm& g, hipStream_t st);

// the hyper-parameters of a call: the caller's doubles, or the widened floats of the structs
inline bsig_f64_hyper resolve_hyper(const bsig_f64_hyper* h, const bsig_head_dims* d, const bsig_mdn_cfg* c) {
  if (h) return *h;
  bsig_f64_hyper r{};
  if (c) { r.lr = c->lr; r.beta1 = c->beta1; r.beta2 = c->beta2; r.adam_eps = c->adam_eps; r.rff_scale = c->rff_scale; }
  if (d) { r.eps_noise = d->eps_noise; r.min_weight = d->min_weight; r.ll_limit = d->ll_limit; }
  return r;
}

// (the engine's 32-word state block: fit_protocol.h)
struct FinishHook {
  int32_t* state = nullptr; int kind = 0;   // 1: end of an update's forward half, 2: end of an evaluation
  double lr = 0, beta1 = 0, beta2 = 0;
};

// mdn_nll_f64_kernel + finish.  Segments as in the fp32 launcher: logits / weights, mu, pre_diag /
// sigma, strict-lower entries, each with its pitch; from_tuple: weights and sigma are final.
int head_nll_launch(const bsig_head_dims* dims, const bsig_f64_hyper& hy, const double* seg_w, int64_t ld_w,
                    const double* seg_mu, int64_t ld_mu, const double* seg_sg, int64_t ld_sg,
                    const double* seg_lo, int64_t ld_lo, int from_tuple, const double* y, int64_t ldy,
                    const int32_t* y_rows, int64_t batch, int64_t norm_batch, const double* noise,
                    uint64_t seed, uint64_t stream_id, double* loss, double* d_out, int64_t ld_dout,
                    double* colsum_out, int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                    hipStream_t st, const FinishHook& hook);

int adam_launch(double* p, const double* g, double* m, double* v, int64_t n, double beta1, double beta2,
                double eps, double step_size, double bc2_sqrt, const double* dyn, hipStream_t st);
int colsum_launch(const double* x, int64_t ld, int64_t rows, int64_t cols, double* out, hipStream_t st);

}  // namespace f64
}  // namespace bsig
