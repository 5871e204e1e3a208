// Estimator and fit loop of the fp64 mode (include/bsig_f64.h): forward, NLL, backward and Adam as
// plain per-phase launches over the flat parameter layout of bsig_mdn_param_offsets, in doubles.
// No persistent kernel, no HIP graph, no factor rows, no data-parallel exchange.  The layout, the workspace carve
// and the forward / backward sequence are the float estimator's, instantiated for double (../network_pass.h).
#include "../network_pass.h"

#include <algorithm>
#include <cmath>
#include <new>

namespace bsig {
namespace f64 {

static int head_nll(const bsig_mdn_cfg* c, const bsig_f64_hyper& hy, const Layout& L, const Scratch<double>& s,
                    const double* y, int64_t ldy, const int32_t* y_rows, int64_t B, int64_t norm_batch,
                    const double* noise, uint64_t seed, uint64_t stream_id, double* loss, bool bwd,
                    double* head_bias_grad, int32_t* nonfinite, const FinishHook& hook, hipStream_t st) {
  const int64_t D = c->head.out_dim, K = c->head.n_comp;
  return head_nll_launch(&c->head, hy, s.o, L.nh, s.o + K, L.nh, s.o + K + D * K, L.nh,
                         c->head.full_cov ? s.o + K + 2 * D * K : nullptr, L.nh, 0, y, ldy, y_rows, B,
                         norm_batch, noise, seed, stream_id, loss, bwd ? s.d_o : nullptr, L.nh,
                         bwd ? head_bias_grad : nullptr, nonfinite, s.head_ws, s.head_ws_bytes, st, hook);
}

// Start of a run_training call: the state block of a fresh optimizer (mdnn.py:203) and its zeroed moments
__global__ __launch_bounds__(256) void fit64_begin_kernel(int32_t* state, double* m, double* v, int64_t n) {
  if (blockIdx.x == 0) {
    if (threadIdx.x < ST64_WORDS) state[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) st64_begin(state);
  }
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    m[i] = 0.0; v[i] = 0.0;
  }
}

// [train_loss at the logging points | test_loss | flag word] of one call, for its single read-back
__global__ void pack_logs_f64_kernel(const double* train_loss, const double* test_loss, const int32_t* state,
                                     int n_updates, int n_evals, double* out) {
  pack_call_logs(train_loss, test_loss, state, n_updates, eval_every(n_updates), n_evals, out, (int)threadIdx.x,
                 (int)blockDim.x);
}

}  // namespace f64
}  // namespace bsig

struct bsig_fit64_plan {
  bsig_mdn_cfg cfg;
  bsig_f64_hyper hy;
  bsig::Layout L;
  int64_t batch, max_train, max_test, n_updates;
  bsig_fit64_buffers buf;
  bool bound;
  uint64_t seed, rng_ctr;   // jitter: one Philox stream per head launch of the call, from 1
  int64_t norm_batch;
  size_t scratch_bytes, ws_bytes;
};

using namespace bsig;
using namespace bsig::f64;

extern "C" size_t bsig_mdn_workspace_bytes_f64(const bsig_mdn_cfg* cfg, int64_t max_batch) {
  Layout L;
  if (make_layout(cfg, &L) != BSIG_OK) return 0;
  Scratch<double> s;
  carve(cfg, L, std::max<int64_t>(max_batch, 1), nullptr, &s);
  return s.total_bytes;
}

extern "C" int bsig_mdn_head_forward_f64(const bsig_mdn_cfg* cfg, const bsig_f64_hyper* hyper,
                                         const double* params, const double* rff_coeff, int64_t ld_coeff,
                                         const double* rff_offset, const double* x, int64_t ldx,
                                         const int32_t* x_rows, int64_t batch, double* head_out,
                                         int64_t ld_head, void* workspace, size_t workspace_bytes,
                                         bsig_stream_t stream) {
  Layout L;
  BSIG_TRY(make_layout(cfg, &L));
  BSIG_REQUIRE(params && x && head_out && batch >= 1, "head_forward_f64: bad args");
  BSIG_REQUIRE(ldx >= cfg->input_dim && ld_head >= L.nh, "head_forward_f64: leading dims too small");
  Scratch<double> s;
  carve(cfg, L, batch, nullptr, &s);
  BSIG_REQUIRE(workspace && workspace_bytes >= s.total_bytes, "head_forward_f64: workspace %zu < %zu",
               workspace_bytes, s.total_bytes);
  carve(cfg, L, batch, workspace, &s);
  Inputs<double> in;
  in.x = x; in.ldx = ldx; in.rows = x_rows;
  in.rff_coeff = rff_coeff; in.ld_coeff = ld_coeff; in.rff_offset = rff_offset;
  return forward_pass(cfg, L, params, in, resolve_hyper(hyper, &cfg->head, cfg).rff_scale, batch, s, head_out,
                      ld_head, as_stream(stream));
}

extern "C" int bsig_mdn_loss_grad_f64(const bsig_mdn_cfg* cfg, const bsig_f64_hyper* hyper,
                                      const double* params, const double* rff_coeff, int64_t ld_coeff,
                                      const double* rff_offset, const double* x, int64_t ldx,
                                      const double* y, int64_t ldy, const int32_t* rows, int64_t batch,
                                      int64_t norm_batch, const double* noise, uint64_t seed,
                                      uint64_t stream_id, double* grads, double* loss, int32_t* nonfinite,
                                      void* workspace, size_t workspace_bytes, bsig_stream_t stream) {
  Layout L;
  BSIG_TRY(make_layout(cfg, &L));
  BSIG_REQUIRE(params && x && y && grads && batch >= 1 && norm_batch >= 1, "loss_grad_f64: bad args");
  BSIG_REQUIRE(ldx >= cfg->input_dim && ldy >= cfg->head.out_dim, "loss_grad_f64: leading dims");
  Scratch<double> s;
  carve(cfg, L, batch, nullptr, &s);
  BSIG_REQUIRE(workspace && workspace_bytes >= s.total_bytes, "loss_grad_f64: workspace %zu < %zu",
               workspace_bytes, s.total_bytes);
  carve(cfg, L, batch, workspace, &s);
  const bsig_f64_hyper hy = resolve_hyper(hyper, &cfg->head, cfg);
  hipStream_t st = as_stream(stream);
  Inputs<double> in;
  in.x = x; in.ldx = ldx; in.rows = rows;
  in.rff_coeff = rff_coeff; in.ld_coeff = ld_coeff; in.rff_offset = rff_offset;
  BSIG_TRY(forward_pass(cfg, L, params, in, hy.rff_scale, batch, s, s.o, L.nh, st));
  BSIG_TRY(head_nll(cfg, hy, L, s, y, ldy, rows, batch, norm_batch, noise, seed, stream_id, loss, true,
                    grads + L.head_b_off, nonfinite, f64::FinishHook(), st));
  return backward_pass(cfg, L, const_cast<double*>(params), in, 0, batch, s, grads, nullptr, st);
}

extern "C" int bsig_fit64_create(const bsig_mdn_cfg* cfg, const bsig_f64_hyper* hyper, int64_t batch,
                                 int64_t max_train_rows, int64_t max_test_rows, int64_t n_updates,
                                 bsig_fit64_plan** plan) {
  BSIG_REQUIRE(plan, "fit64_create: null plan pointer");
  *plan = nullptr;
  Layout L;
  BSIG_TRY(make_layout(cfg, &L));
  BSIG_REQUIRE(batch >= 1 && max_train_rows >= 0 && max_test_rows >= 0 && n_updates >= 0,
               "fit64_create: bad sizes");
  BSIG_REQUIRE(bsig_head_workspace_bytes_f64(&cfg->head, 1) > 0, "fit64_create: head shape not covered");
  bsig_fit64_plan* p = new (std::nothrow) bsig_fit64_plan();
  BSIG_REQUIRE(p, "fit64_create: out of host memory");
  p->cfg = *cfg; p->hy = resolve_hyper(hyper, &cfg->head, cfg); p->L = L;
  p->batch = batch; p->max_train = max_train_rows; p->max_test = max_test_rows; p->n_updates = n_updates;
  p->bound = false; p->seed = 0; p->rng_ctr = 1; p->norm_batch = batch;
  Scratch<double> s;
  carve(cfg, L, std::max<int64_t>(batch, std::max<int64_t>(max_test_rows, 1)), nullptr, &s);
  p->scratch_bytes = s.total_bytes;
  // an MDRFF keeps one feature row per row of the call (rff.py:128-132 is a pure function of the row)
  p->ws_bytes = s.total_bytes +
      (cfg->rff_feats > 0 ? (size_t)(max_train_rows + max_test_rows) * cfg->rff_feats * sizeof(double) : 0);
  *plan = p;
  return BSIG_OK;
}

extern "C" void bsig_fit64_destroy(bsig_fit64_plan* p) { delete p; }

extern "C" size_t bsig_fit64_workspace_bytes(const bsig_fit64_plan* p) { return p ? p->ws_bytes : 0; }

extern "C" int bsig_fit64_bind(bsig_fit64_plan* p, const bsig_fit64_buffers* b, int flags) {
  BSIG_REQUIRE(p && b, "fit64_bind: null pointer");
  if (flags & BSIG_FIT_SPLIT_ADAM) {
    set_error("fit64_bind: the fp64 mode has no data-parallel exchange (BSIG_FIT_SPLIT_ADAM)");
    return BSIG_EUNSUPPORTED;
  }
  if (b->x_kind != BSIG_X_ROWS) {
    set_error("fit64_bind: the fp64 mode takes summary rows only, not cross-correlation factor rows");
    return BSIG_EUNSUPPORTED;
  }
  BSIG_REQUIRE(b->params && b->grads && b->exp_avg && b->exp_avg_sq && b->state, "fit64_bind: null buffer");
  BSIG_REQUIRE(b->x_train && b->y_train && b->ids_table && b->train_loss && b->test_loss,
               "fit64_bind: null training buffer");
  BSIG_REQUIRE(b->n_train >= 1 && b->n_test >= 0, "fit64_bind: bad row counts");
  BSIG_REQUIRE(b->n_test <= p->max_test, "fit64_bind: %lld held-out rows exceed the plan's %lld",
               (long long)b->n_test, (long long)p->max_test);
  BSIG_REQUIRE(p->cfg.rff_feats == 0 || b->n_train <= p->max_train,
               "fit64_bind: %lld training rows exceed the plan's %lld", (long long)b->n_train,
               (long long)p->max_train);
  BSIG_REQUIRE(b->n_test == 0 || (b->x_test && b->y_test), "fit64_bind: null held-out buffer");
  BSIG_REQUIRE(b->ldx_train >= p->cfg.input_dim && b->ldy_train >= p->cfg.head.out_dim &&
               (b->n_test == 0 || (b->ldx_test >= p->cfg.input_dim && b->ldy_test >= p->cfg.head.out_dim)),
               "fit64_bind: leading dims too small");
  BSIG_REQUIRE(p->cfg.rff_feats == 0 || b->rff_coeff, "fit64_bind: MDRFF needs rff_coeff");
  BSIG_REQUIRE(b->workspace && b->workspace_bytes >= p->ws_bytes, "fit64_bind: workspace %zu < %zu",
               b->workspace_bytes, p->ws_bytes);
  p->buf = *b;
  p->bound = true;
  return BSIG_OK;
}

static double* plan_feats(const bsig_fit64_plan* p) {
  return reinterpret_cast<double*>(reinterpret_cast<char*>(p->buf.workspace) + p->scratch_bytes);
}

extern "C" int bsig_fit64_begin(bsig_fit64_plan* p, uint64_t seed, int64_t norm_batch, bsig_stream_t stream) {
  BSIG_REQUIRE(p && p->bound, "fit64_begin: plan not bound");
  BSIG_REQUIRE(norm_batch >= 1, "fit64_begin: norm_batch must be >= 1");
  hipStream_t st = as_stream(stream);
  const bsig_fit64_buffers& b = p->buf;
  p->seed = seed; p->rng_ctr = 1; p->norm_batch = norm_batch;
  const int blocks = (int)std::min<int64_t>(ceil_div<int64_t>(std::max<int64_t>(p->L.total, 1), 256), 1024);
  hipLaunchKernelGGL(fit64_begin_kernel, dim3(blocks), dim3(256), 0, st, b.state, b.exp_avg, b.exp_avg_sq,
                     p->L.total);
  BSIG_CHECK_LAUNCH("fit64_begin");
  if (p->cfg.rff_feats > 0) {   // the call's rows, projected once: training rows, then the held-out rows
    Inputs<double> in;
    in.rff_coeff = b.rff_coeff; in.ld_coeff = b.ld_coeff; in.rff_offset = b.rff_offset;
    in.x = b.x_train; in.ldx = b.ldx_train;
    BSIG_TRY(rff_project(&p->cfg, in, p->hy.rff_scale, b.n_train, plan_feats(p), nullptr, 0, 0, st));
    if (b.n_test > 0) {
      in.x = b.x_test; in.ldx = b.ldx_test;
      BSIG_TRY(rff_project(&p->cfg, in, p->hy.rff_scale, b.n_test, plan_feats(p) + b.n_train * p->cfg.rff_feats,
                           nullptr, 0, 0, st));
    }
  }
  return BSIG_OK;
}

static int fit64_update(bsig_fit64_plan* p, int64_t it, const Scratch<double>& s, hipStream_t st) {
  const bsig_fit64_buffers& b = p->buf;
  const int32_t* ids = b.ids_table + it * p->batch;   // mdnn.py:219-222
  Inputs<double> in;
  in.rows = ids;
  if (p->cfg.rff_feats > 0) { in.x = plan_feats(p); in.ldx = p->cfg.rff_feats; in.is_feat = true; }
  else { in.x = b.x_train; in.ldx = b.ldx_train; }
  f64::FinishHook hook;
  hook.state = b.state; hook.kind = 1; hook.lr = p->hy.lr; hook.beta1 = p->hy.beta1; hook.beta2 = p->hy.beta2;
  BSIG_TRY(forward_pass(&p->cfg, p->L, b.params, in, p->hy.rff_scale, p->batch, s, s.o, p->L.nh, st));
  BSIG_TRY(head_nll(&p->cfg, p->hy, p->L, s, b.y_train, b.ldy_train, ids, p->batch, p->norm_batch, nullptr,
                    p->seed, p->rng_ctr++, b.train_loss + it, true, b.grads + p->L.head_b_off,
                    b.state + ST_FLAGS, hook, st));
  BSIG_TRY(backward_pass(&p->cfg, p->L, b.params, in, 0, p->batch, s, b.grads, nullptr, st));
  return adam_launch(b.params, b.grads, b.exp_avg, b.exp_avg_sq, p->L.total, p->hy.beta1, p->hy.beta2,
                     p->hy.adam_eps, 0.0, 1.0, st64_dbl(b.state), st);
}

static int fit64_eval(bsig_fit64_plan* p, int64_t e, const Scratch<double>& s, hipStream_t st) {
  const bsig_fit64_buffers& b = p->buf;
  if (b.n_test <= 0) return BSIG_OK;   // (mean over an empty split: the caller reports NaN)
  Inputs<double> in;
  if (p->cfg.rff_feats > 0) {
    in.x = plan_feats(p) + b.n_train * p->cfg.rff_feats; in.ldx = p->cfg.rff_feats; in.is_feat = true;
  } else { in.x = b.x_test; in.ldx = b.ldx_test; }
  f64::FinishHook hook;
  hook.state = b.state; hook.kind = 2;
  BSIG_TRY(forward_pass(&p->cfg, p->L, b.params, in, p->hy.rff_scale, b.n_test, s, s.o, p->L.nh, st));
  return head_nll(&p->cfg, p->hy, p->L, s, b.y_test, b.ldy_test, nullptr, b.n_test, b.n_test, nullptr, p->seed,
                  p->rng_ctr++, b.test_loss + e, false, nullptr, b.state + ST_FLAGS, hook, st);
}

extern "C" int bsig_fit64_run(bsig_fit64_plan* p, int64_t n_updates, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit64_run");
  BSIG_REQUIRE(p && p->bound, "fit64_run: plan not bound");
  BSIG_REQUIRE(n_updates >= 0 && n_updates <= p->n_updates, "fit64_run: n_updates %lld exceeds the plan's %lld",
               (long long)n_updates, (long long)p->n_updates);
  hipStream_t st = as_stream(stream);
  Scratch<double> s;
  carve(&p->cfg, p->L, std::max<int64_t>(p->batch, std::max<int64_t>(p->max_test, 1)), p->buf.workspace, &s);
  const int64_t every = eval_every(n_updates);
  int64_t e = 0;
  for (int64_t it = 0; it < n_updates; ++it) {
    BSIG_TRY(fit64_update(p, it, s, st));
    if (is_logging_point(it, n_updates, every)) BSIG_TRY(fit64_eval(p, e++, s, st));
  }
  return BSIG_OK;
}

extern "C" int bsig_fit64_pack_logs(bsig_fit64_plan* p, int64_t n_updates, int64_t n_evals, double* out,
                                    bsig_stream_t stream) {
  BSIG_REQUIRE(p && p->bound && out, "fit64_pack_logs: plan not bound / null");
  BSIG_REQUIRE(n_updates >= 0 && n_updates <= p->n_updates, "fit64_pack_logs: bad n_updates");
  BSIG_REQUIRE(n_evals == count_logging_points(n_updates),
               "fit64_pack_logs: the caller counts %lld logging points in %lld updates, the fit loop ran %lld",
               (long long)n_evals, (long long)n_updates, (long long)count_logging_points(n_updates));
  hipLaunchKernelGGL(pack_logs_f64_kernel, dim3(1), dim3(64), 0, as_stream(stream), p->buf.train_loss,
                     p->buf.test_loss, p->buf.state, (int)n_updates, (int)n_evals, out);
  BSIG_CHECK_LAUNCH("pack_logs_f64");
  return BSIG_OK;
}
