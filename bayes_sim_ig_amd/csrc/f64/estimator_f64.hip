// Estimator and fit loop of the fp64 mode (include/bsig_f64.h): forward, NLL, backward and Adam as
// plain per-phase launches over the flat parameter layout of bsig_mdn_param_offsets, in doubles.
// No persistent kernel, no HIP graph, no factor rows, no data-parallel exchange.
#include "f64.h"

#include <algorithm>
#include <cmath>
#include <new>

namespace bsig {
namespace f64 {

struct Layout {
  int n_layers;
  int64_t in_dim[BSIG_MAX_HIDDEN + 1];
  int64_t w_off[BSIG_MAX_HIDDEN], b_off[BSIG_MAX_HIDDEN];
  int64_t feat_dim, nh, head_w_off, head_b_off, total;
};

static int make_layout(const bsig_mdn_cfg* c, Layout* L) {
  BSIG_REQUIRE(c, "cfg is null");
  int64_t offs[2 * (BSIG_MAX_HIDDEN + 4)];
  BSIG_TRY(bsig_mdn_param_offsets(c, offs, 2 * (BSIG_MAX_HIDDEN + 4)));   // (validates the cfg)
  L->n_layers = c->n_hidden;
  int64_t width = c->rff_feats > 0 ? c->rff_feats : c->input_dim;
  for (int l = 0; l < c->n_hidden; ++l) {
    L->in_dim[l] = width;
    L->w_off[l] = offs[2 * l]; L->b_off[l] = offs[2 * l + 1];
    width = c->hidden[l];
  }
  L->in_dim[c->n_hidden] = width;
  L->feat_dim = width;
  L->nh = bsig_head_width(&c->head);
  L->head_w_off = offs[2 * c->n_hidden]; L->head_b_off = offs[2 * c->n_hidden + 1];
  L->total = bsig_mdn_param_count(c);
  return BSIG_OK;
}

struct Scratch {
  double* feat;                     // [B, F] RFF features (MDRFF, projected per call)
  double* h[BSIG_MAX_HIDDEN];       // trunk activations [B, hidden_l]
  double* dz[2];                    // ping-pong [B, max hidden]
  double* o; double* d_o;           // [B, Nh] raw head outputs and their gradient
  double* head_ws; size_t head_ws_bytes;
  size_t total_bytes;
};

static void carve(const bsig_mdn_cfg* c, const Layout& L, int64_t B, void* base, Scratch* s) {
  size_t off = 0;
  auto take = [&](size_t doubles) {
    double* p = base ? reinterpret_cast<double*>(reinterpret_cast<char*>(base) + off) : nullptr;
    off += round_up<size_t>(doubles * sizeof(double), 256);
    return p;
  };
  s->feat = c->rff_feats > 0 ? take((size_t)B * c->rff_feats) : nullptr;
  int64_t hmax = 0;
  for (int l = 0; l < L.n_layers; ++l) {
    s->h[l] = take((size_t)B * c->hidden[l]);
    hmax = std::max<int64_t>(hmax, c->hidden[l]);
  }
  s->dz[0] = hmax ? take((size_t)B * hmax) : nullptr;
  s->dz[1] = hmax ? take((size_t)B * hmax) : nullptr;
  s->o = take((size_t)B * L.nh);
  s->d_o = take((size_t)B * L.nh);
  s->head_ws_bytes = bsig_head_workspace_bytes_f64(&c->head, B);
  s->head_ws = take(s->head_ws_bytes / sizeof(double) + 1);
  s->total_bytes = off;
}

// Where the input rows come from: row i reads x[(rows ? rows[i] : i) * ldx]; with `is_feat` the
// source already holds RFF features.
struct Inputs {
  const double* x = nullptr; int64_t ldx = 0;
  const int32_t* rows = nullptr;
  bool is_feat = false;
  const double* rff_coeff = nullptr; int64_t ld_coeff = 0; const double* rff_offset = nullptr;
};

static int rff_project(const bsig_mdn_cfg* c, const bsig_f64_hyper& hy, const Inputs& in, int64_t rows,
                       double* feats, hipStream_t st) {
  BSIG_REQUIRE(in.rff_coeff, "MDRFF needs rff_coeff");
  return bsig_rff_project_f64(in.x, in.ldx, in.rows, in.rff_coeff, in.ld_coeff, in.rff_offset, feats,
                              c->rff_feats, rows, c->input_dim,
                              c->rff_cos_only ? c->rff_feats : c->rff_feats / 2, hy.rff_scale,
                              c->rff_cos_only, st);
}

// trunk (or RFF) + heads -> o; leaves the activations in s.h / s.feat
static int forward_pass(const bsig_mdn_cfg* c, const bsig_f64_hyper& hy, const Layout& L, const double* params,
                        const Inputs& in, int64_t B, const Scratch& s, double* o, int64_t ldo, hipStream_t st) {
  const double* feat = in.x; int64_t ldf = in.ldx; const int32_t* rows = in.rows;
  if (c->rff_feats > 0 && !in.is_feat) {
    BSIG_TRY(rff_project(c, hy, in, B, s.feat, st));
    feat = s.feat; ldf = c->rff_feats; rows = nullptr;
  }
  for (int l = 0; l < L.n_layers; ++l) {   // nn.Linear + activation, mdnn.py:108
    Gemm g;
    g.a = feat; g.lda = ldf; g.a_rows = rows;
    g.b = params + L.w_off[l]; g.ldb = L.in_dim[l];
    g.c = s.h[l]; g.ldc = c->hidden[l];
    g.m = B; g.n = c->hidden[l]; g.k = L.in_dim[l];
    g.epilogue = BSIG_EPI_BIAS_ACT; g.act = c->activation; g.bias = params + L.b_off[l];
    BSIG_TRY(gemm_run(g, st));
    feat = s.h[l]; ldf = c->hidden[l]; rows = nullptr;
  }
  Gemm g;   // the four heads as one [Nh, F] product, mdnn.py:109-119
  g.a = feat; g.lda = ldf; g.a_rows = rows;
  g.b = params + L.head_w_off; g.ldb = L.feat_dim;
  g.c = o; g.ldc = ldo; g.m = B; g.n = L.nh; g.k = L.feat_dim;
  g.epilogue = BSIG_EPI_BIAS; g.bias = params + L.head_b_off;
  return gemm_run(g, st);
}

// dW[nout, nin] = dY^T X for one layer
static int weight_grad(const double* dy, int64_t nout, int64_t ld_dy, const double* xin, int64_t ldin,
                       const int32_t* xrows, int64_t nin, int64_t B, double* dw, hipStream_t st) {
  Gemm g;
  g.a = dy; g.lda = ld_dy; g.a_kmajor = 1;
  g.b = xin; g.ldb = ldin; g.b_kmajor = 1; g.b_rows = xrows;
  g.c = dw; g.ldc = nin; g.m = nout; g.n = nin; g.k = B;
  return gemm_run(g, st);
}

// backward from s.d_o (autograd through mdnn.py:108-119); the head bias gradients come from the
// head's finishing kernel
static int backward_pass(const bsig_mdn_cfg* c, const Layout& L, const double* params, const Inputs& in,
                         int64_t B, const Scratch& s, double* grads, hipStream_t st) {
  const double* feat; int64_t ldf; const int32_t* frows = nullptr;
  if (L.n_layers > 0) { feat = s.h[L.n_layers - 1]; ldf = c->hidden[L.n_layers - 1]; }
  else if (c->rff_feats > 0 && !in.is_feat) { feat = s.feat; ldf = c->rff_feats; }
  else { feat = in.x; ldf = in.ldx; frows = in.rows; }
  int cur = 0;
  if (L.n_layers > 0) {   // dz_L = (dO W_heads) * act'(h_L)
    Gemm g;
    g.a = s.d_o; g.lda = L.nh;
    g.b = params + L.head_w_off; g.ldb = L.feat_dim; g.b_kmajor = 1;
    g.c = s.dz[cur]; g.ldc = L.feat_dim; g.m = B; g.n = L.feat_dim; g.k = L.nh;
    g.epilogue = BSIG_EPI_MUL_DACT; g.act = c->activation; g.aux = feat; g.ldaux = ldf;
    BSIG_TRY(gemm_run(g, st));
  }
  BSIG_TRY(weight_grad(s.d_o, L.nh, L.nh, feat, ldf, frows, L.feat_dim, B, grads + L.head_w_off, st));
  for (int l = L.n_layers - 1; l >= 0; --l) {
    const int64_t hw = c->hidden[l];
    const double* xin; int64_t ldin; const int32_t* xrows = nullptr;
    if (l > 0) { xin = s.h[l - 1]; ldin = c->hidden[l - 1]; }
    else {   // the first layer reads the input rows themselves: there is no trunk on RFF features
      BSIG_REQUIRE(c->rff_feats == 0, "backward_f64: a trunk on RFF features (mdrff.py:18 has none)");
      xin = in.x; ldin = in.ldx; xrows = in.rows;
    }
    BSIG_TRY(colsum_launch(s.dz[cur], hw, B, hw, grads + L.b_off[l], st));
    if (l > 0) {   // dz_{l-1} = (dz_l W_l) * act'(h_{l-1})
      Gemm g;
      g.a = s.dz[cur]; g.lda = hw;
      g.b = params + L.w_off[l]; g.ldb = L.in_dim[l]; g.b_kmajor = 1;
      g.c = s.dz[cur ^ 1]; g.ldc = L.in_dim[l]; g.m = B; g.n = L.in_dim[l]; g.k = hw;
      g.epilogue = BSIG_EPI_MUL_DACT; g.act = c->activation; g.aux = xin; g.ldaux = ldin;
      BSIG_TRY(gemm_run(g, st));
    }
    BSIG_TRY(weight_grad(s.dz[cur], hw, hw, xin, ldin, xrows, L.in_dim[l], B, grads + L.w_off[l], st));
    cur ^= 1;
  }
  return BSIG_OK;
}

static int head_nll(const bsig_mdn_cfg* c, const bsig_f64_hyper& hy, const Layout& L, const Scratch& s,
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
  bsig::f64::Layout L;
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
  Scratch s;
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
  Scratch s;
  carve(cfg, L, batch, nullptr, &s);
  BSIG_REQUIRE(workspace && workspace_bytes >= s.total_bytes, "head_forward_f64: workspace %zu < %zu",
               workspace_bytes, s.total_bytes);
  carve(cfg, L, batch, workspace, &s);
  Inputs in;
  in.x = x; in.ldx = ldx; in.rows = x_rows;
  in.rff_coeff = rff_coeff; in.ld_coeff = ld_coeff; in.rff_offset = rff_offset;
  return forward_pass(cfg, resolve_hyper(hyper, &cfg->head, cfg), L, params, in, batch, s, head_out, ld_head,
                      as_stream(stream));
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
  Scratch s;
  carve(cfg, L, batch, nullptr, &s);
  BSIG_REQUIRE(workspace && workspace_bytes >= s.total_bytes, "loss_grad_f64: workspace %zu < %zu",
               workspace_bytes, s.total_bytes);
  carve(cfg, L, batch, workspace, &s);
  const bsig_f64_hyper hy = resolve_hyper(hyper, &cfg->head, cfg);
  hipStream_t st = as_stream(stream);
  Inputs in;
  in.x = x; in.ldx = ldx; in.rows = rows;
  in.rff_coeff = rff_coeff; in.ld_coeff = ld_coeff; in.rff_offset = rff_offset;
  BSIG_TRY(forward_pass(cfg, hy, L, params, in, batch, s, s.o, L.nh, st));
  BSIG_TRY(head_nll(cfg, hy, L, s, y, ldy, rows, batch, norm_batch, noise, seed, stream_id, loss, true,
                    grads + L.head_b_off, nonfinite, FinishHook(), st));
  return backward_pass(cfg, L, params, in, batch, s, grads, st);
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
  Scratch s;
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
    Inputs in;
    in.rff_coeff = b.rff_coeff; in.ld_coeff = b.ld_coeff; in.rff_offset = b.rff_offset;
    in.x = b.x_train; in.ldx = b.ldx_train;
    BSIG_TRY(rff_project(&p->cfg, p->hy, in, b.n_train, plan_feats(p), st));
    if (b.n_test > 0) {
      in.x = b.x_test; in.ldx = b.ldx_test;
      BSIG_TRY(rff_project(&p->cfg, p->hy, in, b.n_test, plan_feats(p) + b.n_train * p->cfg.rff_feats, st));
    }
  }
  return BSIG_OK;
}

static int fit64_update(bsig_fit64_plan* p, int64_t it, const Scratch& s, hipStream_t st) {
  const bsig_fit64_buffers& b = p->buf;
  const int32_t* ids = b.ids_table + it * p->batch;   // mdnn.py:219-222
  Inputs in;
  in.rows = ids;
  if (p->cfg.rff_feats > 0) { in.x = plan_feats(p); in.ldx = p->cfg.rff_feats; in.is_feat = true; }
  else { in.x = b.x_train; in.ldx = b.ldx_train; }
  FinishHook hook;
  hook.state = b.state; hook.kind = 1; hook.lr = p->hy.lr; hook.beta1 = p->hy.beta1; hook.beta2 = p->hy.beta2;
  BSIG_TRY(forward_pass(&p->cfg, p->hy, p->L, b.params, in, p->batch, s, s.o, p->L.nh, st));
  BSIG_TRY(head_nll(&p->cfg, p->hy, p->L, s, b.y_train, b.ldy_train, ids, p->batch, p->norm_batch, nullptr,
                    p->seed, p->rng_ctr++, b.train_loss + it, true, b.grads + p->L.head_b_off,
                    b.state + ST_FLAGS, hook, st));
  BSIG_TRY(backward_pass(&p->cfg, p->L, b.params, in, p->batch, s, b.grads, st));
  return adam_launch(b.params, b.grads, b.exp_avg, b.exp_avg_sq, p->L.total, p->hy.beta1, p->hy.beta2,
                     p->hy.adam_eps, 0.0, 1.0, st64_dbl(b.state), st);
}

static int fit64_eval(bsig_fit64_plan* p, int64_t e, const Scratch& s, hipStream_t st) {
  const bsig_fit64_buffers& b = p->buf;
  if (b.n_test <= 0) return BSIG_OK;   // (mean over an empty split: the caller reports NaN)
  Inputs in;
  if (p->cfg.rff_feats > 0) {
    in.x = plan_feats(p) + b.n_train * p->cfg.rff_feats; in.ldx = p->cfg.rff_feats; in.is_feat = true;
  } else { in.x = b.x_test; in.ldx = b.ldx_test; }
  FinishHook hook;
  hook.state = b.state; hook.kind = 2;
  BSIG_TRY(forward_pass(&p->cfg, p->hy, p->L, b.params, in, b.n_test, s, s.o, p->L.nh, st));
  return head_nll(&p->cfg, p->hy, p->L, s, b.y_test, b.ldy_test, nullptr, b.n_test, b.n_test, nullptr, p->seed,
                  p->rng_ctr++, b.test_loss + e, false, nullptr, b.state + ST_FLAGS, hook, st);
}

extern "C" int bsig_fit64_run(bsig_fit64_plan* p, int64_t n_updates, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit64_run");
  BSIG_REQUIRE(p && p->bound, "fit64_run: plan not bound");
  BSIG_REQUIRE(n_updates >= 0 && n_updates <= p->n_updates, "fit64_run: n_updates %lld exceeds the plan's %lld",
               (long long)n_updates, (long long)p->n_updates);
  hipStream_t st = as_stream(stream);
  Scratch s;
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
