// MDNN / MDRFF estimator passes and the fit engine.
//   head forward   : mdnn.py:108-119 (trunk + heads) / mdrff.py:28-30 (RFF first)
//   loss + grad    : mdnn.py:229-233 (forward, mdn_loss_fn, backward)
//   fit engine     : mdnn.py:228-242 — one update (minibatch gather, forward,
//                    NLL, backward, Adam) is captured once in a HIP graph and
//                    replayed per step with no host synchronisation.
//
// Replay without per-step host work: everything that changes between updates
// is resolved on the device from a 16-word state block.  The step counter is
// advanced by the single-writer hook of the head's finishing kernel, which sits
// between the forward and the backward half of the update: forward kernels read
// `step`, backward kernels read `step - 1`.  Minibatch rows are looked up in the
// [n_updates, B] id table (drawn on the host in the reference's numpy-RNG
// order, mdnn.py:219-222) at row offset step * B by the GEMM loaders and the
// head kernel themselves — no gather kernel, no copies.
//
// MDRFF: the RFF features of a minibatch row depend only on the row, not on
// the weights, so the projections of ALL minibatches of a run_training call
// (n_updates * B gathered rows, plus the held-out rows once per evaluation)
// are computed up front by ONE large fp32-MFMA GEMM — the same rows, the same
// arithmetic and the same number of row visits as the reference's per-step
// `rff.to_features(x_batch)` (mdrff.py:29), at large-GEMM efficiency instead of
// 100 latency-bound M=100 launches.  The per-step graph then starts at the heads.
//
// Single rank: Adam is fused into the epilogue of each dW GEMM (weights and,
// via the column-0 threads, the layer's bias), so an update has no optimizer
// kernel.  Data parallel: gradients go to the flat buffer, the caller
// all-reduces it, then one flat Adam kernel runs (bsig_fit_grad / _apply).
//
// The parameter layout, the workspace carve and the forward / backward sequence of products are
// shared with the fp64 mode: network_pass.h.
#include "comm.h"
#include "network_pass.h"
#include "persist.h"
#include "persist_mdnn.h"
#include "fit_protocol.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

namespace bsig {

static int head_nll(const bsig_mdn_cfg* c, const Layout& L, const Scratch<float>& s, const float* y,
                    int64_t ldy, const int32_t* y_rows, int64_t B, int64_t norm_batch,
                    const float* noise, uint64_t seed, uint64_t stream_id,
                    const uint64_t* dyn_rng, float* loss, const int32_t* loss_slot, bool bwd,
                    float* head_bias_grad, int32_t* nonfinite, const HeadDyn* dyn,
                    hipStream_t st, HeadBiasPartials* bias_partials = nullptr) {
  const int64_t D = c->head.out_dim, K = c->head.n_comp;
  return mdn_head_nll_launch(&c->head, s.o, s.ld_o, s.o + K, s.ld_o, s.o + K + D * K, s.ld_o,
                             c->head.full_cov ? s.o + K + 2 * D * K : nullptr, s.ld_o, 0, y, ldy,
                             y_rows, B, norm_batch, noise, seed, stream_id, dyn_rng, loss,
                             loss_slot, bwd ? s.d_o : nullptr, s.ld_o,
                             bwd ? head_bias_grad : nullptr, nonfinite, s.head_ws,
                             s.head_ws_bytes, st, dyn, bias_partials);
}

// ---- fit engine -----------------------------------------------------------
// (the device state block, the logging schedule and the stream numbering: fit_protocol.h)

// Start of a run_training call: reset the state block and clear what the call needs cleared
// (a fresh optimizer's moments, mdnn.py:203, unless the persistent kernels start them in
// registers; the persistent kernels' flags / granules) -- ONE launch, no runtime memsets.
struct BeginZero { float4* ptr[4]; int64_t n4[4]; };
__global__ __launch_bounds__(256) void fit_begin_kernel(int32_t* state, uint64_t seed, BeginZero z) {
  if (blockIdx.x == 0) {
    if (threadIdx.x < ST_WORDS) state[threadIdx.x] = 0;
    __syncthreads();
    if (threadIdx.x == 0) st_begin(state, seed);
  }
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int r = 0; r < 4; ++r)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < z.n4[r];
         i += (int64_t)gridDim.x * blockDim.x)
      z.ptr[r][i] = zero;
}

__global__ void iota_mod_kernel(int32_t* out, int n, int mod) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
    out[i] = i % mod;
}

}  // namespace bsig

using namespace bsig;

struct bsig_fit_plan {
  bsig_mdn_cfg cfg;
  Layout L;
  int64_t batch, max_test, n_updates, n_evals;
  bool hoist;                  // RFF projection once per run_training call
  bool feat_cache;             // ... may keep one feature row per training row (feat_cache_applies; BSIG_NO_FEAT_CACHE)
  bool feat_unique;            // ... of the distinct training rows (else of every gathered minibatch row)
  bool feats_preloaded;        // ... already handed over by the caller (bsig_fit_set_features)
  const float* ext_feats;      // ... and read where they lie (this call only) instead of copied
  int64_t feat_rows;           // rows of the hoisted feature block (+ max_test)
  int64_t max_train;           // caller's bound on n_train (0: none)
  bsig_fit_buffers buf;
  bool bound;
  int64_t norm_batch;
  size_t train_ws_bytes, test_ws_bytes, feats_bytes, big_gemm_ws_bytes, iota_bytes;
  bool use_graph, split_adam;
  int matmul;                  // BSIG_PLAN_SPLIT_BF16: the matmul precision of every gemm_run product of this plan

  PersistEngine eng;           // the persistent update engine resolved at creation (persist.h) ...
  UGeom ug; MdnnGeom mg;       // ... its geometry (linear heads / two-layer MDNN)
  bool eng_off;                // ... does not run this binding's updates (a streamed first layer bound
                               // to rows it does not take): the per-phase kernels do -- engine()
  int dp_evals_done;           // data-parallel + in-launch evaluations: bsig_fit_eval calls so far
  bool resident_ran;           // a resident data-parallel call ran since bsig_fit_begin (its workgroup count word is used up)
  bool adam_pending;           // ... data-parallel: the Adam step on the reduced gradients is
                               // taken by the next launch (or flushed before an evaluation)
  // single rank, linear heads: the held-out evaluations run in kernels behind the update launch, from weight
  // snapshots (persist.h: DeferredEval) -- unless BSIG_EVAL_IN_LAUNCH=1 or the snapshots would exceed their cap
  bool eval_deferred;
  bsig::DeferredEval deferred;
  int64_t n_deferred, n_in_launch;   // (bsig_debug_fit_deferred) launches of a single rank's whole call, either way
  hipStream_t cap_stream;
  hipGraphExec_t g_step, g_grad, g_apply, g_eval;
  bool graphs_ready;           // ensure_graphs has run for this binding (g_eval may legitimately be absent)
  const float* graph_feats;    // the feature block the captured graphs read (kernel argument)
  // data-parallel rank in the persistent kernel of the linear heads: one steady-state update
  // (launch with the pending Adam step -> ncclAllReduce of the gradients) as ONE graph
  hipGraphExec_t g_dp; const bsig_comm* g_dp_comm;
  int g_dp_state;              // 0: not tried, 1: captured, -1: capture failed (g_dp_error), -2: not applicable
  char g_dp_error[200];
};

namespace bsig {

static size_t plan_ws_bytes(const bsig_fit_plan* p) {
  return p->train_ws_bytes + p->test_ws_bytes + p->feats_bytes + p->big_gemm_ws_bytes +
         p->iota_bytes + p->eng.workspace_bytes;
}

// the persistent engine that runs the bound plan's updates: 0 none (per-phase kernels), 1 linear heads, 2 MDNN
static int engine(const bsig_fit_plan* p) { return p->eng_off ? 0 : p->eng.kind; }

// Do a call's held-out evaluations run inside the persistent launches?  dp: a data-parallel rank's
// launches (one per update), else a single rank's call (or a resident data-parallel one).  A streamed
// first layer evaluates only from the held-out pairs' factor rows (test_factors).  (The plan's engine;
// whether it runs the bound updates and whether the binding holds held-out rows, the callers ask.)
static bool evals_in_launch(const bsig_fit_plan* p, bool dp, bool test_factors) {
  return (dp ? p->eng.eval_dp : p->eng.eval_single) && (!p->eng.streams || test_factors);
}

// Does a call over n_train training rows keep one projected feature row per training row (the
// feature cache: the call visits its rows more than once)?
static bool feat_cache_applies(const bsig_fit_plan* p, int64_t n_train) {
  return p->hoist && p->feat_cache && n_train <= p->n_updates * p->batch;
}

struct PlanMem { Scratch<float> tr, te; float* feats; float* big_ws; int32_t* iota; void* persist_ws; };

// fit_begin_kernel clears up to four regions: the persistent kernels' exchange areas (2), the Adam
// moments (2; not where a single-rank persistent plan starts them in registers) -- and, where that
// leaves room, the combine tickets of the two scratch areas (gemm_wide.h; else: no combine)
static int begin_regions(const bsig_fit_plan* p) {
  const bool pers = engine(p) != 0;
  return (pers ? 2 : 0) + (!(pers && !p->split_adam) ? 2 : 0);
}
static bool tickets_zeroed(const bsig_fit_plan* p) { return begin_regions(p) + 2 <= 4; }

static void plan_mem(const bsig_fit_plan* p, PlanMem* m) {
  char* base = reinterpret_cast<char*>(p->buf.workspace);
  carve(&p->cfg, p->L, p->batch, base, &m->tr);
  base += p->train_ws_bytes;
  carve(&p->cfg, p->L, std::max<int64_t>(p->max_test, 1), base, &m->te);
  base += p->test_ws_bytes;
  m->feats = p->ext_feats ? const_cast<float*>(p->ext_feats) : reinterpret_cast<float*>(base);
  base += p->feats_bytes;
  m->big_ws = reinterpret_cast<float*>(base); base += p->big_gemm_ws_bytes;
  m->iota = reinterpret_cast<int32_t*>(base); base += p->iota_bytes;
  m->persist_ws = base;
  if (!tickets_zeroed(p)) m->tr.tickets = m->te.tickets = nullptr;
  m->tr.math = m->te.math = p->matmul;
}

static PersistShape persist_shape(const bsig_fit_plan* p) {
  return PersistShape{(int)p->batch, (int)p->L.feat_dim, p->cfg.head.out_dim, p->cfg.head.n_comp,
                      (int)std::min<int64_t>(p->max_test, 1 << 20)};
}

static PersistMdnnShape persist_mdnn_shape(const bsig_fit_plan* p) {
  const bsig_mdn_cfg& c = p->cfg;
  return PersistMdnnShape{(int)p->batch, c.input_dim, c.n_hidden > 0 ? c.hidden[0] : 0,
                          c.n_hidden > 1 ? c.hidden[1] : 0, c.activation, c.head.out_dim,
                          c.head.n_comp, c.head.full_cov,
                          (int)std::min<int64_t>(p->max_test, 1 << 20)};
}

// n consecutive updates in the plan's persistent kernel.  Data-parallel plans (split_adam): ONE
// update whose gradients go to the flat gradient buffer, after the pending Adam step of the previous
// one; n = 0 flushes that step.  eval_total > 0: the launch belongs to a call of eval_total updates
// whose held-out evaluations run inside the launches.  xr: the whole call in one launch, resident
// across the exchange (persist.h).  blk: a block of chunks in one launch (bsig_fit_run_block), n the updates of a chunk.
struct BlockRun {
  const float* feats; int64_t ld_feats; const float* y; int64_t ldy; const int32_t* ids;
  const bsig_fit_chunk* chunks; int n_chunks, max_test, total_updates; float* train_loss; float* test_loss;
};
static int enqueue_persistent(bsig_fit_plan* p, int n, hipStream_t st, int eval_total = 0,
                              const CommXr* xr = nullptr, const BlockRun* blk = nullptr, bool deferred = false) {
  PlanMem m; plan_mem(p, &m);
  const bsig_fit_buffers& b = p->buf;
  PersistCommon c;
  c.y = b.y_train; c.ldy = b.ldy_train; c.ids = b.ids_table;
  c.params = b.params; c.exp_avg = b.exp_avg; c.exp_avg_sq = b.exp_avg_sq;
  c.state = b.state; c.train_loss = b.train_loss;
  c.workspace = m.persist_ws; c.workspace_bytes = p->eng.workspace_bytes;
  if (p->split_adam) {
    c.grads = b.grads; c.adam_pending = p->adam_pending ? 1 : 0;
    p->adam_pending = false;
  }
  if (xr) { c.xr_ready = xr->ready; c.xr_done = xr->done; c.xr_base = xr->base; c.n_total = n; }
  if (eval_total > 0) {
    c.do_eval = 1; c.n_total = eval_total; c.eval_every = eval_every(eval_total);
    c.n_test = (int)b.n_test;
    c.y_test = b.y_test; c.ldy_test = b.ldy_test; c.test_loss = b.test_loss;
  }
  c.hy.lr = p->cfg.lr; c.hy.beta1 = p->cfg.beta1; c.hy.beta2 = p->cfg.beta2;
  c.hy.adam_eps = p->cfg.adam_eps; c.hy.eps_noise = p->cfg.head.eps_noise;
  c.hy.min_weight = p->cfg.head.min_weight; c.hy.ll_limit = p->cfg.head.ll_limit;
  c.hy.norm_batch = p->norm_batch;
  if (engine(p) == 1) {
    PersistBuffers pb;
    static_cast<PersistCommon&>(pb) = c;
    pb.feats = m.feats; pb.ld_feats = p->cfg.rff_feats;
    pb.feat_ids = p->feat_unique ? b.ids_table : nullptr;
    pb.w_off = p->L.head_w_off; pb.b_off = p->L.head_b_off;
    pb.eval_row0 = p->feat_unique ? b.n_train : p->n_updates * p->batch;  // as eval_inputs()
    if (blk) {
      pb.feats = blk->feats; pb.ld_feats = blk->ld_feats; pb.feat_ids = blk->ids; pb.eval_row0 = 0;
      pb.y = blk->y; pb.ldy = blk->ldy; pb.ids = blk->ids;
      pb.train_loss = blk->train_loss; pb.test_loss = blk->test_loss;
      pb.y_test = blk->y; pb.ldy_test = blk->ldy; pb.n_test = blk->max_test;
      pb.chunks = blk->chunks; pb.n_chunks = blk->n_chunks;
    }
    // a single rank's whole call (or block of calls): the evaluations behind the launch, where the plan's
    // snapshot memory holds them (else, as ever, inside it)
    if (deferred && p->eval_deferred && eval_total == n && !p->split_adam && !xr &&
        deferred_eval_reserve(p->ug, (int)count_logging_points(n) * (blk ? blk->n_chunks : 1), &p->deferred)) {
      pb.deferred = p->deferred.mem;
      ++p->n_deferred;
      BSIG_TRY(persist_run(persist_shape(p), p->ug, pb, n, st));
      return deferred_eval_run(persist_shape(p), p->ug, pb, n, st);
    }
    if (deferred) ++p->n_in_launch;
    return persist_run(persist_shape(p), p->ug, pb, n, st);
  }
  PersistMdnnBuffers pb;
  static_cast<PersistCommon&>(pb) = c;
  pb.x = b.x_train; pb.ldx = b.ldx_train;
  pb.x_kind = b.x_kind; pb.x_s = b.x_s; pb.x_a = b.x_a;
  pb.w1_off = p->L.w_off[0]; pb.b1_off = p->L.b_off[0];
  pb.w2_off = p->L.w_off[1]; pb.b2_off = p->L.b_off[1];
  pb.wh_off = p->L.head_w_off; pb.bh_off = p->L.head_b_off;
  pb.x_test = b.x_test; pb.ldx_test = b.ldx_test;
  pb.x_test_fac = b.x_test_factors; pb.ldx_test_fac = b.ldx_test_factors;
  return persist_mdnn_run(persist_mdnn_shape(p), p->mg, pb, n, st);
}

static Inputs<float> train_inputs(const bsig_fit_plan* p, const PlanMem& m) {
  const bsig_fit_buffers& b = p->buf;
  Inputs<float> in;
  in.dyn = b.state + ST_STEP; in.dyn_stride = p->batch;
  in.rff_coeff = b.rff_coeff; in.ld_coeff = b.ld_coeff; in.rff_offset = b.rff_offset;
  if (p->hoist) {
    in.x = m.feats; in.ldx = p->cfg.rff_feats; in.is_feat = true;
    if (p->feat_unique) in.rows = b.ids_table;   // feature cache: one row per training row
  }
  else { in.x = b.x_train; in.ldx = b.ldx_train; in.rows = b.ids_table; }
  return in;
}

static Inputs<float> eval_inputs(const bsig_fit_plan* p, const PlanMem& m) {
  const bsig_fit_buffers& b = p->buf;
  Inputs<float> in;
  in.rff_coeff = b.rff_coeff; in.ld_coeff = b.ld_coeff; in.rff_offset = b.rff_offset;
  if (p->hoist) {
    in.x = m.feats; in.ldx = p->cfg.rff_feats; in.is_feat = true;
    // the held-out rows are the same at every evaluation: projected once
    in.dyn = b.state + ST_EVAL; in.dyn_stride = 0;
    in.dyn_base = p->feat_unique ? b.n_train : p->n_updates * p->batch;
  } else {
    in.x = b.x_test; in.ldx = b.ldx_test;
  }
  return in;
}

// forward + NLL + finish (advances the step) [+ backward]
static int enqueue_grad(bsig_fit_plan* p, hipStream_t st, bool fuse_adam) {
  if (p->buf.x_kind != BSIG_X_ROWS) { set_error("per-phase update on factor rows"); return BSIG_EUNSUPPORTED; }
  PlanMem m; plan_mem(p, &m);
  const bsig_fit_buffers& b = p->buf;
  const Inputs<float> in = train_inputs(p, m);
  HeadDyn hd;
  hd.y_dyn = b.state + ST_STEP; hd.y_dyn_stride = p->batch;
  hd.hook.state = b.state; hd.hook.kind = 1;
  hd.hook.lr = p->cfg.lr; hd.hook.beta1 = p->cfg.beta1; hd.hook.beta2 = p->cfg.beta2;
  AdamFuse fuse{b.exp_avg, b.exp_avg_sq, st_adam(b.state), p->cfg.beta1, p->cfg.beta2, p->cfg.adam_eps};
  const uint64_t* rng = st_rng(b.state);
  int n_sig = 0;
  BSIG_TRY(forward_pass(&p->cfg, p->L, b.params, in, p->cfg.rff_scale, p->batch, m.tr, m.tr.o, m.tr.ld_o, st,
                        &n_sig));
  hd.n_sig_ready = n_sig;
  // a fused Adam step whose weight gradient runs as the whole-width kernel + reduce: the head bias
  // gradients stay partial column sums (no colsum kernel); gemm_run refuses them on any other path
  HeadBiasPartials bp;
  const bool partial_bias = fuse_adam && p->L.n_layers == 0 && in.rows != nullptr &&
      gemm_wide_gradient_applies(p->L.nh, p->L.feat_dim, p->batch, m.tr.ld_o, in.ldx, m.tr.d_o, in.x, true);
  BSIG_TRY(head_nll(&p->cfg, p->L, m.tr, b.y_train, b.ldy_train, b.ids_table, p->batch,
                    p->norm_batch, nullptr, 0, 0, rng, b.train_loss, b.state + ST_STEP, true,
                    b.grads + p->L.head_b_off, b.state + ST_FLAGS, &hd, st,
                    partial_bias ? &bp : nullptr));
  return backward_pass(&p->cfg, p->L, b.params, in, -1, p->batch, m.tr, b.grads,
                       fuse_adam ? &fuse : nullptr, st, partial_bias ? &bp : nullptr);
}

static int enqueue_apply(bsig_fit_plan* p, hipStream_t st) {
  const bsig_fit_buffers& b = p->buf;
  return adam_launch(b.params, b.grads, b.exp_avg, b.exp_avg_sq, p->L.total, p->cfg.lr,
                     p->cfg.beta1, p->cfg.beta2, p->cfg.adam_eps, 1, st_adam(b.state), st);
}

static int enqueue_eval(bsig_fit_plan* p, hipStream_t st) {
  PlanMem m; plan_mem(p, &m);
  const bsig_fit_buffers& b = p->buf;
  HeadDyn hd;
  hd.hook.state = b.state; hd.hook.kind = 2;
  if (b.n_test <= 0) {   // nothing held out: still consume an evaluation slot
    hipLaunchKernelGGL(iota_mod_kernel, dim3(1), dim3(64), 0, st, b.state + ST_EVAL + 0, 0, 1);
    BSIG_CHECK_LAUNCH("eval_noop");
    return BSIG_OK;
  }
  const Inputs<float> in = eval_inputs(p, m);
  int n_sig = 0;
  BSIG_TRY(forward_pass(&p->cfg, p->L, b.params, in, p->cfg.rff_scale, b.n_test, m.te, m.te.o, m.te.ld_o, st,
                        &n_sig));
  hd.n_sig_ready = n_sig;
  return head_nll(&p->cfg, p->L, m.te, b.y_test, b.ldy_test, nullptr, b.n_test, b.n_test,
                  nullptr, 0, 0, st_rng(b.state),
                  b.test_loss, b.state + ST_EVAL, false, nullptr, b.state + ST_FLAGS, &hd,
                  st);
}

// RFF projection of every minibatch row of this call (and of the held-out rows,
// once per evaluation) in two large GEMMs.
static int enqueue_hoisted_rff(bsig_fit_plan* p, hipStream_t st) {
  PlanMem m; plan_mem(p, &m);
  const bsig_fit_buffers& b = p->buf;
  Inputs<float> in;
  in.x = b.x_train; in.ldx = b.ldx_train;
  in.rff_coeff = b.rff_coeff; in.ld_coeff = b.ld_coeff; in.rff_offset = b.rff_offset;
  // feature cache: each distinct training row once (it is visited ~n_updates*batch/n_train
  // times); when that does not fit the plan's buffer, every gathered minibatch row
  const int64_t train_rows = p->feat_unique ? b.n_train : p->n_updates * p->batch;
  if (!p->feat_unique) in.rows = b.ids_table;
  // the held-out rows lie right behind the training rows (the usual binding: one staged block of
  // the chunk): ONE projection over all of them -- a 1000-pair chunk is 16 x 32 tiles of 64 x 64 =
  // 512 workgroups, two per CU, where 800 + 200 rows were 416 + 128 in two launches
  if (p->feat_unique && b.n_test > 0 && b.ldx_test == b.ldx_train &&
      b.x_test == b.x_train + (size_t)b.n_train * b.ldx_train)
    return rff_project(&p->cfg, in, p->cfg.rff_scale, train_rows + b.n_test, m.feats, m.big_ws, p->big_gemm_ws_bytes, p->matmul, st);
  BSIG_TRY(rff_project(&p->cfg, in, p->cfg.rff_scale, train_rows, m.feats, m.big_ws, p->big_gemm_ws_bytes, p->matmul, st));
  if (b.n_test > 0) {
    in.x = b.x_test; in.ldx = b.ldx_test; in.rows = nullptr;
    BSIG_TRY(rff_project(&p->cfg, in, p->cfg.rff_scale, b.n_test, m.feats + (size_t)train_rows * p->cfg.rff_feats,
                         m.big_ws, p->big_gemm_ws_bytes, p->matmul, st));
  }
  return BSIG_OK;
}

static void drop_graphs(bsig_fit_plan* p) {
  hipGraphExec_t* gs[5] = {&p->g_step, &p->g_grad, &p->g_apply, &p->g_eval, &p->g_dp};
  for (auto g : gs)
    if (*g) { (void)hipGraphExecDestroy(*g); *g = nullptr; }
  p->g_dp_state = 0; p->g_dp_comm = nullptr;
  p->graphs_ready = false;
}

template <typename F>
static int capture(bsig_fit_plan* p, hipGraphExec_t* out, F&& body) {
  hipGraph_t graph = nullptr;
  BSIG_HIP(hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeRelaxed));
  const int rc = body(p->cap_stream);
  const hipError_t e = hipStreamEndCapture(p->cap_stream, &graph);
  if (rc != BSIG_OK) { if (graph) (void)hipGraphDestroy(graph); return rc; }
  if (e != hipSuccess) { set_error("hipStreamEndCapture: %s", hipGetErrorString(e)); return BSIG_ELAUNCH; }
  const hipError_t e2 = hipGraphInstantiate(out, graph, nullptr, nullptr, 0);
  (void)hipGraphDestroy(graph);
  if (e2 != hipSuccess) { set_error("hipGraphInstantiate: %s", hipGetErrorString(e2)); return BSIG_ELAUNCH; }
  return BSIG_OK;
}

static int ensure_graphs(bsig_fit_plan* p) {
  PlanMem fm; plan_mem(p, &fm);
  // the graphs carry the feature block's address as a kernel argument: a block handed over in
  // place (bsig_fit_set_features) or taken back (bsig_fit_begin) invalidates them
  if (p->graphs_ready && p->graph_feats != fm.feats) drop_graphs(p);
  if (!p->use_graph || p->graphs_ready) return BSIG_OK;
  p->graph_feats = fm.feats;
  if (p->split_adam) {
    if (!engine(p)) {
      BSIG_TRY(capture(p, &p->g_grad, [&](hipStream_t s) { return enqueue_grad(p, s, false); }));
      BSIG_TRY(capture(p, &p->g_apply, [&](hipStream_t s) { return enqueue_apply(p, s); }));
    }
  } else if (engine(p)) {
    // updates are single launches of a persistent kernel: no update graph
  } else {
    BSIG_TRY(capture(p, &p->g_step, [&](hipStream_t s) { return enqueue_grad(p, s, true); }));
  }
  // (a binding without held-out summary rows evaluates from factor rows inside its launches:
  // bsig_fit_evaluates_from_factors -- there is nothing an evaluation graph could read)
  if (p->buf.n_test < 1 || p->buf.x_test)
    BSIG_TRY(capture(p, &p->g_eval, [&](hipStream_t s) { return enqueue_eval(p, s); }));
  p->graphs_ready = true;
  return BSIG_OK;
}

}  // namespace bsig

extern "C" int64_t bsig_mdn_param_count(const bsig_mdn_cfg* cfg) {
  Layout L;
  if (make_layout(cfg, &L) != BSIG_OK) return -1;
  return L.total;
}

extern "C" int bsig_mdn_param_offsets(const bsig_mdn_cfg* cfg, int64_t* offsets, int n_offsets) {
  Layout L;
  BSIG_TRY(make_layout(cfg, &L));
  const int need = 2 * (L.n_layers + 4);
  BSIG_REQUIRE(offsets && n_offsets >= need, "param_offsets: need %d slots", need);
  int q = 0;
  for (int l = 0; l < L.n_layers; ++l) { offsets[q++] = L.w_off[l]; offsets[q++] = L.b_off[l]; }
  const int64_t D = cfg->head.out_dim, K = cfg->head.n_comp, F = L.feat_dim;
  const int64_t row0[4] = {0, K, K + D * K, K + 2 * D * K};
  for (int hsel = 0; hsel < 4; ++hsel) {
    offsets[q++] = L.head_w_off + row0[hsel] * F;
    offsets[q++] = L.head_b_off + row0[hsel];
  }
  return BSIG_OK;
}

extern "C" size_t bsig_mdn_workspace_bytes(const bsig_mdn_cfg* cfg, int64_t max_batch) {
  Layout L;
  if (make_layout(cfg, &L) != BSIG_OK) return 0;
  Scratch<float> s;
  carve(cfg, L, std::max<int64_t>(max_batch, 1), nullptr, &s);
  return s.total_bytes;
}

extern "C" int bsig_mdn_head_forward(const bsig_mdn_cfg* cfg, const float* params,
                                     const float* rff_coeff, int64_t ld_coeff,
                                     const float* rff_offset, const float* x, int64_t ldx,
                                     const int32_t* x_rows, int64_t batch, float* head_out,
                                     int64_t ld_head, void* workspace, size_t workspace_bytes,
                                     bsig_stream_t stream) {
  Layout L;
  BSIG_TRY(make_layout(cfg, &L));
  BSIG_REQUIRE(params && x && head_out && batch >= 1, "head_forward: bad args");
  BSIG_REQUIRE(ldx >= cfg->input_dim && ld_head >= L.nh, "head_forward: leading dims too small");
  Scratch<float> s;
  carve(cfg, L, batch, nullptr, &s);
  BSIG_REQUIRE(workspace && workspace_bytes >= s.total_bytes,
               "head_forward: workspace %zu < %zu", workspace_bytes, s.total_bytes);
  carve(cfg, L, batch, workspace, &s);
  s.tickets = nullptr;   // (nobody zeroes a caller's workspace: the head product reduces in its own kernel)
  Inputs<float> in;
  in.x = x; in.ldx = ldx; in.rows = x_rows;
  in.rff_coeff = rff_coeff; in.ld_coeff = ld_coeff; in.rff_offset = rff_offset;
  return forward_pass(cfg, L, params, in, cfg->rff_scale, batch, s, head_out, ld_head, as_stream(stream));
}

extern "C" int bsig_mdn_loss_grad(const bsig_mdn_cfg* cfg, const float* params,
                                  const float* rff_coeff, int64_t ld_coeff,
                                  const float* rff_offset, const float* x, int64_t ldx,
                                  const float* y, int64_t ldy, const int32_t* rows,
                                  int64_t batch, int64_t norm_batch, const float* noise,
                                  uint64_t seed, uint64_t stream_id, float* grads, float* loss,
                                  int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                                  bsig_stream_t stream) {
  Layout L;
  BSIG_TRY(make_layout(cfg, &L));
  BSIG_REQUIRE(params && x && y && grads && batch >= 1 && norm_batch >= 1,
               "loss_grad: bad args");
  BSIG_REQUIRE(ldx >= cfg->input_dim && ldy >= cfg->head.out_dim, "loss_grad: leading dims");
  Scratch<float> s;
  carve(cfg, L, batch, nullptr, &s);
  BSIG_REQUIRE(workspace && workspace_bytes >= s.total_bytes, "loss_grad: workspace %zu < %zu",
               workspace_bytes, s.total_bytes);
  carve(cfg, L, batch, workspace, &s);
  s.tickets = nullptr;   // (nobody zeroes a caller's workspace: the head product reduces in its own kernel)
  hipStream_t st = as_stream(stream);
  Inputs<float> in;
  in.x = x; in.ldx = ldx; in.rows = rows;
  in.rff_coeff = rff_coeff; in.ld_coeff = ld_coeff; in.rff_offset = rff_offset;
  int n_sig = 0;
  BSIG_TRY(forward_pass(cfg, L, params, in, cfg->rff_scale, batch, s, s.o, s.ld_o, st, &n_sig));
  HeadDyn hd;
  hd.n_sig_ready = n_sig;
  BSIG_TRY(head_nll(cfg, L, s, y, ldy, rows, batch, norm_batch, noise, seed, stream_id, nullptr,
                    loss, nullptr, true, grads + L.head_b_off, nonfinite, &hd, st));
  return backward_pass(cfg, L, const_cast<float*>(params), in, 0, batch, s, grads, nullptr, st);
}

extern "C" int bsig_fit_create(const bsig_mdn_cfg* cfg, int64_t batch, int64_t max_test_rows,
                               int64_t n_updates, bsig_fit_plan** plan) {
  return bsig_fit_create_sized(cfg, batch, 0, max_test_rows, n_updates, plan);
}

extern "C" int bsig_fit_create_sized(const bsig_mdn_cfg* cfg, int64_t batch,
                                     int64_t max_train_rows, int64_t max_test_rows,
                                     int64_t n_updates, bsig_fit_plan** plan) {
  return bsig_fit_create_ex(cfg, batch, max_train_rows, max_test_rows, n_updates, 0, plan);
}

extern "C" int bsig_fit_create_ex(const bsig_mdn_cfg* cfg, int64_t batch,
                                  int64_t max_train_rows, int64_t max_test_rows,
                                  int64_t n_updates, int plan_flags, bsig_fit_plan** plan) {
  BSIG_REQUIRE(cfg && plan && batch >= 1 && max_train_rows >= 0 && max_test_rows >= 0 &&
               n_updates >= 0, "fit_create: bad args");
  bsig_fit_plan* p = new (std::nothrow) bsig_fit_plan();
  BSIG_REQUIRE(p, "fit_create: out of memory");
  std::memset(p, 0, sizeof(*p));
  p->cfg = *cfg;
  const int rc = make_layout(cfg, &p->L);
  if (rc != BSIG_OK) { delete p; return rc; }
  p->batch = batch; p->max_test = max_test_rows; p->norm_batch = batch;
  p->n_updates = n_updates; p->n_evals = count_logging_points(n_updates);
  p->matmul = (plan_flags & BSIG_PLAN_SPLIT_BF16) ? BSIG_MATMUL_SPLIT_BF16 : BSIG_MATMUL_FP32;
  Scratch<float> s;
  carve(cfg, p->L, batch, nullptr, &s); p->train_ws_bytes = s.total_bytes;
  carve(cfg, p->L, std::max<int64_t>(max_test_rows, 1), nullptr, &s);
  p->test_ws_bytes = s.total_bytes;
  // MDRFF feature block: one row per gathered minibatch row, or -- when the caller bounds the
  // training rows and they are fewer -- one per distinct training row (feature cache)
  p->max_train = max_train_rows;
  // the plan's switches (diagnostics, A/B runs), read here once
  const auto set = [](const char* name) { const char* e = getenv(name); return e && e[0] == '1'; };
  p->feat_cache = !set("BSIG_NO_FEAT_CACHE");   // (set: every gathered row projected)
  if (!p->feat_cache) max_train_rows = 0;
  p->feat_rows = (max_train_rows > 0 ? std::min(n_updates * batch, max_train_rows)
                                     : n_updates * batch) + max_test_rows;
  const size_t feats = (size_t)p->feat_rows * (size_t)std::max(cfg->rff_feats, 0) * sizeof(float);
  p->hoist = cfg->rff_feats > 0 && n_updates > 0 && feats <= ((size_t)4 << 30) && !set("BSIG_NO_RFF_HOIST");
  // the persistent update engine: resolved once, here (a streamed first layer: completed at bind)
  if (!((plan_flags & BSIG_PLAN_NO_PERSISTENT) || set("BSIG_NO_PERSISTENT"))) {
    if (p->hoist && p->L.n_layers == 0 && cfg->head.full_cov == 0)
      persist_resolve(persist_shape(p), &p->ug, &p->eng);
    else if (cfg->rff_feats == 0 && p->L.n_layers == 2 && n_updates > 0)
      persist_mdnn_resolve(persist_mdnn_shape(p), &p->mg, &p->eng);
  }
  if (set("BSIG_NO_INKERNEL_EVAL")) p->eng.eval_single = p->eng.eval_dp = false;
  p->eng.block_launch = block_launch_resolved(p->eng.kind, p->eng.eval_single, set("BSIG_FIT_CHUNK_PER_LAUNCH"));
  p->eng.workspace_bytes = round_up<size_t>(p->eng.workspace_bytes, 256);
  p->eval_deferred = p->eng.kind == 1 && p->eng.eval_single && !set("BSIG_EVAL_IN_LAUNCH");
  if (p->hoist) {
    p->feats_bytes = round_up<size_t>(feats, 256);
    const int64_t mf = cfg->rff_cos_only ? cfg->rff_feats : cfg->rff_feats / 2;
    p->big_gemm_ws_bytes = round_up<size_t>(
        std::max(bsig_gemm_workspace_bytes(p->feat_rows - max_test_rows, mf, cfg->input_dim),
                 bsig_gemm_workspace_bytes(std::max<int64_t>(max_test_rows, 1), mf,
                                           cfg->input_dim)) + 256, 256);
  }
  *plan = p;
  return BSIG_OK;
}

extern "C" void bsig_fit_destroy(bsig_fit_plan* p) {
  if (!p) return;
  drop_graphs(p);
  if (p->cap_stream) (void)hipStreamDestroy(p->cap_stream);
  deferred_eval_free(&p->deferred);
  delete p;
}

extern "C" size_t bsig_fit_workspace_bytes(const bsig_fit_plan* p) {
  return p ? plan_ws_bytes(p) : 0;
}

extern "C" int bsig_fit_bind(bsig_fit_plan* p, const bsig_fit_buffers* b, int flags) {
  BSIG_REQUIRE(p && b, "fit_bind: null");
  BSIG_REQUIRE(b->params && b->grads && b->exp_avg && b->exp_avg_sq && b->state &&
               b->workspace && b->x_train && b->y_train && b->ids_table && b->train_loss &&
               b->test_loss, "fit_bind: null buffer");
  BSIG_REQUIRE(b->workspace_bytes >= plan_ws_bytes(p), "fit_bind: workspace %zu < %zu",
               b->workspace_bytes, plan_ws_bytes(p));
  BSIG_REQUIRE(!(p->max_train > 0 && b->n_train > p->max_train),
               "fit_bind: %lld training rows exceed the %lld the plan was sized for",
               (long long)b->n_train, (long long)p->max_train);
  BSIG_REQUIRE(b->n_train >= 1 && b->n_test >= 0 && b->n_test <= std::max<int64_t>(p->max_test, 0),
               "fit_bind: n_train=%lld n_test=%lld (max %lld)", (long long)b->n_train,
               (long long)b->n_test, (long long)p->max_test);
  const bool fac = b->x_kind == BSIG_X_CROSSCORR_FACTORS;
  BSIG_REQUIRE(b->x_kind == BSIG_X_ROWS || fac, "fit_bind: unknown x_kind %d", b->x_kind);
  const bool graph = (flags & BSIG_FIT_GRAPH) != 0, split = (flags & BSIG_FIT_SPLIT_ADAM) != 0;
  // a streamed first layer exists for factor rows only: summary rows of that width go through
  // the per-phase kernels
  const bool eng_off = p->eng.streams && !(fac && bsig_fit_accepts_factor_rows(p, b->x_s, b->x_a));
  if (eng_off != p->eng_off) { drop_graphs(p); p->eng_off = eng_off; p->bound = false; }
  // ... and the launch of the streamed tile workgroups takes these factor dimensions
  const MdnnGeom& g = p->mg;
  if (engine(p) == 2 && p->eng.streams && !(g.s_S == b->x_s && g.s_A == b->x_a && g.s_dp == (split ? 1 : 0)))
    BSIG_TRY(persist_mdnn_resolve_stream(&p->mg, p->cfg.input_dim, p->cfg.head.full_cov != 0, b->x_s, b->x_a, split));
  if (fac) {
    BSIG_REQUIRE(b->x_s >= 1 && b->x_a >= 1 && (int64_t)b->x_s * b->x_a + 2 == p->cfg.input_dim,
                 "fit_bind: factor rows S=%d A=%d do not give the %d inputs of the first layer",
                 b->x_s, b->x_a, p->cfg.input_dim);
    BSIG_REQUIRE(b->ldx_train >= b->x_s + b->x_a + 3, "fit_bind: factor rows need a pitch >= S + A + 3");
    // (no held-out summary rows at all where the launch evaluates from the held-out FACTOR rows)
    const bool eval_fac = b->x_test_factors && bsig_fit_evaluates_from_factors(p, b->x_s, b->x_a, flags);
    BSIG_REQUIRE(b->n_test == 0 || (eval_fac && !b->x_test) || b->ldx_test >= p->cfg.input_dim,
                 "fit_bind: the held-out rows are summary rows (ldx_test >= input_dim)");
    if (!bsig_fit_accepts_factor_rows(p, b->x_s, b->x_a)) {
      set_error("fit_bind: this plan runs kernels that read materialised summary rows "
                "(bsig_fit_accepts_factors); expand the factors (bsig_crosscorr_expand)");
      return BSIG_EUNSUPPORTED;
    }
  }
  BSIG_REQUIRE((fac || b->ldx_train >= p->cfg.input_dim) && b->ldy_train >= p->cfg.head.out_dim,
               "fit_bind: leading dims too small");
  BSIG_REQUIRE(!(b->n_test > 0 && !b->y_test), "fit_bind: null test buffers");
  BSIG_REQUIRE(!(b->n_test > 0 && !b->x_test &&
                 !(fac && b->x_test_factors && bsig_fit_evaluates_from_factors(p, b->x_s, b->x_a, flags))),
               "fit_bind: null test buffers");
  const bool same = p->bound && std::memcmp(&p->buf, b, sizeof(*b)) == 0 &&
                    p->use_graph == graph && p->split_adam == split;
  if (!same) {
    drop_graphs(p);
    p->buf = *b;
    p->feat_unique = feat_cache_applies(p, b->n_train);
    if (p->hoist && !p->feat_unique && p->feat_rows - p->max_test < p->n_updates * p->batch) {
      p->bound = false;
      set_error("fit_bind: %lld training rows exceed the %lld the plan was sized for",
                (long long)b->n_train, (long long)p->max_train);
      return BSIG_EINVAL;
    }
    p->bound = true;
    p->use_graph = graph;
    p->split_adam = split;
  }
  if (p->use_graph && !p->cap_stream)
    BSIG_HIP(hipStreamCreateWithFlags(&p->cap_stream, hipStreamNonBlocking));
  return BSIG_OK;
}

// Does a captured graph of this plan read the MDRFF feature block?  (Then the block must stay
// at the workspace address the graphs were captured with: a caller's block is copied there.)
static bool graphs_read_feats(const bsig_fit_plan* p) {
  if (!p->use_graph) return false;       // direct launches take the pointer of the call
  if (engine(p) != 1) return true;       // update and evaluation graphs
  if (p->buf.n_test < 1) return false;
  return !evals_in_launch(p, p->split_adam, false);
}

extern "C" int bsig_fit_set_features(bsig_fit_plan* p, const float* feats, int64_t ld_feats,
                                     int64_t rows, bsig_stream_t stream) {
  BSIG_REQUIRE(p && p->bound && feats, "fit_set_features: plan not bound / null");
  BSIG_REQUIRE(p->hoist && p->feat_unique, "fit_set_features: the plan keeps no per-row feature cache");
  BSIG_REQUIRE(rows == p->buf.n_train + p->buf.n_test && ld_feats >= p->cfg.rff_feats,
               "fit_set_features: need the %lld training + %lld held-out rows",
               (long long)p->buf.n_train, (long long)p->buf.n_test);
  p->ext_feats = nullptr;
  if (ld_feats == p->cfg.rff_feats && aligned(feats, 16) && !graphs_read_feats(p)) {
    // a dense block of feature rows: the kernels read it in place (the caller keeps it alive
    // until the call's work has been enqueued and run)
    p->ext_feats = feats;
  } else {
    PlanMem m; plan_mem(p, &m);
    const size_t w = (size_t)p->cfg.rff_feats * sizeof(float);
    BSIG_HIP(hipMemcpy2DAsync(m.feats, w, feats, (size_t)ld_feats * sizeof(float), w, (size_t)rows,
                              hipMemcpyDeviceToDevice, as_stream(stream)));
  }
  p->feats_preloaded = true;
  return BSIG_OK;
}

// project: fill the MDRFF feature cache unless the caller handed the rows' features over (a block of
// chunks reads the caller's feature rows of the whole block: nothing to project)
static int fit_begin(bsig_fit_plan* p, uint64_t seed, int64_t norm_batch, bsig_stream_t stream, bool project) {
  BSIG_REQUIRE(p && p->bound, "fit_begin: plan not bound");
  BSIG_REQUIRE(norm_batch >= 1, "fit_begin: norm_batch must be >= 1");
  if (norm_batch != p->norm_batch) { drop_graphs(p); p->norm_batch = norm_batch; }
  hipStream_t st = as_stream(stream);
  p->adam_pending = false;
  p->resident_ran = false;
  p->dp_evals_done = 0;
  BeginZero bz{};
  int nz = 0;
  int64_t total4 = 0;
  auto add_zero = [&](void* ptr, size_t bytes) {
    bz.ptr[nz] = reinterpret_cast<float4*>(ptr);
    bz.n4[nz] = (int64_t)(bytes / 16);
    total4 += bz.n4[nz];
    ++nz;
  };
  if (engine(p)) {
    PlanMem m; plan_mem(p, &m);
    ZeroRegion zr[2];
    if (engine(p) == 1) BSIG_TRY(persist_reset_regions(p->ug, m.persist_ws, p->eng.workspace_bytes, zr));
    else BSIG_TRY(persist_mdnn_reset_regions(p->mg, m.persist_ws, p->eng.workspace_bytes, zr));
    BSIG_REQUIRE(aligned(zr[0].ptr, 16) && aligned(zr[1].ptr, 16) && zr[0].bytes % 16 == 0 &&
                 zr[1].bytes % 16 == 0, "fit_begin: persistent workspace regions must be 16-byte multiples");
    add_zero(zr[0].ptr, zr[0].bytes);
    add_zero(zr[1].ptr, zr[1].bytes);
  }
  // fresh optimizer state for every run_training call (mdnn.py:203); a single-rank plan in a
  // persistent kernel starts the moments at zero in its registers instead
  if (!(engine(p) && !p->split_adam)) {
    BSIG_REQUIRE(aligned(p->buf.exp_avg, 16) && aligned(p->buf.exp_avg_sq, 16),
                 "fit_begin: the Adam moment buffers must be 16-byte aligned");
    add_zero(p->buf.exp_avg, (size_t)p->L.total * sizeof(float));
    add_zero(p->buf.exp_avg_sq, (size_t)p->L.total * sizeof(float));
  }
  // the combine tickets of the whole-width head products (left zeroed by every launch that uses
  // them; zeroed here once more per call -- where the kernel's four regions have room)
  if (tickets_zeroed(p)) {
    BSIG_REQUIRE(nz == begin_regions(p), "fit_begin: region count out of step with begin_regions()");
    PlanMem tm; plan_mem(p, &tm);
    add_zero(tm.tr.tickets, kWideTickets * sizeof(int32_t));
    add_zero(tm.te.tickets, kWideTickets * sizeof(int32_t));
  }
  const int blocks = (int)std::min<int64_t>(std::max<int64_t>(ceil_div<int64_t>(total4, 256 * 4), 1), 1024);
  hipLaunchKernelGGL(fit_begin_kernel, dim3(blocks), dim3(256), 0, st, p->buf.state, seed, bz);
  BSIG_CHECK_LAUNCH("fit_begin");
  if (p->hoist && project) {
    if (p->feats_preloaded) p->feats_preloaded = false;   // handed over for this call
    else { p->ext_feats = nullptr; BSIG_TRY(enqueue_hoisted_rff(p, st)); }
  }
  return ensure_graphs(p);
}

extern "C" int bsig_fit_begin(bsig_fit_plan* p, uint64_t seed, int64_t norm_batch,
                              bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit_begin");
  return fit_begin(p, seed, norm_batch, stream, true);
}

// data-parallel plans covered by a persistent kernel: the held-out evaluations run inside
// the per-update launches too (the one after the last update in the launch that takes its
// pending Adam step; a rank of a streamed first layer or of wide heads evaluates between its launches)
static int dp_eval_total(const bsig_fit_plan* p) {
  return engine(p) && p->split_adam && p->buf.n_test >= 1 && evals_in_launch(p, true, false) ? (int)p->n_updates : 0;
}

extern "C" int bsig_fit_grad(bsig_fit_plan* p, bsig_stream_t stream) {
  BSIG_REQUIRE(p && p->bound && p->split_adam, "fit_grad: plan not bound with SPLIT_ADAM");
  if (engine(p)) return enqueue_persistent(p, 1, as_stream(stream), dp_eval_total(p));
  if (p->use_graph) { BSIG_TRY(ensure_graphs(p)); BSIG_HIP(hipGraphLaunch(p->g_grad, as_stream(stream))); return BSIG_OK; }
  return enqueue_grad(p, as_stream(stream), false);
}

extern "C" int bsig_fit_apply(bsig_fit_plan* p, bsig_stream_t stream) {
  BSIG_REQUIRE(p && p->bound && p->split_adam, "fit_apply: plan not bound with SPLIT_ADAM");
  // persistent kernel: the step is taken by the next bsig_fit_grad launch while it
  // loads its tiles (bsig_fit_eval / bsig_fit_flush take it at once)
  if (engine(p) && !p->eng.streams) { p->adam_pending = true; return BSIG_OK; }
  // (a streamed first layer: the flat Adam kernel, with the step sizes the launch left in the state block)
  if (engine(p)) return enqueue_apply(p, as_stream(stream));
  if (p->use_graph) { BSIG_TRY(ensure_graphs(p)); BSIG_HIP(hipGraphLaunch(p->g_apply, as_stream(stream))); return BSIG_OK; }
  return enqueue_apply(p, as_stream(stream));
}

extern "C" int bsig_fit_takes_features(const bsig_fit_plan* p, int64_t n_train) {
  // a hoisted MDRFF plan keeps one feature row per training row when the call visits its rows
  // more than once: bsig_fit_set_features then replaces the projection and nothing reads
  // x_train / x_test afterwards (feat_unique in bsig_fit_bind)
  return p && n_train >= 1 && feat_cache_applies(p, n_train) ? 1 : 0;
}

extern "C" int bsig_fit_accepts_factors(const bsig_fit_plan* p) {
  // every update runs in the persistent kernel of the two-layer MDNN, whose first-layer tile
  // workgroups form the products; the evaluations read materialised held-out rows
  // (a plan with a streamed first layer: only through bsig_fit_accepts_factor_rows, which sees S and A)
  return p && p->eng.kind == 2 && !p->eng.streams ? 1 : 0;
}

extern "C" int bsig_fit_accepts_factor_rows(const bsig_fit_plan* p, int s_dim, int a_dim) {
  // ... for these factor dimensions: a plan whose first layer is STREAMED (it does not fit the
  // chip: cfg/anymal.yaml, cfg/shadow_hand_more.yaml) covers A % 4 == 0 and factor rows of two
  // minibatches in a workgroup's LDS
  return p && p->eng.kind == 2 && persist_mdnn_factors_fit(p->mg, p->cfg.input_dim, s_dim, a_dim) ? 1 : 0;
}

// Would a call bound with these factor rows and bind flags evaluate its held-out pairs from their
// FACTOR rows inside the launch (a streamed first layer, single rank)?  Then nothing reads
// materialised held-out summary rows and the caller need not build them (bsig_fit_buffers.x_test
// may be null).
extern "C" int bsig_fit_evaluates_from_factors(const bsig_fit_plan* p, int s_dim, int a_dim, int bind_flags) {
  // (a data-parallel rank evaluates between its launches)
  return p && p->eng.streams && bsig_fit_accepts_factor_rows(p, s_dim, a_dim) &&
                 evals_in_launch(p, (bind_flags & BSIG_FIT_SPLIT_ADAM) != 0, true) ? 1 : 0;
}

extern "C" int bsig_fit_is_persistent(const bsig_fit_plan* p) {
  return p ? engine(p) : 0;
}

extern "C" int bsig_fit_flush(bsig_fit_plan* p, bsig_stream_t stream) {
  BSIG_REQUIRE(p && p->bound, "fit_flush: plan not bound");
  if (engine(p) && p->split_adam && p->adam_pending)
    return enqueue_persistent(p, 0, as_stream(stream));
  return BSIG_OK;
}

extern "C" int bsig_fit_eval(bsig_fit_plan* p, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit_eval");
  BSIG_REQUIRE(p && p->bound, "fit_eval: plan not bound");
  if (const int total = dp_eval_total(p)) {
    // evaluations inside the launches: all but the last are already under way
    if (++p->dp_evals_done < count_logging_points(total)) return BSIG_OK;
    return enqueue_persistent(p, 0, as_stream(stream), total);
  }
  BSIG_REQUIRE(p->buf.n_test < 1 || p->buf.x_test,
               "fit_eval: this binding has no held-out summary rows (its evaluations run inside bsig_fit_run)");
  BSIG_TRY(bsig_fit_flush(p, stream));
  if (p->use_graph) { BSIG_TRY(ensure_graphs(p)); BSIG_HIP(hipGraphLaunch(p->g_eval, as_stream(stream))); return BSIG_OK; }
  return enqueue_eval(p, as_stream(stream));
}

// n consecutive updates, no evaluation: one launch of the persistent kernel when
// the plan is covered by it, else n replays of the update graph
static int enqueue_updates(bsig_fit_plan* p, int64_t n, hipStream_t st) {
  if (n <= 0) return BSIG_OK;
  if (engine(p) && !p->split_adam) return enqueue_persistent(p, (int)n, st);
  if (engine(p)) {   // data-parallel plan driven without an exchange (one rank)
    for (int64_t it = 0; it < n; ++it) {
      BSIG_TRY(enqueue_persistent(p, 1, st, dp_eval_total(p)));
      if (p->eng.streams) BSIG_TRY(enqueue_apply(p, st));
      else p->adam_pending = true;
    }
    return BSIG_OK;
  }
  for (int64_t it = 0; it < n; ++it) {
    if (p->use_graph) {
      if (p->split_adam) {
        BSIG_HIP(hipGraphLaunch(p->g_grad, st));
        BSIG_HIP(hipGraphLaunch(p->g_apply, st));
      } else {
        BSIG_HIP(hipGraphLaunch(p->g_step, st));
      }
    } else {
      BSIG_TRY(enqueue_grad(p, st, !p->split_adam));
      if (p->split_adam) BSIG_TRY(enqueue_apply(p, st));
    }
  }
  return BSIG_OK;
}

extern "C" int bsig_fit_updates(bsig_fit_plan* p, int64_t n_updates, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit_updates");
  BSIG_REQUIRE(p && p->bound, "fit_updates: plan not bound");
  BSIG_REQUIRE(n_updates >= 0 && n_updates <= p->n_updates,
               "fit_updates: n_updates %lld exceeds the plan's %lld", (long long)n_updates,
               (long long)p->n_updates);
  if (p->use_graph) BSIG_TRY(ensure_graphs(p));
  return enqueue_updates(p, n_updates, as_stream(stream));
}

extern "C" int bsig_fit_run(bsig_fit_plan* p, int64_t n_updates, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit_run");
  BSIG_REQUIRE(p && p->bound, "fit_run: plan not bound");
  BSIG_REQUIRE(n_updates >= 0 && n_updates <= p->n_updates,
               "fit_run: n_updates %lld exceeds the plan's %lld", (long long)n_updates,
               (long long)p->n_updates);
  hipStream_t st = as_stream(stream);
  if (p->use_graph) BSIG_TRY(ensure_graphs(p));
  // plans covered by a persistent kernel: the whole call, evaluations included, is ONE launch
  if (engine(p) && !p->split_adam && n_updates >= 1 && p->buf.n_test >= 1 &&
      evals_in_launch(p, false, p->buf.x_test_factors != nullptr))
    return enqueue_persistent(p, (int)n_updates, st, (int)n_updates, nullptr, nullptr, true);
  const int64_t every = eval_every(n_updates);
  int64_t done = 0;
  for (int64_t it = 0; it < n_updates; ++it) {
    if (is_logging_point(it, n_updates, every)) {
      BSIG_TRY(enqueue_updates(p, it + 1 - done, st));   // the run of updates up to here
      done = it + 1;
      BSIG_TRY(bsig_fit_eval(p, stream));
    }
  }
  return BSIG_OK;
}

namespace bsig {
// [train_loss at the logging points | test_loss | flag word] of one call, for its single read-back
__global__ void pack_logs_kernel(const float* train_loss, const float* test_loss,
                                 const int32_t* state, int n_updates, int n_evals, float* out) {
  pack_call_logs(train_loss, test_loss, state, n_updates, eval_every(n_updates), n_evals, out, (int)threadIdx.x,
                 (int)blockDim.x);
}
}  // namespace bsig

extern "C" int bsig_fit_pack_logs(bsig_fit_plan* p, int64_t n_updates, float* out,
                                  bsig_stream_t stream) {
  BSIG_REQUIRE(p && p->bound && out, "fit_pack_logs: plan not bound / null");
  BSIG_REQUIRE(n_updates >= 0 && n_updates <= p->n_updates, "fit_pack_logs: bad n_updates");
  hipLaunchKernelGGL(pack_logs_kernel, dim3(1), dim3(64), 0, as_stream(stream), p->buf.train_loss,
                     p->buf.test_loss, p->buf.state, (int)n_updates, (int)count_logging_points(n_updates), out);
  BSIG_CHECK_LAUNCH("pack_logs");
  return BSIG_OK;
}

namespace bsig {
// pack_logs_kernel for every chunk of a block (workgroup c: chunk c; stride floats per chunk)
__global__ void pack_block_logs_kernel(const float* train_loss, const float* test_loss, const int32_t* state,
                                       const bsig_fit_chunk* chunks, int n_evals, float* out) {
  const bsig_fit_chunk ch = chunks[blockIdx.x];
  pack_call_logs(train_loss + ch.train_slot, test_loss + ch.test_slot, state, ch.n_updates, ch.eval_every, n_evals,
                 out + (int64_t)blockIdx.x * (2 * n_evals + 1), (int)threadIdx.x, (int)blockDim.x);
}
}  // namespace bsig

extern "C" int bsig_debug_fit_deferred(const bsig_fit_plan* p, int64_t* out) {
  BSIG_REQUIRE(p && out, "debug_fit_deferred: null");
  out[0] = p->n_deferred; out[1] = p->n_in_launch; out[2] = (int64_t)p->deferred.bytes;
  return BSIG_OK;
}

extern "C" int bsig_debug_block_launch(int engine_kind, int eval_in_launch, int forced_single) {
  return block_launch_resolved(engine_kind, eval_in_launch != 0, forced_single != 0) ? 1 : 0;
}

extern "C" int bsig_debug_fit_schedule(int n_updates, int step0, int n, int32_t* out, int cap) {
  BSIG_REQUIRE(out && n_updates >= 0 && step0 >= 0 && n >= 0 && (int64_t)step0 + n <= n_updates &&
               (int64_t)cap >= 3 + 2 * (int64_t)n_updates, "debug_fit_schedule: negative argument or short out");
  const int every = eval_every(n_updates);
  out[0] = every; out[1] = count_logging_points(n_updates);
  out[2] = evals_in_run(step0, n, n_updates, every, true);
  for (int it = 0; it < n_updates; ++it) {
    out[3 + 2 * it] = is_logging_point(it, n_updates, every) ? 1 : 0;
    out[4 + 2 * it] = evals_before(it, every);
  }
  return BSIG_OK;
}

extern "C" int bsig_fit_block_chunks(const bsig_fit_plan* p, int64_t n_train) {
  if (!p || !p->bound || p->split_adam || engine(p) != 1 || !p->eng.block_launch) return 0;
  if (n_train < 1 || !feat_cache_applies(p, n_train) || p->n_updates < 1) return 0;
  // (the tags: fewer than 2^30 updates in a launch)
  return (int)std::min<int64_t>(((int64_t)1 << 30) / (p->n_updates + 1), 1 << 16);
}

extern "C" int bsig_fit_run_block(bsig_fit_plan* p, const float* feats, int64_t ld_feats, int64_t rows,
                                  const float* y, int64_t ldy, const int32_t* ids, int64_t n_ids,
                                  const bsig_fit_chunk* chunks_host, const bsig_fit_chunk* chunks_dev, int n_chunks,
                                  float* train_loss, float* test_loss, float* packed_logs, int64_t norm_batch,
                                  bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit_run_block");
  BSIG_REQUIRE(p && p->bound && feats && y && ids && chunks_host && chunks_dev && train_loss && test_loss &&
               packed_logs, "fit_run_block: plan not bound / null");
  BSIG_REQUIRE(n_chunks >= 1 && n_chunks <= bsig_fit_block_chunks(p, 1),
               "fit_run_block: this plan runs one chunk per launch (bsig_fit_block_chunks)");
  BSIG_REQUIRE(rows >= 1 && ld_feats >= p->cfg.rff_feats && ld_feats % 4 == 0 && aligned(feats, 16) &&
               ldy >= p->cfg.head.out_dim && n_ids >= 0, "fit_run_block: bad block");
  const int n_upd = (int)p->n_updates, every = eval_every(n_upd), n_ev = (int)p->n_evals;
  int max_test = 0;
  for (int c = 0; c < n_chunks; ++c) {
    const bsig_fit_chunk& k = chunks_host[c];
    BSIG_REQUIRE(k.n_updates == n_upd && k.eval_every == every && k.upd_base == c * n_upd && k.eval_base == c * n_ev &&
                 k.train_slot == k.upd_base && k.test_slot == k.eval_base,
                 "fit_run_block: chunk %d: updates, evaluation schedule or slots out of step with the plan", c);
    BSIG_REQUIRE(k.n_train >= 1 && k.n_test >= 1 && k.n_test <= p->max_test && feat_cache_applies(p, k.n_train) &&
                 k.row0 >= 0 && k.row0 + k.n_train + k.n_test <= rows,
                 "fit_run_block: chunk %d: rows %lld + %d + %d outside the block's %lld (or more than the plan covers)",
                 c, (long long)k.row0, k.n_train, k.n_test, (long long)rows);
    BSIG_REQUIRE(k.ids_off == (int64_t)k.upd_base * p->batch && k.ids_off + (int64_t)n_upd * p->batch <= n_ids,
                 "fit_run_block: chunk %d: ids outside the table", c);
    max_test = std::max(max_test, k.n_test);
  }
  BSIG_TRY(fit_begin(p, chunks_host[0].seed, norm_batch, stream, false));
  hipStream_t st = as_stream(stream);
  const BlockRun blk{feats, ld_feats, y, ldy, ids, chunks_dev, n_chunks, max_test, n_chunks * n_upd, train_loss, test_loss};
  BSIG_TRY(enqueue_persistent(p, n_upd, st, n_upd, nullptr, &blk, true));
  hipLaunchKernelGGL(pack_block_logs_kernel, dim3(n_chunks), dim3(64), 0, st, train_loss, test_loss, p->buf.state,
                     chunks_dev, n_ev, packed_logs);
  BSIG_CHECK_LAUNCH("pack_block_logs");
  return BSIG_OK;
}

namespace bsig {
// the data-parallel rank's logs, ready to be summed over the ranks
__global__ void pack_dp_logs_kernel(const float* train_loss, const float* test_loss,
                                    const int32_t* state, int n_updates, int n_evals, float n_test,
                                    float* out) {
  const int n = n_updates + n_evals + 3;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    float v;
    if (i < n_updates) v = train_loss[i];
    else if (i < n_updates + n_evals) v = n_test > 0.f ? test_loss[i - n_updates] * n_test : 0.f;
    else if (i == n_updates + n_evals) v = n_test;
    else v = (state[ST_FLAGS] >> (i - n_updates - n_evals - 1)) & 1 ? 1.f : 0.f;
    out[i] = v;
  }
}
}  // namespace bsig

// A steady-state update of a data-parallel rank whose updates run in the persistent kernel of the
// linear heads -- the launch that takes the pending Adam step and writes this update's gradients,
// then RCCL's all-reduce of the flat gradient buffer -- captured into ONE HIP graph (SURVEY.md
// 8(e)).  Nothing in the launch's arguments changes from update to update (everything per-step is
// resolved on the device).  BSIG_DP_GRAPH=0 keeps the direct calls; a failed capture is recorded
// (bsig_fit_dp_graph_status) and the direct calls are used.
// The gradient exchange of a data-parallel update.  (tests) BSIG_DEBUG_GRAD_EXCHANGE_SCALE=s multiplies
// the exchanged gradients by s, as s identical peers would: the all-reduce of a 1-rank group is the
// identity, which cannot tell a rank that takes its Adam step from the REDUCED buffer from one that
// keeps its own gradients -- with s != 1 every path must consume what the exchange left in memory.
__global__ void debug_scale_kernel(float* buf, int64_t n, float s) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    buf[i] *= s;
}
static int allreduce_grads(bsig_fit_plan* p, bsig_comm* comm, bsig_stream_t stream) {
  BSIG_TRY(bsig_comm_allreduce(comm, p->buf.grads, p->L.total, stream));
  if (const char* e = getenv("BSIG_DEBUG_GRAD_EXCHANGE_SCALE")) {
    const float s = (float)atof(e);
    if (s != 1.0f) {
      // 8 workgroups: ONE per XCD is what a kernel on the exchange stream can have while a resident launch
      // holds 248 CUs -- measured with this stand-in (BSIG_DEBUG_GRAD_EXCHANGE_GRID): grids of 1 and 8
      // run, 9 / 16 / 32 / 64 / 256 never get their last workgroups placed and every call times out
      // (profiles/r05_NOTES.md).  The same bound is why comm.cpp caps RCCL at 8 channels for a resident rank.
      const char* ge = getenv("BSIG_DEBUG_GRAD_EXCHANGE_GRID");
      const int grid = ge ? std::max(atoi(ge), 1) : 8;
      hipLaunchKernelGGL(debug_scale_kernel, dim3(grid), dim3(1024), 0, as_stream(stream), p->buf.grads, p->L.total, s);
      BSIG_CHECK_LAUNCH("debug_scale");
    }
  }
  return BSIG_OK;
}

static int ensure_dp_graph(bsig_fit_plan* p, bsig_comm* comm) {
  if (p->g_dp_state == 1 && p->g_dp_comm == comm) return BSIG_OK;
  if (p->g_dp_state < 0 && p->g_dp_comm == comm) return BSIG_OK;
  if (p->g_dp) { (void)hipGraphExecDestroy(p->g_dp); p->g_dp = nullptr; }
  p->g_dp_comm = comm; p->g_dp_error[0] = 0;
  const char* env = getenv("BSIG_DP_GRAPH");
  if (!p->use_graph || engine(p) != 1 || bsig_comm_transport(comm) != 1 || !(env && env[0] == '1')) {
    p->g_dp_state = -2;
    snprintf(p->g_dp_error, sizeof(p->g_dp_error), "%s",
             !(env && env[0] == '1') ? "not requested (BSIG_DP_GRAPH=1)" :
             bsig_comm_transport(comm) != 1 ? "the exchange is not RCCL" : "the plan's updates are not one launch each");
    return BSIG_OK;
  }
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamBeginCapture(p->cap_stream, hipStreamCaptureModeRelaxed);
  int rc = BSIG_OK;
  if (e == hipSuccess) {
    p->adam_pending = true;
    rc = enqueue_persistent(p, 1, p->cap_stream, dp_eval_total(p));
    if (rc == BSIG_OK) rc = allreduce_grads(p, comm, reinterpret_cast<bsig_stream_t>(p->cap_stream));
    e = hipStreamEndCapture(p->cap_stream, &graph);
  }
  if (e == hipSuccess && rc == BSIG_OK) e = hipGraphInstantiate(&p->g_dp, graph, nullptr, nullptr, 0);
  if (graph) (void)hipGraphDestroy(graph);
  if (e != hipSuccess || rc != BSIG_OK || !p->g_dp) {
    snprintf(p->g_dp_error, sizeof(p->g_dp_error), "capture of launch + ncclAllReduce failed: %s",
             rc != BSIG_OK ? bsig_last_error() : hipGetErrorString(e));
    (void)hipGetLastError();
    p->g_dp = nullptr; p->g_dp_state = -1;
    return BSIG_OK;
  }
  p->g_dp_state = 1;
  return BSIG_OK;
}

extern "C" int bsig_fit_dp_graph_status(const bsig_fit_plan* p, char* msg, size_t msg_bytes) {
  if (!p) return 0;
  if (msg && msg_bytes) snprintf(msg, msg_bytes, "%s", p->g_dp_error);
  return p->g_dp_state;
}

// A data-parallel rank covered by a chip-resident persistent kernel (the linear heads, or the two-layer
// MDNN whose first layer fits the chip) can stay RESIDENT across the gradient exchange: ONE launch for
// the call (weights in LDS, moments in registers, held-out evaluations inside, as a single rank), and
// a second stream that per update waits for the kernel's "gradients are out" word, runs the
// all-reduce and writes the word the kernel polls (fit_persistent.hip: XR; persist_mdnn_device.h:
// xr).  No launch boundary and no W / m / v / g round trip through HBM per update.
// Policy (round 6: FROZEN, opt-in everywhere): BSIG_DP_RESIDENT=1 or bsig_comm_set_resident(comm, 1) asks
// for it; unset, every rank runs one launch per update.  Round 5 had it on by default for 1-rank groups
// (all this pool can run: cfg5 29.5 us per update against 34.8 with a launch per update, cfg3 39 against
// 47) -- with one resident call in some 38 000 timing out for a reason nobody found, i.e. an unexplained
// retry on a default path.  With peers it additionally needs RCCL's channels capped when the
// communicator came up (comm.cpp: its kernels have to live on the 8 CUs the launch leaves free) and an
// exchange stream that is served on EVERY rank (comm_xr_group_usable); no run with a peer has happened
// yet.  The exchange stream is chosen by a probe (comm.h); when none is served promptly the call falls
// back to a launch per update, and a launch whose polls time out anyway makes the fit repeat (mdnn.py:
// first without the residency, then on the per-phase kernels), with a warning.
static bool dp_resident_applies(const bsig_fit_plan* p, const bsig_comm* comm, int64_t n_updates) {
  const char* e = getenv("BSIG_DP_RESIDENT");
  const int mode = bsig_comm_resident_mode(comm);      // (bsig_comm_set_resident overrides the policy)
  bool want = mode >= 0 ? mode == 1 : (e && e[0] == '1');
  if (want && !bsig::comm_resident_allowed(comm)) {
    static bool told = false;
    if (!told) fprintf(stderr, "bayes_sim_ig_amd: a rank with peers can stay resident across the gradient exchange only if "
                               "BSIG_DP_RESIDENT=1 was set when its communicator was created (RCCL's channels are capped "
                               "then): one launch per update instead\n");
    told = true;
    want = false;
  }
  // (the two-layer MDNN: with its first layer resident on the chip -- a streamed one takes factor
  // rows, whose held-out pairs a resident launch does not evaluate)
  return want && bsig_comm_transport(comm) == 1 && n_updates >= 1 && n_updates == p->n_updates && !p->adam_pending &&
         engine(p) && p->buf.n_test >= 1 && evals_in_launch(p, false, false) &&
         (engine(p) != 1 || p->buf.x_kind == BSIG_X_ROWS);
}

static int run_dp_resident(bsig_fit_plan* p, bsig_comm* comm, int64_t n_updates, hipStream_t st) {
  const auto t0_host = std::chrono::steady_clock::now();
  CommXr xr;
  BSIG_TRY(comm_xr(comm, st, &xr));
  // At most `depth` calls in flight on the exchange stream: the host waits for the end of call c - depth
  // before it enqueues the exchange of call c (the launch of call c is in `st` by then, the GPU does not
  // idle).  1: with 3 calls or more of stream operations outstanding, calls timed out once ~65 000
  // operations had gone through the stream (always around the 210th call of a process; depth 1 and 2
  // ran 400+ calls clean, same speed).
  constexpr int depth = 1;
  const int slot = (int)(xr.calls % CommXr::kRing);
  BSIG_HIP(hipEventRecord(xr.ev_begin[slot], st));
  BSIG_HIP(hipStreamWaitEvent(xr.stream, xr.ev_begin[slot], 0));
  BSIG_TRY(enqueue_persistent(p, (int)n_updates, st, (int)n_updates, &xr));
  if (xr.calls >= depth)
    BSIG_HIP(hipEventSynchronize(xr.ev_end[(int)((xr.calls - depth) % CommXr::kRing)]));
  // (tests: BSIG_DP_XR_DROP_CALL=k leaves the k-th resident call of the communicator, 0-based, without
  // its exchange -- the launch's bounded polls give up, as when the exchange stream is not served)
  const char* drop = getenv("BSIG_DP_XR_DROP_CALL");
  const bool dropped = drop && atoll(drop) == xr.calls;
  for (int64_t u = 1; u <= (dropped ? 0 : n_updates); ++u) {
    BSIG_HIP(hipStreamWaitValue32(xr.stream, xr.ready, xr.base + (uint32_t)u, hipStreamWaitValueGte, 0xFFFFFFFFu));
    BSIG_TRY(allreduce_grads(p, comm, reinterpret_cast<bsig_stream_t>(xr.stream)));
    BSIG_HIP(hipStreamWriteValue32(xr.stream, xr.done, xr.base + (uint32_t)u, 0));
  }
  BSIG_HIP(hipEventRecord(xr.ev_end[slot], xr.stream));
  BSIG_TRY(comm_xr_advance(comm, (unsigned)n_updates));
  if (getenv("BSIG_DP_XR_TRACE")) {
    // (diagnostics) the time-out bit behind every resident call so far, read without a sync (-1: in flight)
    static int32_t* hist = nullptr; static int n_hist = 0;
    constexpr int kHist = 4096;
    if (!hist) {
      BSIG_HIP(hipHostMalloc(reinterpret_cast<void**>(&hist), kHist * 4, 0));
      for (int i = 0; i < kHist; ++i) hist[i] = -1;
    }
    if (n_hist < kHist) BSIG_HIP(hipMemcpyAsync(&hist[n_hist++], p->buf.state + ST_FLAGS, 4, hipMemcpyDeviceToHost, st));
    const auto t1 = std::chrono::steady_clock::now();
    fprintf(stderr, "run_dp_resident: %lld updates enqueued in %.1f us of host time; time-out bits so far:", (long long)n_updates,
            std::chrono::duration<double, std::micro>(t1 - t0_host).count());
    for (int i = 0; i < n_hist; ++i) fprintf(stderr, " %d", (int)hist[i]);
    fprintf(stderr, "\n");
  }
  return BSIG_OK;
}

extern "C" int bsig_fit_run_dp(bsig_fit_plan* p, bsig_comm* comm, int64_t n_updates,
                               float* reduced_logs, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_fit_run_dp");
  BSIG_REQUIRE(p && p->bound && p->split_adam, "fit_run_dp: plan not bound with SPLIT_ADAM");
  BSIG_REQUIRE(comm, "fit_run_dp: null communicator");
  BSIG_REQUIRE(n_updates >= 0 && n_updates <= p->n_updates,
               "fit_run_dp: n_updates %lld exceeds the plan's %lld", (long long)n_updates,
               (long long)p->n_updates);
  BSIG_REQUIRE(p->norm_batch == p->batch * bsig_comm_world(comm),
               "fit_run_dp: bsig_fit_begin's norm_batch %lld != batch %lld x world %d",
               (long long)p->norm_batch, (long long)p->batch, bsig_comm_world(comm));
  if (p->use_graph) BSIG_TRY(ensure_graphs(p));
  const int64_t every = eval_every(n_updates);
  int64_t n_evals = 0;
  // (the word the workgroups of a resident launch count themselves in is zeroed by bsig_fit_begin: one
  // resident call per begin, a further call continues with a launch per update)
  bool resident = !p->resident_ran && dp_resident_applies(p, comm, n_updates);
  if (resident) {      // ... and an exchange stream that is answered while a kernel runs on `stream` (comm.h)
    CommXr xr;
    BSIG_TRY(comm_xr(comm, as_stream(stream), &xr));
    bool usable = xr.usable;
    BSIG_TRY(bsig::comm_xr_group_usable(comm, as_stream(stream), &usable));
    if (!usable) {
      static bool told = false;
      if (!told) fprintf(stderr, "bayes_sim_ig_amd: BSIG_DP_RESIDENT=1, but no exchange stream of this process is served while a "
                                 "kernel runs on the fit's stream (best probe %.0f us): one launch per update instead\n",
                         std::min(std::min(xr.probe_us[0], xr.probe_us[1]), std::min(xr.probe_us[2], xr.probe_us[3])));
      told = true;
      resident = false;
    }
  }
  if (resident) {
    BSIG_TRY(run_dp_resident(p, comm, n_updates, as_stream(stream)));
    p->resident_ran = true;
    n_evals = count_logging_points(n_updates);
  }
  const bool was_pending = p->adam_pending;
  if (!resident) BSIG_TRY(bsig::comm_xr_drain(comm));     // (stale all-reduces of a resident call that gave up)
  if (!resident) BSIG_TRY(ensure_dp_graph(p, comm));
  p->adam_pending = was_pending;
  for (int64_t it = 0; it < (resident ? 0 : n_updates); ++it) {
    if (p->g_dp_state == 1 && p->adam_pending) {
      // steady state: the captured launch (pending Adam step in, gradients out) + all-reduce
      BSIG_HIP(hipGraphLaunch(p->g_dp, as_stream(stream)));
      p->adam_pending = true;
    } else {
      BSIG_TRY(bsig_fit_grad(p, stream));
      BSIG_TRY(allreduce_grads(p, comm, stream));
      BSIG_TRY(bsig_fit_apply(p, stream));
    }
    if (is_logging_point(it, n_updates, every)) { BSIG_TRY(bsig_fit_eval(p, stream)); ++n_evals; }
  }
  BSIG_TRY(bsig_fit_flush(p, stream));
  if (reduced_logs) {
    hipLaunchKernelGGL(pack_dp_logs_kernel, dim3(1), dim3(256), 0, as_stream(stream),
                       p->buf.train_loss, p->buf.test_loss, p->buf.state, (int)n_updates,
                       (int)n_evals, (float)p->buf.n_test, reduced_logs);
    BSIG_CHECK_LAUNCH("pack_dp_logs");
    BSIG_TRY(bsig_comm_allreduce(comm, reduced_logs, n_updates + n_evals + 3, stream));
  }
  return BSIG_OK;
}

// tests: keep `blocks` CUs busy (workgroups holding lds_bytes of LDS) for `ms` milliseconds
extern "C" int bsig_debug_spin(int blocks, size_t lds_bytes, int ms, bsig_stream_t stream) {
  return debug_spin(blocks, lds_bytes, ms, as_stream(stream));
}

// diagnostics (tools/persist_prof.py): phase time stamps of the persistent kernel
extern "C" void bsig_debug_persist_profile(void* buffer) { persist_set_profile_buffer(buffer); }
namespace bsig {
// (tests) The owners' fma-chain head outputs (persist_mdnn_device.h: heads_fma_chain) rest on one property
// of the hardware: v_mfma_f32_16x16x4_f32 adds its four products as a chain of fused multiply-adds in
// ascending k (= lane group).  One wavefront: D = A [16][K] B [K][16] by a chain of K / 4 MFMAs, and the
// same sums as fmaf chains on the vector ALU; counts the outputs whose bits differ.
__global__ void mfma_vs_fma_kernel(const float* A, const float* B, int K, int32_t* mismatches) {
  typedef float v4 __attribute__((ext_vector_type(4)));
  const int l = threadIdx.x, r = l & 15, g = l >> 4;
  v4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 4)
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(A[r * K + k0 + g], B[(k0 + g) * 16 + r], acc, 0, 0, 0);
  int bad = 0;
  for (int v = 0; v < 4; ++v) {
    const int i = 4 * g + v;           // D[i][r]
    float c = 0.f;
    for (int k = 0; k < K; ++k) c = __builtin_fmaf(A[i * K + k], B[k * 16 + r], c);
    bad += __float_as_uint(c) != __float_as_uint(acc[v]) ? 1 : 0;
  }
  if (bad) atomicAdd(mismatches, bad);
}
}  // namespace bsig

extern "C" int bsig_debug_mfma_vs_fma(const float* a, const float* b, int k, int32_t* mismatches,
                                      bsig_stream_t stream) {
  BSIG_REQUIRE(a && b && mismatches && k >= 4 && k % 4 == 0, "debug_mfma_vs_fma: null / K not a multiple of 4");
  hipLaunchKernelGGL(bsig::mfma_vs_fma_kernel, dim3(1), dim3(64), 0, as_stream(stream), a, b, k, mismatches);
  BSIG_CHECK_LAUNCH("mfma_vs_fma");
  return BSIG_OK;
}

extern "C" int bsig_debug_persist_mdnn_geometry(int batch, int input_dim, int out_dim, int n_comp, int full_cov,
                                                int max_test, int32_t* out) {
  if (!out) return 0;
  return persist_mdnn_geometry(PersistMdnnShape{batch, input_dim, 128, 128, BSIG_ACT_TANH, out_dim, n_comp,
                                                full_cov, max_test}, out);
}
extern "C" int bsig_debug_persist_geometry(int batch, int feat_dim, int out_dim, int n_comp, int max_test,
                                           int32_t* out) {
  if (!out) return 0;
  const PersistShape s{batch, feat_dim, out_dim, n_comp, max_test};
  const int rc = persist_geometry(s, out);
  // which kernel a launch of this shape would really be (asks the device; 0 where there is none)
  UGeom g;
  PersistEngine e;
  out[13] = persist_resolve(s, &g, &e) ? 2 : 0;
  return rc;
}
