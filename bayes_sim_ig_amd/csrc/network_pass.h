// The estimator's per-phase network pass, stated once for fp32 (estimator.hip) and fp64
// (f64/estimator_f64.hip): the flat parameter layout, the workspace carve, and the sequence of
// products of a forward (mdnn.py:108-119 / mdrff.py:28-30) and a backward pass.
//
// T is the element type.  What only one precision has sits behind `if constexpr (kF32<T>)` or one
// of the overloads of run_gemm / colsum_launch below: the fp32 products go through the router of
// gemm_f32.hip (workspace, matmul precision, row offsets resolved on the device for graph replay,
// fused Adam, the head product's side outputs), the fp64 ones through f64::gemm_run as they stand.
#pragma once
#include "flat_ops.h"
#include "gemm.h"
#include "head.h"
#include "f64/f64.h"
#include "../../include/bsig_matmul.h"

#include <algorithm>
#include <type_traits>

namespace bsig {

template <typename T> constexpr bool kF32 = std::is_same<T, float>::value;
template <typename T> using GemmOf = typename std::conditional<kF32<T>, GemmParams, f64::Gemm>::type;

static inline int run_gemm(GemmParams& g, void* ws, size_t ws_bytes, int math, hipStream_t st, int* n_expsum = nullptr) {
  g.math = math;
  return gemm_run(g, ws, ws_bytes, st, n_expsum);
}
static inline int run_gemm(const f64::Gemm& g, void*, size_t, int, hipStream_t st, int* = nullptr) { return f64::gemm_run(g, st); }
static inline int colsum_launch(const double* x, int64_t ld, int64_t rows, int64_t cols, double* out, void*, size_t,
                         hipStream_t st) {
  return f64::colsum_launch(x, ld, rows, cols, out, st);
}
template <typename G> static void set_mnk(G& g, int64_t m, int64_t n, int64_t k) {
  g.m = static_cast<decltype(g.m)>(m); g.n = static_cast<decltype(g.n)>(n); g.k = static_cast<decltype(g.k)>(k);
}

// ---- flat parameter layout (both precisions; bsig_mdn_param_count / _offsets report it) -------
constexpr int64_t kAlign = 4;  // elements: every tensor of the float buffer starts 16-B aligned

struct Layout {
  int n_layers;                        // trunk layers
  int64_t in_dim[BSIG_MAX_HIDDEN + 1]; // input width of trunk layer l / of the heads
  int64_t w_off[BSIG_MAX_HIDDEN], b_off[BSIG_MAX_HIDDEN];
  int64_t feat_dim;                    // F: width of the heads' input
  int64_t nh;                          // Nh
  int64_t head_w_off, head_b_off;
  int64_t total;
};

static inline int make_layout(const bsig_mdn_cfg* c, Layout* L) {
  BSIG_REQUIRE(c, "cfg is null");
  BSIG_REQUIRE(c->input_dim >= 1, "cfg: input_dim must be >= 1");
  BSIG_REQUIRE(c->n_hidden >= 0 && c->n_hidden <= BSIG_MAX_HIDDEN, "cfg: bad n_hidden");
  BSIG_REQUIRE(!(c->rff_feats > 0 && c->n_hidden > 0), "cfg: MDRFF has no trunk (mdrff.py:18)");
  BSIG_REQUIRE(c->rff_feats >= 0 && (c->rff_cos_only || c->rff_feats % 2 == 0),
               "cfg: n_feat must be even (rff.py:105)");
  L->n_layers = c->n_hidden;
  int64_t off = 0, width = c->rff_feats > 0 ? c->rff_feats : c->input_dim;
  for (int l = 0; l < c->n_hidden; ++l) {
    BSIG_REQUIRE(c->hidden[l] >= 1, "cfg: hidden layer width must be >= 1");
    L->in_dim[l] = width;
    L->w_off[l] = off; off = round_up<int64_t>(off + (int64_t)c->hidden[l] * width, kAlign);
    L->b_off[l] = off; off = round_up<int64_t>(off + c->hidden[l], kAlign);
    width = c->hidden[l];
  }
  L->in_dim[c->n_hidden] = width;
  L->feat_dim = width;
  L->nh = bsig_head_width(&c->head);
  BSIG_REQUIRE(L->nh >= 1, "cfg: bad head dims");
  L->head_w_off = off; off = round_up<int64_t>(off + L->nh * width, kAlign);
  L->head_b_off = off; off = round_up<int64_t>(off + L->nh, kAlign);
  L->total = off;
  return BSIG_OK;
}

// ---- workspace carve ------------------------------------------------------
template <typename T>
struct Scratch {
  T* feat = nullptr;                // [B, F] RFF features (MDRFF, not hoisted)
  T* h[BSIG_MAX_HIDDEN] = {};       // trunk activations [B, hidden_l]
  T* dz[2] = {};                    // ping-pong [B, max hidden]
  T* o = nullptr;                   // [B, ld_o] raw head outputs
  T* d_o = nullptr;                 // [B, ld_o]
  int64_t ld_o = 0;                 // Nh -- or, float, ceil16(Nh) where the whole-width products take these buffers (gemm_wide.h)
  T* head_ws = nullptr; size_t head_ws_bytes = 0;
  size_t total_bytes = 0;
  // float only
  int32_t* tickets = nullptr;       // kWideTickets zeroed words: in-launch combine of the head product's K slices
  T* gemm_ws = nullptr; size_t gemm_ws_bytes = 0;
  T* colsum_ws = nullptr; size_t colsum_ws_bytes = 0;
  int math = BSIG_MATMUL_FP32;      // matmul precision of every product issued on this scratch (gemm.h; a plan's: plan_mem)
};

constexpr int kWideTickets = 1024;

static inline size_t gemm_ws_need(const bsig_mdn_cfg* c, const Layout& L, int64_t B) {
  size_t need = 0;
  auto upd = [&](int64_t m, int64_t n, int64_t k) {
    need = std::max(need, bsig_gemm_workspace_bytes(m, n, k));
  };
  if (c->rff_feats > 0) upd(B, c->rff_cos_only ? c->rff_feats : c->rff_feats / 2, c->input_dim);
  for (int l = 0; l < L.n_layers; ++l) {
    upd(B, c->hidden[l], L.in_dim[l]);       // forward
    upd(c->hidden[l], L.in_dim[l], B);       // dW
    if (l > 0) upd(B, L.in_dim[l], c->hidden[l]);  // dX
  }
  upd(B, L.nh, L.feat_dim);
  upd(L.nh, L.feat_dim, B);
  if (L.n_layers > 0) upd(B, L.feat_dim, L.nh);
  return need;
}

// every piece starts on a 256-byte boundary; the float-only pieces keep their place in the sequence
template <typename T>
static void carve(const bsig_mdn_cfg* c, const Layout& L, int64_t B, void* base, Scratch<T>* s) {
  *s = Scratch<T>();
  size_t off = 0;
  auto take = [&](size_t elems) {
    T* p = base ? reinterpret_cast<T*>(reinterpret_cast<char*>(base) + off) : nullptr;
    off += round_up<size_t>(elems * sizeof(T), 256);
    return p;
  };
  if (c->rff_feats > 0) s->feat = take((size_t)B * c->rff_feats);
  int64_t hmax = 0;
  for (int l = 0; l < L.n_layers; ++l) {
    s->h[l] = take((size_t)B * c->hidden[l]);
    hmax = std::max<int64_t>(hmax, c->hidden[l]);
  }
  if (hmax) { s->dz[0] = take((size_t)B * hmax); s->dz[1] = take((size_t)B * hmax); }
  // float, large minibatches of a head the whole-width kernels cover: pitch ceil16(Nh) (dO is their k-major
  // operand at exactly that pitch; the forward product stores the padded width)
  s->ld_o = (kF32<T> && B >= 2048 && gemm_wide_covers((int)L.nh) && B <= 64 * (int64_t)kWideTickets) ? round_up<int64_t>(L.nh, 16) : L.nh;
  s->o = take((size_t)B * s->ld_o);
  s->d_o = take((size_t)B * s->ld_o);
  if constexpr (kF32<T>) s->tickets = reinterpret_cast<int32_t*>(take(kWideTickets));
  s->head_ws_bytes = kF32<T> ? bsig_head_workspace_bytes(&c->head, B) : bsig_head_workspace_bytes_f64(&c->head, B);
  s->head_ws = take(s->head_ws_bytes / sizeof(T) + 1);
  if constexpr (kF32<T>) {
    s->gemm_ws_bytes = gemm_ws_need(c, L, B);
    s->gemm_ws = take(s->gemm_ws_bytes / sizeof(T) + 1);
    s->colsum_ws_bytes = (size_t)64 * std::max<int64_t>(L.nh, std::max<int64_t>(hmax, 1)) * sizeof(T);
    s->colsum_ws = take(s->colsum_ws_bytes / sizeof(T));
  }
  s->total_bytes = off;
}

// ---- passes ---------------------------------------------------------------
// Where the estimator's input rows come from.  Logical minibatch row i reads source index i -- float:
// i + (dyn[0] + delta) * dyn_stride + dyn_base, resolved on the device; f64::Gemm has no such offsets
// and the fp64 mode sets none -- looked up in `rows` when that is given.  With `is_feat` the source
// already holds RFF features (projected up front).
template <typename T>
struct Inputs {
  const T* x = nullptr; int64_t ldx = 0;
  const int32_t* rows = nullptr;
  const int32_t* dyn = nullptr; int64_t dyn_stride = 0, dyn_base = 0;
  bool is_feat = false;
  const T* rff_coeff = nullptr; int64_t ld_coeff = 0; const T* rff_offset = nullptr;
};

// Adam fused into the dW GEMMs (float, single rank)
struct AdamFuse {
  float* m; float* v; const float* dyn; float beta1, beta2, eps;
};

template <typename T>
static void set_src_a(GemmOf<T>& g, const T* x, int64_t ld, const Inputs<T>* in, int delta) {
  g.a = x; g.lda = ld; g.a_kmajor = 0;
  if (in) {
    g.a_rows = in->rows;
    if constexpr (kF32<T>) {
      g.dyn = in->dyn; g.dyn_delta = delta;
      g.a_dyn_stride = in->dyn_stride; g.a_dyn_base = in->dyn_base;
    }
  }
}
template <typename T>
static void set_src_b_kmajor(GemmOf<T>& g, const T* x, int64_t ld, const Inputs<T>* in, int delta) {
  g.b = x; g.ldb = ld; g.b_kmajor = 1;
  if (in) {
    g.b_rows = in->rows;
    if constexpr (kF32<T>) {
      g.dyn = in->dyn; g.dyn_delta = delta;
      g.b_dyn_stride = in->dyn_stride; g.b_dyn_base = in->dyn_base;
    }
  }
}

// rff.py:128-132 (122-126 cos-only); rff_scale: the cfg's in float, the call's bsig_f64_hyper's in double
template <typename T>
static int rff_project(const bsig_mdn_cfg* c, const Inputs<T>& in, T rff_scale, int64_t rows, T* feats,
                       void* ws, size_t ws_bytes, int math, hipStream_t st) {
  BSIG_REQUIRE(in.rff_coeff, "MDRFF needs rff_coeff");
  BSIG_REQUIRE(!(c->rff_cos_only && !in.rff_offset), "cos-only RFF needs an offset");
  GemmOf<T> g;
  set_src_a<T>(g, in.x, in.ldx, &in, 0);
  g.b = in.rff_coeff; g.ldb = in.ld_coeff;
  g.c = feats; g.ldc = c->rff_feats;
  set_mnk(g, rows, c->rff_cos_only ? c->rff_feats : c->rff_feats / 2, c->input_dim);
  g.epilogue = c->rff_cos_only ? BSIG_EPI_COS_OFF : BSIG_EPI_COS_SIN;
  g.bias = in.rff_offset; g.alpha = rff_scale;
  return run_gemm(g, ws, ws_bytes, math, st);
}

// trunk (or RFF) + heads -> o ; leaves activations in s.h / s.feat
template <typename T>
static int forward_pass(const bsig_mdn_cfg* c, const Layout& L, const T* params, const Inputs<T>& in,
                        T rff_scale, int64_t B, const Scratch<T>& s, T* o, int64_t ldo, hipStream_t st,
                        int* n_sig = nullptr) {
  const T* feat = in.x; int64_t ldf = in.ldx; const Inputs<T>* src = &in;
  if (c->rff_feats > 0 && !in.is_feat) {
    BSIG_TRY(rff_project(c, in, rff_scale, B, s.feat, s.gemm_ws, s.gemm_ws_bytes, s.math, st));
    feat = s.feat; ldf = c->rff_feats; src = nullptr;
  }
  for (int l = 0; l < L.n_layers; ++l) {   // nn.Linear + activation, mdnn.py:108
    GemmOf<T> g;
    set_src_a<T>(g, feat, ldf, src, 0);
    g.b = params + L.w_off[l]; g.ldb = L.in_dim[l];
    g.c = s.h[l]; g.ldc = c->hidden[l];
    set_mnk(g, B, c->hidden[l], L.in_dim[l]);
    g.epilogue = BSIG_EPI_BIAS_ACT; g.act = c->activation; g.bias = params + L.b_off[l];
    BSIG_TRY(run_gemm(g, s.gemm_ws, s.gemm_ws_bytes, s.math, st));
    feat = s.h[l]; ldf = c->hidden[l]; src = nullptr;
  }
  GemmOf<T> g;   // the four heads as one [Nh, F] product, mdnn.py:109-119
  set_src_a<T>(g, feat, ldf, src, 0);
  g.b = params + L.head_w_off; g.ldb = L.feat_dim;
  g.c = o; g.ldc = ldo;
  set_mnk(g, B, L.nh, L.feat_dim);
  g.epilogue = BSIG_EPI_BIAS; g.bias = params + L.head_b_off;
  if constexpr (kF32<T>) {
    if (o == s.o) { g.combine_tickets = s.tickets; g.combine_capacity = kWideTickets; }   // (the scratch buffer has the padded pitch the combine stores)
    if (n_sig && c->head.eps_noise != 0.f) {   // sum(exp(pre_diag)) partials for the jitter scale
      g.expsum = s.head_ws;
      g.expsum_col0 = c->head.n_comp + c->head.out_dim * c->head.n_comp;
      g.expsum_ncols = c->head.out_dim * c->head.n_comp;
    }
  }
  int n = 0;
  BSIG_TRY(run_gemm(g, s.gemm_ws, s.gemm_ws_bytes, s.math, st, &n));
  if (n_sig) *n_sig = n <= head_sig_capacity() ? n : 0;
  if (n > head_sig_capacity()) { set_error("head GEMM produced %d exp partials", n); return BSIG_EUNSUPPORTED; }
  return BSIG_OK;
}

// dW[nout, nin] = dY^T X for one layer, into grads -- or, float with `fuse`, as one Adam step on params
template <typename T>
static int weight_grad(const T* dy, int64_t nout, int64_t ld_dy, const T* xin, int64_t ldin,
                       const Inputs<T>* src, int delta, int64_t nin, int64_t B, T* params, T* grads,
                       int64_t w_off, int64_t b_off, const AdamFuse* fuse, const Scratch<T>& s,
                       hipStream_t st, const HeadBiasPartials* bias_partials = nullptr) {
  GemmOf<T> g;
  g.a = dy; g.lda = ld_dy; g.a_kmajor = 1;
  set_src_b_kmajor<T>(g, xin, ldin, src, delta);
  set_mnk(g, nout, nin, B); g.ldc = nin;
  g.c = grads + w_off;
  if constexpr (kF32<T>) {
    if (fuse) {
      g.epilogue = EPI_ADAM;
      g.c = params + w_off; g.adam_m = fuse->m + w_off; g.adam_v = fuse->v + w_off;
      g.adam_dyn = fuse->dyn; g.beta1 = fuse->beta1; g.beta2 = fuse->beta2; g.adam_eps = fuse->eps;
      g.bias_p = params + b_off; g.bias_m = fuse->m + b_off; g.bias_v = fuse->v + b_off;
      g.bias_g = grads + b_off;
      if (bias_partials && bias_partials->n > 1) {   // the finishing kernel's slab sums, added up by the reduce + Adam kernel
        g.bias_g = bias_partials->sums; g.bias_g_n = bias_partials->n; g.bias_g_stride = bias_partials->stride;
      }
    }
  }
  return run_gemm(g, s.gemm_ws, s.gemm_ws_bytes, s.math, st);
}

// backward from s.d_o (autograd through mdnn.py:108-119); the head bias gradients come from the
// head's finishing kernel.  Every product that READS a weight matrix is issued before the GEMM that
// updates it (fused Adam).  `delta` = offset of the step counter seen by these kernels relative to
// the forward half.  The first layer reads the input rows themselves: make_layout refuses a trunk on
// RFF features.
template <typename T>
static int backward_pass(const bsig_mdn_cfg* c, const Layout& L, T* params, const Inputs<T>& in,
                         int delta, int64_t B, const Scratch<T>& s, T* grads, const AdamFuse* fuse,
                         hipStream_t st, const HeadBiasPartials* bias_partials = nullptr) {
  // input of the heads
  const T* feat; int64_t ldf; const Inputs<T>* fsrc = nullptr;
  if (L.n_layers > 0) { feat = s.h[L.n_layers - 1]; ldf = c->hidden[L.n_layers - 1]; }
  else if (c->rff_feats > 0 && !in.is_feat) { feat = s.feat; ldf = c->rff_feats; }
  else { feat = in.x; ldf = in.ldx; fsrc = &in; }
  int cur = 0;
  if (L.n_layers > 0) {   // dz_L = (dO W_heads) * act'(h_L)   [reads W_heads]
    GemmOf<T> g;
    g.a = s.d_o; g.lda = s.ld_o;
    g.b = params + L.head_w_off; g.ldb = L.feat_dim; g.b_kmajor = 1;
    g.c = s.dz[cur]; g.ldc = L.feat_dim;
    set_mnk(g, B, L.feat_dim, L.nh);
    g.epilogue = BSIG_EPI_MUL_DACT; g.act = c->activation; g.aux = feat; g.ldaux = ldf;
    BSIG_TRY(run_gemm(g, s.gemm_ws, s.gemm_ws_bytes, s.math, st));
  }
  // heads: dW = dO^T feat (bias gradient = column sums of dO, from the finish kernel)
  BSIG_TRY(weight_grad(s.d_o, L.nh, s.ld_o, feat, ldf, fsrc, delta, L.feat_dim, B, params, grads,
                       L.head_w_off, L.head_b_off, fuse, s, st, bias_partials));
  for (int l = L.n_layers - 1; l >= 0; --l) {
    const int64_t hw = c->hidden[l];
    const T* xin; int64_t ldin; const Inputs<T>* xsrc = nullptr;
    if (l > 0) { xin = s.h[l - 1]; ldin = c->hidden[l - 1]; }
    else { xin = in.x; ldin = in.ldx; xsrc = &in; }
    BSIG_TRY(colsum_launch(s.dz[cur], hw, B, hw, grads + L.b_off[l], s.colsum_ws,
                           s.colsum_ws_bytes, st));
    if (l > 0) {           // dz_{l-1} = (dz_l W_l) * act'(h_{l-1})   [reads W_l]
      GemmOf<T> g;
      g.a = s.dz[cur]; g.lda = hw;
      g.b = params + L.w_off[l]; g.ldb = L.in_dim[l]; g.b_kmajor = 1;
      g.c = s.dz[cur ^ 1]; g.ldc = L.in_dim[l];
      set_mnk(g, B, L.in_dim[l], hw);
      g.epilogue = BSIG_EPI_MUL_DACT; g.act = c->activation; g.aux = xin; g.ldaux = ldin;
      BSIG_TRY(run_gemm(g, s.gemm_ws, s.gemm_ws_bytes, s.math, st));
    }
    BSIG_TRY(weight_grad(s.dz[cur], hw, hw, xin, ldin, xsrc, delta, L.in_dim[l], B, params, grads,
                         L.w_off[l], L.b_off[l], fuse, s, st));
    cur ^= 1;
  }
  return BSIG_OK;
}

}  // namespace bsig
