// Persistent update kernel of the fit engine (fit_persistent.hip): a run of
// consecutive Adam updates of a linear mixture-density head on precomputed
// features (MDRFF with the hoisted RFF projection) in ONE launch.  What both
// persistent engines share (this one and persist_mdnn.h) is declared here too.
#pragma once
#include "common.h"

namespace bsig {

// The persistent update engine of a fit plan, resolved once when the plan is created
// (persist_resolve / persist_mdnn_resolve); every entry point of the plan reads it.
struct PersistEngine {
  int kind = 0;                 // 0: none (per-phase kernels), 1: linear heads (this file), 2: two-layer MDNN
  bool streams = false;         // (MDNN) the first layer is streamed: cross-correlation factor rows only
  bool eval_single = false;     // a single rank's call evaluates its held-out rows inside the launch
  bool eval_dp = false;         // ... and so do a data-parallel rank's launches (one per update)
  bool block_launch = false;    // one launch may run several chunks of a fit (bsig_fit_run_block): linear heads with
                                // the evaluations inside the launch (block_launch_resolved; single rank: the callers ask)
  size_t workspace_bytes = 0;
};

// the "several chunks per launch" answer of an engine (forced_single: BSIG_FIT_CHUNK_PER_LAUNCH=1)
inline bool block_launch_resolved(int kind, bool eval_single, bool forced_single) {
  return kind == 1 && eval_single && !forced_single;
}

struct PersistShape {
  int batch, feat_dim, out_dim, n_comp;
  int max_test = 0;   // held-out rows the plan may evaluate inside the launches (0: none)
};

// The tiling fit_persistent.hip plans for a shape (host only)
struct UGeom {
  int NT, Bp, MT, FP, KS, ksteps, KB, WP, Nh, NhP, n_blocks, k_slices, G, T, n_owner, R;
  int per_wave, xs_floats;
  int eval_passes, NE, RE;      // eval_passes 0: evaluations stay outside the launches
  size_t lds, slab_floats, dout_floats, eval_floats;
};

struct PersistHyper {
  double lr, beta1, beta2; float adam_eps, eps_noise, min_weight, ll_limit;
  int64_t norm_batch;
};

// What the launches of both engines take
struct PersistCommon {
  const float* y; int64_t ldy;            // targets, gathered through ids
  const int32_t* ids;                     // [n_updates*batch] minibatch row ids
  float* params; float* exp_avg; float* exp_avg_sq;   // flat buffers
  int32_t* state;                         // the fit engine's 16-word state block (fit_protocol.h)
  float* train_loss;                      // [n_updates]
  void* workspace; size_t workspace_bytes;
  // data-parallel ranks (null / 0 otherwise): the gradients of the update go to
  // `grads` (flat layout) for the caller's all-reduce instead of into Adam; with
  // `adam_pending` the launch first takes the Adam step of the previous update
  // from the (reduced) `grads`.  n = 0 with adam_pending: that step only.
  float* grads = nullptr; int adam_pending = 0;
  // ... or RESIDENT across the exchange (plans whose evaluations run inside the launch; the MDNN:
  // its first layer resident on the chip): ONE launch for the whole call; after update u (1-based) the
  // kernel writes its gradients through to `grads`, raises *xr_ready to xr_base + u (a word a stream can
  // wait on) and polls *xr_done until the caller's exchange stream has written the same number behind
  // its all-reduce.  The two words only ever grow (xr_base: the updates of earlier calls): nothing has
  // to reset them between calls, so no stream operation of one call has to be ordered against the
  // exchange of another.
  unsigned* xr_ready = nullptr; const unsigned* xr_done = nullptr; unsigned xr_base = 0;
  // held-out evaluations inside the launch (PersistEngine::eval_*): after update `it` of the call
  // with it % eval_every == 0 and after the last of its n_total updates (mdnn.py:235-242);
  // evaluation k writes test_loss[state[ST_EVAL]] and advances that word (fit_protocol.h)
  int do_eval = 0; int eval_every = 1; int n_total = 0; int n_test = 0;
  const float* y_test = nullptr; int64_t ldy_test = 0;
  float* test_loss = nullptr;
  PersistHyper hy;
};

struct PersistBuffers : PersistCommon {
  const float* feats; int64_t ld_feats;   // feature rows
  const int32_t* feat_ids;                // minibatch row i of update `step` = feats[feat_ids[step*batch+i]]
                                          // (null: feats[step*batch + i])
  int64_t w_off, b_off;                   // head weights [Nh, feat_dim] / bias [Nh] inside the flat buffers
  int64_t eval_row0 = 0;                  // held-out rows: feats[eval_row0 .. +n_test)
  // A block of chunks in one launch (bsig.h: bsig_fit_chunk; device memory, checked by the caller): feats, y, ids
  // (= feat_ids), train_loss and test_loss are the block's, n_test the most of any chunk, n_total the updates of
  // the whole launch; every chunk evaluates inside the launch.  null: one chunk, described by the fields above.
  const bsig_fit_chunk* chunks = nullptr; int n_chunks = 1;
  // Deferred evaluations (single rank, do_eval): the plan's DeferredEval memory, reserved for at least the
  // evaluations of this launch.  The update launch then only snapshots the weight tiles at the evaluation points
  // and deferred_eval_run, enqueued behind it, evaluates from the snapshots.  null: evaluations inside the launch.
  void* deferred = nullptr;
};

// ---- held-out evaluations behind the update launch (fit_deferred_eval.hip) ---------------------------------
// Device memory of a plan's deferred evaluations: [copy of the state block | snapshots of the weight tiles at
// the evaluation points of a launch | partial products, row sums and owner sums of a GROUP of evaluations].
// Allocated at the first launch that needs it (and again when a launch holds more evaluations), freed with the plan.
struct DeferredEval { void* mem = nullptr; size_t bytes = 0; int n_evals = 0; };
// The most a plan's snapshots may take (BSIG_DEFERRED_EVAL_CAP_MB overrides: tests): a launch whose evaluations
// need more keeps them inside the launch.
constexpr size_t kDeferredSnapCapBytes = (size_t)2 << 30;
// bytes the partial products of a group of evaluations may take (the evaluations of a launch run in groups)
constexpr size_t kDeferredGroupBytes = (size_t)96 << 20;
size_t deferred_eval_snapshot_bytes(const UGeom& g, int n_evals);
// true: *d holds a launch of n_evals evaluations (false: over the cap, or no memory -- evaluate inside the launch)
bool deferred_eval_reserve(const UGeom& g, int n_evals, DeferredEval* d);
void deferred_eval_free(DeferredEval* d);
// the evaluations of the launch persist_run(s, g, b, n, st) made with b.deferred set, on the same stream
int deferred_eval_run(const PersistShape& s, const UGeom& g, const PersistBuffers& b, int n, hipStream_t st);

// The tiling of a shape and whether the device can hold every workgroup of its launch at once (asks
// the device and raises the kernels' dynamic-LDS limit: once per plan).  false: not covered, *g and
// *e as they were.
bool persist_resolve(const PersistShape& s, UGeom* g, PersistEngine* e);
// what must be zero at the start of a fit call (cross-workgroup flags, granules, the padding of
// the d_out rows): two regions of the workspace, cleared by the engine's begin kernel
struct ZeroRegion { void* ptr; size_t bytes; };
int persist_reset_regions(const UGeom& g, void* workspace, size_t workspace_bytes, ZeroRegion* regions);
// n consecutive updates starting at the state block's step counter; advances
// the counter, the jitter RNG stream and the Adam bias-correction powers
int persist_run(const PersistShape& s, const UGeom& g, const PersistBuffers& b, int n, hipStream_t st);

// (diagnostics) the tiling fit_persistent.hip plans for a shape, bsig.h: bsig_debug_persist_geometry
int persist_geometry(const PersistShape& s, int32_t* out);

// The > 64 KB dynamic-LDS limit of every kernel of a launcher, raised on the current device (a plan's,
// while its engine is resolved): common.h's raise_lds_limit per kernel, `raised[i]` being kernels[i]'s.
template <int N>
inline int allow_dynamic_lds(LdsRaised (&raised)[N], const void* const (&kernels)[N], int bytes) {
  for (int i = 0; i < N; ++i) BSIG_TRY(raise_lds_limit(kernels[i], bytes, &raised[i]));
  return BSIG_OK;
}

// diagnostics: [256][8][16] int64 wall-clock stamps of the first 8 updates of every
// following launch (null: off)
void persist_set_profile_buffer(void* buf);
// (tests) occupy `blocks` CUs (workgroups holding lds_bytes of LDS) for `ms` milliseconds
int debug_spin(int blocks, size_t lds_bytes, int ms, hipStream_t st);
void* persist_profile_buffer();

}  // namespace bsig
