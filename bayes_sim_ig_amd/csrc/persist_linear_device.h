// Device code shared by the persistent update kernel of the linear heads (fit_persistent.hip) and the
// deferred held-out evaluation kernels behind it (fit_deferred_eval.hip): the launch arguments, the chunk
// and evaluation descriptors, and the arithmetic of a held-out evaluation -- the products of the held-out
// rows with a weight tile in LDS, the k-slice sums of an evaluation owner's rows, the rows' NLL and the log
// entry.  Both paths run THESE functions, in the same thread layout: an evaluation gives the same bits
// whether it runs in the waits of the update launch or in kernels of its own.
#pragma once
#include "persist.h"
#include "head_device.h"
#include "persist_device.h"

namespace bsig {

constexpr int kUT = 512;             // threads per workgroup (8 wavefronts)
constexpr int kUSteps = 18;          // 16-column steps of a k-slice a lane can hold (18 x 16 B registers)
constexpr int kUGroup = 6;           // k-slices are 1, 2 or 3 groups of 6 steps (96 / 192 / 288 columns): the
                                     // unrolled step loops branch once per group, not once per step
constexpr int kUMT = 7;              // 16-row m-tiles of the minibatch (<= 112 rows): fixed, so that the
                                     // dW product's loop over the minibatch has no run-time bound
constexpr int kUProf = 8;            // profiled updates per launch
// Pitch of the F^T / d_out^T rows in LDS (floats): minibatches of up to 112 rows.  = 4 (mod 8):
// conflict-free 16-byte reads down 8 rows and 4-byte writes across rows.  A compile-time constant:
// the 72 transposed writes of a lane per update are then immediate offsets off one address --
// with a run-time pitch the compiler keeps 72 loop-invariant addresses in registers (or scratch).
constexpr int kUFP = 116;

struct UArgs {
  int B, Bp, MT;                     // minibatch rows, padded to 16, 16-row m-tiles
  int Fdim, KS, ksteps, KB, WP;      // features, k-slice width, its 16-column steps / blocks, pitch of W rows
  int Nh, NhP, D, K;
  int n_blocks, k_slices, G, T, n_owner, R;
  int n_updates, xs_floats;
  int fast_rows;                     // (A/B runs: BSIG_PERSIST_FAST_ROWS=0 keeps the shape-generic row)
  const float* feats; int64_t ld_feats; const int32_t* feat_ids;
  const float* y; int64_t ldy; const int32_t* ids;
  float* params; float* m1; float* m2; int64_t w_off, b_off;
  int32_t* state; float* train_loss;
  double lr, beta1, beta2;
  float adam_eps, eps_noise, min_w, ll_limit, inv_norm;
  float* slabs; float* d_out; float* e_out; unsigned* flag_fwd; unsigned long long* gran;
  unsigned long long* gran_rep;      // [2][8][kGranArr] replicated granules (gran_rep())
  // data-parallel ranks (one update per launch; see PersistBuffers)
  float* grads; int adam_pending; int quad_ok;
  // data-parallel rank RESIDENT across the exchange (XR instantiation; see PersistBuffers)
  unsigned* xr_ready; const unsigned* xr_done; unsigned* xr_count; unsigned xr_base;   // (xr_count: a word of the sync region)
  // held-out evaluations inside the launch
  int do_eval, eval_every, n_total, n_test, eval_passes, NE, RE;
  int64_t eval_row0;
  const float* y_test; int64_t ldy_test;
  float* test_loss;
  float* eval_slabs;                 // [3][eval_passes][k_slices][B][NhP] (eval_passes: the most of any chunk)
  unsigned* flag_eval;               // [G]   evaluation number + 1
  unsigned long long* gran_eval;     // [2][kGranArr]
  long long* prof;                   // diagnostics: [T][kUProf][16] wall-clock stamps, or null
  int prof_t0;                       // ... of updates prof_t0 .. prof_t0 + kUProf of the launch (BSIG_PROF_T0)
  // a block of chunks in one launch (persist.h: PersistBuffers::chunks): entry c replaces, at the boundary in
  // front of chunk c, what the fields above say about ONE chunk (n_updates, n_total, eval_every, n_test,
  // eval_row0, y_test, the state block's step / seed / stream counter); feats, y, ids, train_loss and
  // test_loss are then the block's.  null: one chunk, described by the fields above (n_chunks = 1).
  const bsig_fit_chunk* chunks; int n_chunks;
  // Evaluations deferred to kernels behind the launch (SNAP instantiation; null: they run inside the launch):
  // [evaluation of the launch][tile slot][16 NT x WP weights | 16 NT biases], the weight tiles as they lie in LDS
  float* snap;
  // where u_eval_of reads the step, seed and stream counter a one-chunk call STARTED with: the state block,
  // or the copy the SNAP launch leaves in front of the snapshots for the kernels that run behind it
  const int32_t* state_in;
};
// the arguments of the launch persist_run makes of (s, g, b, n) (fit_persistent.hip)
int persist_fill_args(const PersistShape& s, const UGeom& g, const PersistBuffers& b, int n, UArgs* out);
// floats of one tile slot of a snapshot
__host__ __device__ inline int64_t u_snap_slot_floats(int NT, int WP) { return (int64_t)16 * NT * (WP + 1); }

// What a workgroup keeps of the chunk it is in (workgroup-uniform; read at the chunk boundary)
struct UCk {
  int step0, n_updates, n_total, eval_every, do_eval;
  // Flag and granule tags count the updates / evaluations of the LAUNCH (they must stay monotonic across
  // chunks): update t of the chunk has epoch ubase + step + 1, evaluation e the tag evbase + e + 1.  The
  // widest tag is epoch * 4 + 3 in 32 bits: a launch holds fewer than 2^30 updates (persist_run checks;
  // 32 chunks of 100 updates and 6 evaluations reach epoch 3200 and evaluation tag 192).  Adam, the jitter
  // streams and the evaluation schedule count chunk-local steps.
  unsigned ubase, evbase;
  // (The update loops index the ids and the train-loss log by the update of the LAUNCH, epoch - 1: the chunks'
  // ids and log slots follow each other, the ids are rows of the block; n_updates, eval_every and do_eval are the
  // same for every chunk of a launch -- the loops read the launch's arguments, which cost no live register.)
  uint64_t seed, rng_ctr0;
};
__device__ __forceinline__ int u_uniform(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ int64_t u_uniform(int64_t v) {
  return (int64_t)(((uint64_t)(uint32_t)u_uniform((int)((uint64_t)v >> 32)) << 32) | (uint32_t)u_uniform((int)(uint64_t)v));
}
__device__ __forceinline__ void u_chunk_load(const UArgs& p, int c, UCk& k) {
  if (p.chunks == nullptr) {
    k.step0 = p.state[ST_STEP]; k.n_updates = p.n_updates; k.n_total = p.n_total; k.eval_every = p.eval_every;
    k.do_eval = p.do_eval; k.ubase = 0u; k.evbase = 0u;
    k.seed = st_rng(p.state)[0];
    k.rng_ctr0 = st_rng(p.state)[1];
    return;
  }
  const bsig_fit_chunk& e = p.chunks[c];
  k.step0 = 0; k.n_updates = u_uniform(e.n_updates); k.n_total = k.n_updates; k.eval_every = u_uniform(e.eval_every);
  k.do_eval = 1; k.ubase = (unsigned)u_uniform(e.upd_base); k.evbase = (unsigned)u_uniform(e.eval_base);
  k.seed = (uint64_t)u_uniform((int64_t)e.seed); k.rng_ctr0 = (uint64_t)u_uniform((int64_t)e.rng_ctr0);
}

// One held-out evaluation: evaluation e (chunk-local) of chunk c.  Built where it is used (the evaluation
// whose parts run in the waits of the NEXT chunk's first updates still belongs to its own chunk).
struct UEval {
  int n_test, passes; int64_t row0;  // held-out feature rows feats[row0 .. row0 + n_test)
  const float* y_test; int64_t ldy_test;
  float* out;                        // its slot of the test-loss log (null: test_loss[state[ST_EVAL]], one chunk)
  unsigned gidx;                     // evaluation number of the launch: slab buffer gidx % 3, tag gidx + 1
  uint64_t seed, stream;             // jitter stream (one per update and per evaluation, in program order:
                                     // the per-phase path's numbering)
};
__device__ __forceinline__ UEval u_eval_of(const UArgs& p, int c, int e) {
  UEval v;
  int every, n_total, step0;
  uint64_t ctr0;
  if (p.chunks == nullptr) {
    v.n_test = p.n_test; v.row0 = p.eval_row0; v.y_test = p.y_test; v.ldy_test = p.ldy_test; v.out = nullptr;
    v.gidx = (unsigned)e; every = p.eval_every; n_total = p.n_total; step0 = p.state_in[ST_STEP];
    v.seed = st_rng(p.state_in)[0];
    ctr0 = st_rng(p.state_in)[1];
  } else {
    const bsig_fit_chunk& k = p.chunks[c];
    v.n_test = u_uniform(k.n_test); v.row0 = u_uniform(k.row0) + u_uniform(k.n_train);
    v.y_test = p.y + v.row0 * p.ldy; v.ldy_test = p.ldy; v.out = p.test_loss + u_uniform(k.test_slot) + e;
    v.gidx = (unsigned)u_uniform(k.eval_base) + (unsigned)e; every = u_uniform(k.eval_every);
    n_total = u_uniform(k.n_updates); step0 = 0;
    v.seed = (uint64_t)u_uniform((int64_t)k.seed); ctr0 = (uint64_t)u_uniform((int64_t)k.rng_ctr0);
  }
  v.passes = (v.n_test + p.B - 1) / p.B;
  const int at = eval_at_step(e, every, n_total);
  const int ev0 = p.do_eval || p.chunks ? evals_before(step0, every) : 0;
  v.stream = launch_stream(ctr0, at - step0, e, ev0);
  return v;
}

__device__ __forceinline__ f32x4 umfma(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// A row owner's sum over the k-slices: out[r * out_pitch + col] = sum_z slabs[z * zs + rowoff(r) + col]
// for r < nrows, col < n_cols (float offsets; `slabs` workgroup-uniform), slices added in order, up
// to 16 loads in flight per lane -- buffer loads: one address register per lane, the slice offset
// is scalar.  `fn(col, v)` sees every sum.
template <typename RowOff, typename F>
__device__ __forceinline__ void u_rows_sum(const float* slabs, RowOff&& rowoff, int k_slices, int zs, int nrows,
                                           int n_cols, float* out, int out_pitch, int tid, F&& fn) {
  const __amdgpu_buffer_rsrc_t sr = xwg_buffer(slabs);
  for (int idx = tid; idx < nrows * n_cols; idx += kUT) {
    const int r = idx / n_cols, col = idx - r * n_cols;
    const int voff = (rowoff(r) + col) * 4;
    float v = 0.f;
    for (int z = 0; z < k_slices; z += 16) {
      float q[16];
#pragma unroll
      for (int u = 0; u < 16; ++u)
        q[u] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(sr, voff, min(z + u, k_slices - 1) * zs * 4, kXwgPolicy));
#pragma unroll
      for (int u = 0; u < 16; ++u)
        if (z + u < k_slices) v += q[u];
    }
    out[r * out_pitch + col] = v;
    fn(col, v);
  }
}

// ---- held-out evaluation ev, its parts.  The in-launch path (u_tile_eval, u_owner_eval) strings them together
//      with flags and granules, the deferred path (fit_deferred_eval.hip) with kernel boundaries.
// The buffer of partial products of ONE evaluation: [passes][k_slices][B][NhP] floats.

// Products: held-out rows x this tile's weights (Wl, biasl: LDS; the B operand straight from memory, six
// 16-column steps at a time) -> the evaluation's slab buffer `ebase`.  Every thread of the workgroup.
template <int NT>
__device__ __forceinline__ void u_eval_products(const UArgs& p, const float* Wl, const float* biasl, int ks, int n0,
                                                int k0, const UEval& ev, float* ebase) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));    // (nothing below may be computed ahead of the update loop and kept live in it)
  const int lane = tid & 63, w = tid >> 6, c16 = lane & 15, g4 = lane >> 4;
  const int B = p.B, NhP = p.NhP;
  for (int pass = 0; pass < ev.passes; ++pass) {
    const int rows = min(B, ev.n_test - pass * B);
    if (rows <= 0) break;
    if (w < p.MT) {
      f32x4 acc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        acc[nt] = ks == 0 ? *reinterpret_cast<const f32x4*>(biasl + 16 * nt + 4 * g4) : zero;
      }
      const int64_t r = ev.row0 + pass * B + min(16 * w + c16, rows - 1);
      const float* src = p.feats + r * p.ld_feats;
      const float* ap = Wl + c16 * p.WP + 4 * g4;
#pragma unroll 1
      for (int s0 = 0; s0 < p.ksteps; s0 += kUGroup) {
        f32x4 breg[kUGroup];
#pragma unroll
        for (int q = 0; q < kUGroup; ++q) {
          const int col = k0 + 16 * (s0 + q) + 4 * g4;
          const f32x4 v = *reinterpret_cast<const f32x4*>(src + min((int64_t)col, p.ld_feats - 4));
          const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
          breg[q] = col < p.Fdim ? v : zero;
        }
#pragma unroll
        for (int q = 0; q < kUGroup; ++q) {
#pragma unroll
          for (int nt = 0; nt < NT; ++nt) {
            const f32x4 a4 = *reinterpret_cast<const f32x4*>(ap + nt * 16 * p.WP + 16 * (s0 + q));
            acc[nt] = umfma(a4[0], breg[q][0], acc[nt]);
            acc[nt] = umfma(a4[1], breg[q][1], acc[nt]);
            acc[nt] = umfma(a4[2], breg[q][2], acc[nt]);
            acc[nt] = umfma(a4[3], breg[q][3], acc[nt]);
          }
        }
      }
      if (16 * w + c16 < rows) {
        const __amdgpu_buffer_rsrc_t sr = xwg_buffer(ebase + (((int64_t)pass * p.k_slices + ks) * B) * NhP + n0);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          xwg_store4(sr, (16 * w + c16) * NhP + 16 * nt + 4 * g4, acc[nt][0], acc[nt][1], acc[nt][2], acc[nt][3]);
      }
    }
  }
}

// Rows, first part, by evaluation owner `eo` (held-out rows eo, eo + NE, ...: RE of them at the most): the
// k-slice sums of its rows -> XS; returns (thread 0) the owner's sum of exp over the sigma columns.  Every
// thread of the workgroup; ends behind a barrier (XS and the sum are complete).
__device__ __forceinline__ float u_eval_rows(const UArgs& p, const float* ebase, float* XS, float* red, int eo,
                                             const UEval& ev, int tid) {
  const int lane = tid & 63, w = tid >> 6;
  const int B = p.B, Nh = p.Nh, NhP = p.NhP, K = p.K, DK = p.D * p.K;
  const int per_wave = Nh + p.D + 3 * K;
  const int nr = eo < ev.n_test ? min(p.RE, (ev.n_test - eo + p.NE - 1) / p.NE) : 0;   // this owner's rows
  float eacc = 0.f;
  u_rows_sum(ebase,
             [&](int r) {
               const int erow = eo + p.NE * r, pass = erow / B, rb = erow - pass * B;
               return (pass * p.k_slices * B + rb) * NhP;
             },
             p.k_slices, B * NhP, nr, Nh, XS, per_wave, tid,
             [&](int col, float v) { if (col >= K + DK && col < K + 2 * DK) eacc += expf(v); });
  eacc = wave_sum_dpp(eacc);
  if (lane == 0) red[w] = eacc;
  __syncthreads();
  float sx = 0.f;
  if (tid == 0)
    for (int q = 0; q < kUT / 64; ++q) sx += red[q];
  return sx;
}

// Rows, second part: the NLL of the owner's rows (one wavefront each, forward only) from their sums in XS.
// `sum_exp()`: the sum over ALL owners of what u_eval_rows returned, in slot order (granule_slot_sum); called
// by whole wavefronts, only where the head has a jitter scale.  Returns (thread 0) the owner's sum of the rows'
// log-likelihoods; `bad`: a row was not finite (per lane).  Every thread of the workgroup; ends behind a barrier.
template <typename SumExp>
__device__ __forceinline__ float u_eval_nll(const UArgs& p, float* XS, float* red, int eo, const UEval& ev,
                                            const HeadArgs& a, int tid, SumExp&& sum_exp, bool& bad) {
  const int lane = tid & 63, w = tid >> 6;
  const int Nh = p.Nh, D = p.D, K = p.K, DK = D * K;
  const int per_wave = Nh + D + 3 * K;
  const int nr = eo < ev.n_test ? min(p.RE, (ev.n_test - eo + p.NE - 1) / p.NE) : 0;
  const int erow = eo + p.NE * w;
  const bool act = w < nr;
  float* tile = XS + w * per_wave;
  float* yv = tile + Nh;
  float* rk = yv + D;
  float* lpk = rk + K;
  float* dlg = lpk + K;
  if (act)
    for (int j = lane; j < D; j += 64) yv[j] = ev.y_test[(int64_t)erow * ev.ldy_test + j];
  RowOut ro;
  ro.lse = 0.f; ro.uds = 0.f; ro.bad = false;
#pragma unroll
  for (int q = 0; q < kElemsPerLane; ++q) ro.esg0[q] = 0.f;
  if (w < p.RE) {
    HeadArgs ae = a;
    ae.d_out = nullptr;                    // forward only
    ae.batch = ev.n_test;
    ae.seed = ev.seed;
    ae.stream_id = ev.stream;
    diag_row(ae, erow, act, lane, tile, yv, rk, lpk, dlg,
             [&] {
               return p.eps_noise != 0.f ? p.eps_noise * (sum_exp() / ((float)ev.n_test * (float)DK)) : 0.f;
             },
             ro);
  }
  if (lane == 0) red[16 + w] = act ? ro.lse : 0.f;
  __syncthreads();
  float sl = 0.f;
  if (tid == 0)
    for (int q = 0; q < kUT / 64; ++q) sl += red[16 + q];
  bad = ro.bad;
  return sl;
}

// The log entry (one lane): `sum` is the sum over all owners of what u_eval_nll returned, in slot order
__device__ __forceinline__ void u_eval_log(const UArgs& p, const UEval& ev, float sum, int32_t* flagp) {
  const float l = -sum / (float)ev.n_test;
  if (ev.out) *ev.out = l;
  else p.test_loss[p.state[ST_EVAL]] = l;
  p.state[ST_EVAL] = p.state[ST_EVAL] + 1;
  if (!isfinite(l)) atomicOr(flagp, kFlagNonfinite);
}

// The head arguments of the rows of this launch (what does not change from row to row)
__device__ __forceinline__ HeadArgs u_head_args(const UArgs& p) {
  HeadArgs a{};
  a.D = p.D; a.K = p.K; a.Nh = p.Nh; a.batch = p.B; a.from_tuple = 0;
  a.min_w = p.min_w; a.ll_limit = p.ll_limit; a.inv_norm = p.inv_norm;
  a.eps_noise = p.eps_noise; a.d_out = p.d_out;
  return a;
}

// ---- in-launch: tile part of held-out evaluation ev -> evaluation slab buffer gidx % 3, flag
template <int NT>
__device__ __forceinline__ void u_tile_eval(const UArgs& p, const float* Wl, const float* biasl, int slot,
                                            int ks, int n0, int k0, const UEval& ev) {
  u_eval_products<NT>(p, Wl, biasl, ks, n0, k0, ev,
                      p.eval_slabs + (int64_t)(ev.gidx % 3u) * p.eval_passes * p.k_slices * p.B * p.NhP);
  __builtin_amdgcn_s_waitcnt(0);
  __syncthreads();
  if (threadIdx.x == 0) flag_raise(p.flag_eval, slot, ev.gidx + 1u);
}

// ---- in-launch: row part of held-out evaluation ev by evaluation owner `eo`
__device__ __forceinline__ void u_owner_eval(const UArgs& p, float* XS, float* red, int eo, const UEval& ev,
                                             const HeadArgs& a) {
  int tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63, w = tid >> 6;
  int32_t* flagp = p.state + ST_FLAGS;
  const unsigned etag = ev.gidx + 1u;
  if (w == 0) flags_wait(p.flag_eval, p.G, etag, lane, flagp);
  __syncthreads();
  const float* ebase = p.eval_slabs + (int64_t)(ev.gidx % 3u) * p.eval_passes * p.k_slices * p.B * p.NhP;
  const float sx = u_eval_rows(p, ebase, XS, red, eo, ev, tid);
  if (tid == 0) granule_publish(p.gran_eval, eo, etag, sx);
  bool bad;
  const float sl = u_eval_nll(p, XS, red, eo, ev, a, tid,
                              [&] { return granule_gather(p.gran_eval, p.NE, etag, lane, flagp); }, bad);
  if (tid == 0) granule_publish(p.gran_eval + kGranArr, eo, etag, sl);
  if (eo == 0 && w == 0) {
    const float sum = granule_gather(p.gran_eval + kGranArr, p.NE, etag, lane, flagp);
    if (lane == 0) u_eval_log(p, ev, sum, flagp);
  }
  if (bad) atomicOr(flagp, kFlagNonfinite);
  __syncthreads();
}

}  // namespace bsig
