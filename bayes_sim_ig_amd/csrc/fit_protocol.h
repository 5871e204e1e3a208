// The chunk protocol of run_training, stated once for the native side (bayes_sim_ig_amd/protocol.py
// is the Python statement): the device state block that carries a call between launches, the flag
// word's bits, the logging schedule of mdnn.py:235, the numbering of the jitter streams, the Adam
// bias-correction advance, the advances of the block and the packing of a call's logs.  Every
// update engine -- per-phase fp32 and fp64, the three persistent kernels, block and data-parallel
// launches -- agrees on this to the bit, so each takes it from here.
//
// Header-only, host and device, nothing of the project included.  Everything is passed and returned
// BY VALUE and reads go through pointers to const: the persistent kernels are tuned to their register
// allocation, and this form compiles to the code the written-out arithmetic did (reference parameters
// and non-const accessors in the update loops did not).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define BSIG_PROTO __host__ __device__ inline __attribute__((always_inline))
#else
#define BSIG_PROTO inline
#endif

namespace bsig {

// ---- state block (int32 words) ----------------------------------------------------------------
// Words shared by the fp32 and the fp64 engine: updates done, evaluations done (= next slot of the
// test-loss log), flag word.
enum { ST_STEP = 0, ST_EVAL = 1, ST_FLAGS = 2 };
// fp32 engines, 16 words: lr / (1 - beta1^t) and 1 / sqrt(1 - beta2^t) as floats (what the Adam
// kernels read), the jitter RNG pair {seed, next stream} (uint64 x2), {beta1^t, beta2^t} (double x2).
enum { ST_ADAM0 = 4, ST_ADAM1 = 5, ST_RNG = 8, ST_BETA_POW = 12, ST_WORDS = 16 };
// fp64 engine, 32 words: doubles from word 8: beta1^t, beta2^t, lr / (1 - beta1^t), sqrt(1 - beta2^t)
// (its stream counter lives on the host).
enum { ST64_DBL = 8, ST64_WORDS = 32 };

// flag word: a loss or a gradient was not finite / a bounded poll of a persistent kernel gave up
constexpr int32_t kFlagNonfinite = 1, kFlagTimeout = 2;

BSIG_PROTO const float* st_adam(const int32_t* st) { return reinterpret_cast<const float*>(st) + ST_ADAM0; }
BSIG_PROTO const uint64_t* st_rng(const int32_t* st) { return reinterpret_cast<const uint64_t*>(st + ST_RNG); }
BSIG_PROTO const double* st_beta_pow(const int32_t* st) { return reinterpret_cast<const double*>(st + ST_BETA_POW); }
BSIG_PROTO const double* st64_dbl(const int32_t* st) { return reinterpret_cast<const double*>(st + ST64_DBL); }

// The block of a fresh optimizer (mdnn.py:203), after its words were zeroed: streams count from 1.
BSIG_PROTO void st_begin(int32_t* st, uint64_t seed) {
  reinterpret_cast<uint64_t*>(st + ST_RNG)[0] = seed;
  reinterpret_cast<uint64_t*>(st + ST_RNG)[1] = 1;
  reinterpret_cast<double*>(st + ST_BETA_POW)[0] = 1.0;   // beta1^0, beta2^0
  reinterpret_cast<double*>(st + ST_BETA_POW)[1] = 1.0;
}
BSIG_PROTO void st64_begin(int32_t* st) {
  reinterpret_cast<double*>(st + ST64_DBL)[0] = 1.0;
  reinterpret_cast<double*>(st + ST64_DBL)[1] = 1.0;
}

// ---- logging schedule (mdnn.py:235) -----------------------------------------------------------
// The held-out loss is logged after update `it` (0-based) when it % every == 0, and after the last.
template <typename I> BSIG_PROTO I eval_every(I n_updates) { return n_updates / 5 > 1 ? n_updates / 5 : 1; }
template <typename I> BSIG_PROTO bool is_logging_point(I it, I n_updates, I every) {
  return it % every == 0 || it + 1 == n_updates;
}
// evaluations that precede update `step` (those after the updates it < step with it % every == 0)
BSIG_PROTO int evals_before(int step, int every) { return step == 0 ? 0 : (step - 1) / every + 1; }
// is update `step` preceded by the evaluation of update step - 1?
BSIG_PROTO bool eval_follows_update(int step, int every) { return step > 0 && (step - 1) % every == 0; }
// index of the evaluation after the last update of a call of n_total updates (for n_total >= 1 this
// is evals_before(n_total - 1, every): the last update's own evaluation, scheduled or not)
BSIG_PROTO int last_eval_index(int n_total, int every) { return n_total <= 1 ? 0 : (n_total - 2) / every + 1; }
// evaluations of the n updates from step0 of a call of n_total; with_final: the one after the last
// update counts where the schedule does not hold it already (a data-parallel launch leaves it out)
BSIG_PROTO int evals_in_run(int step0, int n, int n_total, int every, bool with_final) {
  int n_ev = evals_before(step0 + n, every) - evals_before(step0, every);
  if (with_final && step0 + n == n_total && (n_total - 1) % every != 0) ++n_ev;
  return n_ev;
}
// (in the caller's integer type, as eval_every: the multiples of `every` below n_updates, and the last update
// where it is none -- evals_in_run(0, n, n, every, true))
template <typename I> BSIG_PROTO I count_logging_points(I n_updates) {
  const I every = eval_every(n_updates);
  return n_updates <= 0 ? 0 : (n_updates - 1) / every + 1 + ((n_updates - 1) % every != 0 ? 1 : 0);
}

// ---- jitter streams ---------------------------------------------------------------------------
// One stream per update and per evaluation, in program order, from the block's `next stream` at the
// start of the launch (ctr0): what runs with `updates_done` updates of the launch behind it, and the
// call's evaluations before `evals_done` (ev0 of them before the launch: evals_before(step0, every), 0
// in a launch whose evaluations run outside it), takes this stream.  Update t of the launch at chunk
// step `step`: (t, evals_before(step, every)); evaluation e of the call: (eval_at_step(e) - step0, e).
BSIG_PROTO uint64_t launch_stream(uint64_t ctr0, int updates_done, int evals_done, int ev0) {
  return ctr0 + (uint64_t)updates_done + (uint64_t)(evals_done - ev0);
}
// the update that evaluation e precedes: e * every + 1, the call's count for the one after the last
BSIG_PROTO int eval_at_step(int e, int every, int n_total) {
  return e * every + 1 < n_total ? e * every + 1 : n_total;
}

// ---- Adam bias correction ---------------------------------------------------------------------
// beta^t as running products in double (no pow() on the device); a0 = lr / (1 - beta1^t) and
// a1 = 1 / sqrt(1 - beta2^t) rounded to float once, here, for every engine.
struct AdamAdvance { double b1t, b2t; float a0, a1; };
BSIG_PROTO AdamAdvance adam_advance(double b1t, double b2t, double beta1, double beta2, double lr) {
  AdamAdvance r;
  r.b1t = b1t * beta1; r.b2t = b2t * beta2;
  r.a0 = (float)(lr / (1.0 - r.b1t));
  r.a1 = (float)(1.0 / sqrt(1.0 - r.b2t));
  return r;
}
// ---- single-writer advances of the block ------------------------------------------------------
// Per-phase engines, the head's finishing hook: the end of the forward half of an update (`update`),
// or of a held-out evaluation.  Either takes the next jitter stream.
BSIG_PROTO void st_finish_hook(int32_t* st, bool update, double beta1, double beta2, double lr) {
  if (update) {
    const double* bp = st_beta_pow(st);
    const AdamAdvance a = adam_advance(bp[0], bp[1], beta1, beta2, lr);
    reinterpret_cast<double*>(st + ST_BETA_POW)[0] = a.b1t;
    reinterpret_cast<double*>(st + ST_BETA_POW)[1] = a.b2t;
    reinterpret_cast<float*>(st)[ST_ADAM0] = a.a0;
    reinterpret_cast<float*>(st)[ST_ADAM1] = a.a1;
    st[ST_STEP] = st[ST_STEP] + 1;
  } else {
    st[ST_EVAL] = st[ST_EVAL] + 1;
  }
  reinterpret_cast<uint64_t*>(st + ST_RNG)[1] += 1;
}
// the fp64 engine keeps the step size and sqrt(1 - beta2^t) (torch's bias_correction2_sqrt) in double
BSIG_PROTO void st64_finish_hook(int32_t* st, bool update, double beta1, double beta2, double lr) {
  if (update) {
    double* dv = reinterpret_cast<double*>(st + ST64_DBL);
    const double b1t = dv[0] * beta1, b2t = dv[1] * beta2;
    dv[0] = b1t; dv[1] = b2t;
    dv[2] = lr / (1.0 - b1t);
    dv[3] = sqrt(1.0 - b2t);
    st[ST_STEP] += 1;
  } else {
    st[ST_EVAL] += 1;
  }
}

// Persistent engines, end of a launch of n updates from step0 (thread 0 of one workgroup, written out at
// the end of each kernel's tile workgroup: a call here changed the kernels' register allocation):
//   the powers and the two Adam floats as st_finish_hook stores them;
//   next stream += n + n_ev, n_ev = evals_in_run(step0, n, n_total, every, with_final) where the launch's
//   evaluations ran inside it (with_final: not in a data-parallel rank's launch), else 0;
//   step = step0 + n.
// A block of chunks leaves what the call of its last chunk would have left: that chunk's seed, and its
// first stream advanced.  The evaluation counter is advanced by the evaluations' owners as they log.

// ---- a call's logs for its single read-back ---------------------------------------------------
// out = [train_loss at the logging points | test_loss | flag word], 2 * n_evals + 1 values; thread
// `tid` of `n_threads` of one workgroup.
template <typename T>
BSIG_PROTO void pack_call_logs(const T* train_loss, const T* test_loss, const int32_t* state, int n_updates,
                               int every, int n_evals, T* out, int tid, int n_threads) {
  if (tid == 0) {
    int e = 0;
    for (int it = 0; it < n_updates; ++it)
      if (is_logging_point(it, n_updates, every)) { out[e] = train_loss[it]; ++e; }
    out[2 * n_evals] = (T)state[ST_FLAGS];
  }
  for (int i = tid; i < n_evals; i += n_threads) out[n_evals + i] = test_loss[i];
}

}  // namespace bsig
