/*
 * bsig_f64.h — the fp64 mode of libbsig_hip.so: a second, self-contained PER-PHASE update path
 * (GEMMs on v_mfma_f64_16x16x4_f64, mixture-density head, Adam, fit loop) behind MDNN.double() /
 * MDRFF.double(), and the trajectory summarizers in double (summarizers' dtype=torch.float64).  Companion of bsig.h, whose rules hold here too: raw DEVICE pointers (to fp64 /
 * int32 unless stated), leading dimensions in elements, every call asynchronous on `stream`, no
 * allocation, no synchronisation, BSIG_OK or a negative code, the thread-local message of bsig.h.
 *
 * There are no persistent kernels, HIP graphs, factor rows, block launches or data-parallel
 * exchange in fp64: an update is a sequence of plain launches.
 *
 * The arithmetic of the fp64 mode: EVERY value is a double, the per-component log-probabilities
 * included -- the reference under torch.set_default_dtype(torch.float64).  The reference's
 * `result = torch.zeros(b, K)` (mdnn.py:149) is fp32 whenever the default dtype is fp32, even on a
 * .double() model; that quirk is NOT reproduced here.
 *
 * bsig_mdn_cfg / bsig_head_dims are reused unchanged; the flat parameter layout is that of
 * bsig_mdn_param_offsets, in doubles.  Their float hyper-parameters (1e-3f is not 1e-3) are
 * overridden by a bsig_f64_hyper where one is given.
 */
#ifndef BSIG_F64_H
#define BSIG_F64_H

#include "bsig.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The hyper-parameters as the doubles the reference computes with in fp64 mode (Python floats:
 * mdnn.py:22-24, torch.optim.Adam defaults mdnn.py:203, rff.py:107).  NULL wherever one is taken
 * = the floats of the cfg / dims, widened. */
typedef struct bsig_f64_hyper {
  double lr, beta1, beta2, adam_eps;
  double eps_noise, min_weight, ll_limit;
  double rff_scale;
} bsig_f64_hyper;

/* ------------------------------------------------------------------ */
/* Trajectory summarizers in double: the fp32 entry points of bsig.h    */
/* with double pointers -- same argument lists, same row layouts, same  */
/* widths (the shared width function of bsig.h), ld_out in doubles.     */
/* states [N,T,sd], actions [N,Ta,ad] contiguous doubles in, [N,ld_out] */
/* double rows out: what the reference's torch ops give on double       */
/* trajectories.  One workgroup per trajectory, at most                 */
/* BSIG_F64_SUMMARY_GRID_CAP workgroups (they stride over the rest).    */
/* ------------------------------------------------------------------ */
#define BSIG_F64_SUMMARY_GRID_CAP 4096

/* summary_start / summary_waypts, summarizers.py:65-87 after the crop / pad of :20-62 (a copy). */
int bsig_summary_start_f64(const double* states, const double* actions, double* out, int64_t n,
                           int t_states, int t_actions, int sd, int ad, int max_t, int64_t ld_out,
                           bsig_stream_t stream);

/* cross_correlation, summarizers.py:90-122: out[i*A + j] = sf[i] * af[j] -- ONE double multiply
 * per element, the state features one subtraction (use_state_diff) or a copy -- then mean and
 * unbiased std of the state features, two passes (:114-119), std = 0 for fewer than two features.
 * `nonfinite` (int32, may be NULL) is OR-ed with 1 where the reference asserts isfinite (:120).
 * BSIG_EUNSUPPORTED when the features of a row exceed a workgroup's LDS. */
int bsig_crosscorr_f64(const double* states, const double* actions, double* out, int64_t n,
                       int t_states, int t_actions, int sd, int ad, int use_state_diff,
                       int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream);

/* summary_signatory, summarizers.py:144-168: the signature of [t | s | a], levels 1..depth
 * (depth <= 0: the reference's choice, :133-141) by Chen's identity in double.  Depth 3 covers
 * every path dimension the reference takes at depth 3 (d = 1 + sd + ad <= 22); a wider forced
 * depth 3, or a path whose points, increments and d^3 level-3 terms exceed a workgroup's 160 KB
 * of LDS, is BSIG_EUNSUPPORTED. */
int bsig_signature_f64(const double* states, const double* actions, double* out, int64_t n,
                       int length, int sd, int ad, int depth, int64_t ld_out, bsig_stream_t stream);

/* ------------------------------------------------------------------ */
/* fp64 MFMA GEMM with the epilogues of the fp32 GEMM of bsig.h: same  */
/* operand forms (k-contiguous / k-major, optional int32 row gather),  */
/* same BSIG_EPI_* / BSIG_ACT_* codes, evaluated in double.  K is not  */
/* split: every output is ONE ascending-k accumulation chain, so two   */
/* runs are bitwise equal.  Replaces nn.Linear / autograd matmuls of   */
/* mdnn.py:108-119,233 on a .double() model.                           */
/* ------------------------------------------------------------------ */
int bsig_gemm_f64(const double* a, int64_t lda, int a_kmajor, const int32_t* a_rows,
                  const double* b, int64_t ldb, int b_kmajor, const int32_t* b_rows,
                  double* c, int64_t ldc, int64_t m, int64_t n, int64_t k,
                  int epilogue, int act, const double* bias, const double* aux,
                  int64_t ldaux, double alpha, bsig_stream_t stream);

/* RFF projection in double, rff.py:128-132 / :122-126: feats = a*[cos|sin](x coeff^T), coeff
 * [m_feat, in_dim] = freqs / sigma (the caller's: freqs.double() / sigma.double()).  x_rows gathers
 * rows (may be NULL); cos_only uses offset[m_feat]. */
int bsig_rff_project_f64(const double* x, int64_t ldx, const int32_t* x_rows,
                         const double* coeff, int64_t ld_coeff, const double* offset,
                         double* feats, int64_t ld_feats, int64_t batch, int64_t in_dim,
                         int64_t m_feat, double a, int cos_only, bsig_stream_t stream);

/* ------------------------------------------------------------------ */
/* Mixture-density head in double (mdnn.py:108-178; closed forms of    */
/* SURVEY.md Appendix A.1-A.3).  head_out as in bsig.h.  One wavefront  */
/* per row; n_comp <= 64; out_dim bounded by the workgroup's LDS.      */
/* Jitter: the Philox uniform of element (b*D + d)*K + k, word 0, the  */
/* 24-bit draw of the fp32 thread-per-component kernels widened to     */
/* double; an injected `noise` [B,D,K] takes precedence.  `nonfinite`  */
/* (int32) is OR-ed with 1 where the reference asserts isfinite.       */
/* ------------------------------------------------------------------ */
size_t bsig_head_workspace_bytes_f64(const bsig_head_dims* dims, int64_t batch);

/* forward() tuple from raw head outputs, mdnn.py:109-119. */
int bsig_mdn_head_outputs_f64(const bsig_head_dims* dims, const bsig_f64_hyper* hyper,
                              const double* head_out, int64_t ld, int64_t batch,
                              const double* noise, uint64_t seed, uint64_t stream_id,
                              double* weights, double* mu, double* l_d, double* lower,
                              int32_t* nonfinite, void* workspace, size_t workspace_bytes,
                              bsig_stream_t stream);

/* mdn_loss_fn(weights, mu, L_d, L, y), mdnn.py:127-178 -> loss[0]. */
int bsig_mdn_nll_from_tuple_f64(const bsig_head_dims* dims, const bsig_f64_hyper* hyper,
                                const double* weights, const double* mu, const double* l_d,
                                const double* lower, const double* y, int64_t ldy, int64_t batch,
                                double* loss, int32_t* nonfinite, void* workspace,
                                size_t workspace_bytes, bsig_stream_t stream);

/* Fused forward()+mdn_loss_fn (+ backward when d_head_out != NULL), mdnn.py:109-178 and the
 * autograd pass of mdnn.py:233 through them: loss[0] = mean NLL over `batch` rows, d_head_out
 * [B, ld] = d(sum_b nll_b / norm_batch) / d head_out, clamp masks and the non-detached
 * jitter-mean term included. */
int bsig_mdn_head_nll_f64(const bsig_head_dims* dims, const bsig_f64_hyper* hyper,
                          const double* head_out, int64_t ld, const double* y, int64_t ldy,
                          const int32_t* y_rows, int64_t batch, int64_t norm_batch,
                          const double* noise, uint64_t seed, uint64_t stream_id, double* loss,
                          double* d_head_out, int32_t* nonfinite, void* workspace,
                          size_t workspace_bytes, bsig_stream_t stream);

/* ------------------------------------------------------------------ */
/* Flat-buffer helpers in double                                       */
/* ------------------------------------------------------------------ */
/* torch.optim.Adam step (mdnn.py:203,234), t = 1-based step number; beta^t as running products. */
int bsig_adam_flat_f64(double* params, const double* grads, double* exp_avg, double* exp_avg_sq,
                       int64_t n, double lr, double beta1, double beta2, double eps, int64_t t,
                       bsig_stream_t stream);
/* normalize_samples, mdnn.py:245-248: out = (theta - lows) / (highs - lows). */
int bsig_normalize_rows_f64(const double* theta, int64_t ld_in, const double* lows,
                            const double* highs, double* out, int64_t ld_out, int64_t rows,
                            int64_t cols, bsig_stream_t stream);
/* dst[i, :cols] = src[rows ? rows[i] : i, :cols]  (mdnn.py:206-211,222: split / minibatch gather). */
int bsig_copy_rows_f64(const double* src, int64_t ld_src, const int32_t* rows, double* dst,
                       int64_t ld_dst, int64_t n_rows, int64_t cols, bsig_stream_t stream);

/* ------------------------------------------------------------------ */
/* Estimator in double                                                 */
/* ------------------------------------------------------------------ */
size_t bsig_mdn_workspace_bytes_f64(const bsig_mdn_cfg* cfg, int64_t max_batch);

/* head_out[B, Nh] = heads(trunk(x)) (or heads(rff(x))): mdnn.py:108-119 without the softmax/exp. */
int bsig_mdn_head_forward_f64(const bsig_mdn_cfg* cfg, const bsig_f64_hyper* hyper,
                              const double* params, const double* rff_coeff, int64_t ld_coeff,
                              const double* rff_offset, const double* x, int64_t ldx,
                              const int32_t* x_rows, int64_t batch, double* head_out,
                              int64_t ld_head, void* workspace, size_t workspace_bytes,
                              bsig_stream_t stream);

/* One forward + NLL + backward over a minibatch, mdnn.py:229-233: flat `grads` (layout of params;
 * every parameter's slot overwritten) and loss[0]. */
int bsig_mdn_loss_grad_f64(const bsig_mdn_cfg* cfg, const bsig_f64_hyper* hyper,
                           const double* params, const double* rff_coeff, int64_t ld_coeff,
                           const double* rff_offset, const double* x, int64_t ldx,
                           const double* y, int64_t ldy, const int32_t* rows, int64_t batch,
                           int64_t norm_batch, const double* noise, uint64_t seed,
                           uint64_t stream_id, double* grads, double* loss, int32_t* nonfinite,
                           void* workspace, size_t workspace_bytes, bsig_stream_t stream);

/* Fit loop: MDNN.run_training's loop (mdnn.py:203-242) for one chunk, the protocol of bsig_fit_*
 * (bsig.h) as plain launches: create -> bind -> begin (fresh optimizer, mdnn.py:203; an MDRFF's
 * rows are projected here, once per call) -> run (n_updates updates over the [n_updates, batch] id
 * table, held-out evaluations at the logging points of mdnn.py:235-242) -> pack_logs (the call's
 * ONE read-back).  Step number, beta powers, step sizes, losses and the non-finite flag live on
 * the device. */
typedef struct bsig_fit64_buffers {
  double* params; double* grads; double* exp_avg; double* exp_avg_sq; /* [P] */
  const double* rff_coeff; int64_t ld_coeff; const double* rff_offset;
  const double* x_train; int64_t ldx_train; int64_t n_train;
  const double* y_train; int64_t ldy_train;          /* normalised theta */
  const double* x_test; int64_t ldx_test; int64_t n_test;
  const double* y_test; int64_t ldy_test;
  const int32_t* ids_table;      /* [n_updates, batch] */
  double* train_loss;            /* [n_updates] */
  double* test_loss;             /* [n_evals]   */
  int32_t* state;                /* [32] int32 engine state (reset by begin; csrc/fit_protocol.h); word 2 = flag word */
  void* workspace; size_t workspace_bytes;
  int32_t x_kind;                /* BSIG_X_ROWS; factor rows: BSIG_EUNSUPPORTED */
} bsig_fit64_buffers;

typedef struct bsig_fit64_plan bsig_fit64_plan;

int bsig_fit64_create(const bsig_mdn_cfg* cfg, const bsig_f64_hyper* hyper, int64_t batch,
                      int64_t max_train_rows, int64_t max_test_rows, int64_t n_updates,
                      bsig_fit64_plan** plan);
void bsig_fit64_destroy(bsig_fit64_plan* plan);
size_t bsig_fit64_workspace_bytes(const bsig_fit64_plan* plan);
/* flags as bsig_fit_bind: BSIG_FIT_GRAPH is ignored (there is no graph), BSIG_FIT_SPLIT_ADAM (a
 * data-parallel plan) is BSIG_EUNSUPPORTED. */
int bsig_fit64_bind(bsig_fit64_plan* plan, const bsig_fit64_buffers* buffers, int flags);
int bsig_fit64_begin(bsig_fit64_plan* plan, uint64_t seed, int64_t norm_batch, bsig_stream_t stream);
int bsig_fit64_run(bsig_fit64_plan* plan, int64_t n_updates, bsig_stream_t stream);
/* out[2*E + 1] doubles (device): train_loss at the E logging points | test_loss[E] | flag word.
 * n_evals = E as the caller counts the logging points of mdnn.py:235 (it sized `out` by it):
 * BSIG_EINVAL unless the fit loop ran the same number. */
int bsig_fit64_pack_logs(bsig_fit64_plan* plan, int64_t n_updates, int64_t n_evals, double* out,
                         bsig_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* BSIG_F64_H */
