// Persistent update kernel of the fit engine for the MDNN estimator with the
// reference's default trunk (two hidden layers of 128 tanh units, diagonal
// covariance; fit_persistent_mdnn.hip): a run of consecutive Adam updates
// (mdnn.py:219-233) in ONE launch.
#pragma once
#include "persist.h"

namespace bsig {

struct PersistMdnnShape {
  int batch, input_dim, h1, h2, activation, out_dim, n_comp, full_cov;
  int max_test = 0;   // held-out rows the plan may evaluate inside the launches (0: none)
};

// The decomposition fit_persistent_mdnn.hip plans for a shape (host only)
struct MdnnGeom {
  int FR, Nh, Nh16, NhP, k_slices, G1, n_owner, n_small, x_floats;
  int wide;                     // head outputs formed by the head-block workgroups (see MdnnArgs)
  int stream, s_chunks;         // W1 streamed by G1 tile workgroups (fit_persistent_mdnn_stream.hip)
  int mr;                       // minibatch rows per owner workgroup
  int eval_passes;              // 0: evaluations stay outside the launches
  size_t lds;
  size_t slab_floats, act_floats, dout_floats, eval_floats, eval_slab_floats;
  // streamed W1: the tile workgroups' layout of S x A factor rows, known at bind
  // (persist_mdnn_resolve_stream; s_S = 0: none yet)
  int s_S, s_A, s_dp, s_nip, s_pf;
  size_t s_lds;
};

struct PersistMdnnBuffers : PersistCommon {
  const float* x; int64_t ldx;            // summary rows (training split of the chunk), or
  int x_kind = 0, x_s = 0, x_a = 0;       // ... cross-correlation factor rows (bsig.h: the tile
                                          // workgroups form x[i*A + j] = sf[i] * af[j] themselves)
  int64_t w1_off, b1_off, w2_off, b2_off, wh_off, bh_off;
  // held-out rows of the in-launch evaluations: summary rows, or -- streamed first layer -- the
  // held-out pairs' factor rows
  const float* x_test = nullptr; int64_t ldx_test = 0;
  const float* x_test_fac = nullptr; int64_t ldx_test_fac = 0;
};

// The decomposition of a shape and whether the device can hold every workgroup of its launch at once
// (asks the device and raises the kernels' dynamic-LDS limit: once per plan).  With a streamed first
// layer (it does not fit the chip) such a plan takes cross-correlation factor rows only; the Adam step
// of a data-parallel rank runs outside the launches (flat kernel after the all-reduce); a single rank's
// held-out evaluations run INSIDE its one launch, from the held-out pairs' factor rows
// (bsig_fit_evaluates_from_factors).  false: not covered, *g and *e as they were.
bool persist_mdnn_resolve(const PersistMdnnShape& s, MdnnGeom* g, PersistEngine* e);
// S x A cross-correlation factor rows give the first layer's input_dim and -- streamed first layer --
// fit its tile workgroups (arithmetic only; bsig.h: x_kind)
bool persist_mdnn_factors_fit(const MdnnGeom& g, int input_dim, int S, int A);
// streamed first layer, at bind: the tile workgroups' layout for S x A factor rows, and whether the
// device can hold every workgroup of the launch (data-parallel or single-rank instantiation) at once
// (asks the device).  *g unchanged on failure.
int persist_mdnn_resolve_stream(MdnnGeom* g, int input_dim, bool full_cov, int S, int A, bool dp);
// (diagnostics) the decomposition fit_persistent_mdnn.hip plans for a shape, bsig.h: bsig_debug_persist_mdnn_geometry
int persist_mdnn_geometry(const PersistMdnnShape& s, int32_t* out);
int persist_mdnn_reset_regions(const MdnnGeom& g, void* workspace, size_t workspace_bytes, ZeroRegion* regions);
// n consecutive updates starting at the state block's step counter; advances the
// counter, the jitter RNG stream and the Adam bias-correction powers
int persist_mdnn_run(const PersistMdnnShape& s, const MdnnGeom& g, const PersistMdnnBuffers& b, int n,
                     hipStream_t st);
// fit_persistent_mdnn_stream.hip: can the device hold the streamed launch's `grid` workgroups of `lds`
// bytes at once (asks the device)?
int mdnn_stream_can_host(bool dp, bool wide, bool full, int grid, size_t lds);

}  // namespace bsig
