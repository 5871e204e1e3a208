// include/bsig_input_norm.h on double rows: bsig_input_norm_stats_f64 and bsig_input_norm_apply_f64, the twins of
// csrc/input_norm.hip on the same kernel templates (csrc/input_norm.h); u = 2^-52 in the flat rule.
#include "f64.h"
#include "../input_norm.h"

using namespace bsig;

// column means and reciprocal standard deviations of double rows
extern "C" int bsig_input_norm_stats_f64(const double* x, int64_t ld, int64_t n, int64_t width, double* mean,
                                         double* inv_std, void* workspace, size_t workspace_bytes,
                                         bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_input_norm_stats_f64");
  return inorm::stats_run<double>("input_norm_stats_f64", x, ld, n, width, mean, inv_std, workspace,
                                  workspace_bytes, as_stream(stream));
}

// out = (x - mean) * inv_std on double rows
extern "C" int bsig_input_norm_apply_f64(const double* x, int64_t ld_x, const double* mean, const double* inv_std,
                                         double* out, int64_t ld_out, int64_t n, int64_t width,
                                         bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_input_norm_apply_f64");
  return inorm::apply_run<double>("input_norm_apply_f64", x, ld_x, mean, inv_std, out, ld_out, n, width,
                                  as_stream(stream));
}
