// include/bsig_input_norm.h in fp32: the workspace size (host arithmetic), bsig_input_norm_stats and
// bsig_input_norm_apply.  The kernels and the argument checks are csrc/input_norm.h.
#include "input_norm.h"

using namespace bsig;

extern "C" int64_t bsig_input_norm_workspace_bytes(int64_t n, int64_t width) {
  return inorm::workspace_bytes(n, width);
}

// column means and reciprocal standard deviations of fp32 rows
extern "C" int bsig_input_norm_stats(const float* x, int64_t ld, int64_t n, int64_t width, double* mean,
                                     double* inv_std, void* workspace, size_t workspace_bytes,
                                     bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_input_norm_stats");
  return inorm::stats_run<float>("input_norm_stats", x, ld, n, width, mean, inv_std, workspace, workspace_bytes,
                                 as_stream(stream));
}

// out = (x - mean) * inv_std on fp32 rows
extern "C" int bsig_input_norm_apply(const float* x, int64_t ld_x, const double* mean, const double* inv_std,
                                     float* out, int64_t ld_out, int64_t n, int64_t width, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_input_norm_apply");
  return inorm::apply_run<float>("input_norm_apply", x, ld_x, mean, inv_std, out, ld_out, n, width,
                                 as_stream(stream));
}
