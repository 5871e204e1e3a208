// Trajectory summarizers of the fp64 mode (include/bsig_f64.h): the double instantiation of csrc/summaries.h.
#include "f64.h"
#include "../summaries.h"

using namespace bsig::summaries;

extern "C" int bsig_summary_start_f64(const double* states, const double* actions, double* out,
                                      int64_t n, int t_states, int t_actions, int sd, int ad,
                                      int max_t, int64_t ld_out, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_summary_start_f64");
  return run_start<double>(states, actions, out, n, t_states, t_actions, sd, ad, max_t, ld_out, stream);
}

extern "C" int bsig_crosscorr_f64(const double* states, const double* actions, double* out, int64_t n,
                                  int t_states, int t_actions, int sd, int ad, int use_state_diff,
                                  int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_crosscorr_f64");
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(out, "crosscorr_f64: null pointer");
  return run_crosscorr<double>(states, actions, out, ld_out, nullptr, 0, n, t_states, t_actions, sd, ad,
                               use_state_diff, nonfinite, stream);
}

extern "C" int bsig_signature_f64(const double* states, const double* actions, double* out, int64_t n,
                                  int length, int sd, int ad, int depth, int64_t ld_out,
                                  bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_signature_f64");
  return run_signature<double>(states, actions, out, n, length, sd, ad, depth, ld_out, stream);
}
