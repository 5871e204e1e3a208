// include/bsig_ragged.h in double, the cross-correlation: bsig_xcorr_ragged_f64, the fp64 twin of
// csrc/xcorr_ragged.hip on the same kernel template (csrc/xcorr.h).
#include "f64.h"
#include "../xcorr.h"

using namespace bsig;

extern "C" int bsig_xcorr_ragged_f64(const double* states, const double* actions, const int32_t* lengths,
                                     double* out, int64_t n, int ts, int ta, int sd, int ad, int max_lag,
                                     int state_diff, int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_xcorr_ragged_f64");
  return xcorr::run_any<double, true>("xcorr_ragged_f64", BSIG_F64_SUMMARY_GRID_CAP, states, actions, lengths, out,
                                      n, ts, ta, sd, ad, max_lag, state_diff, ld_out, nonfinite, stream);
}
