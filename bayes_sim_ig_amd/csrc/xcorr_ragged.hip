// include/bsig_ragged.h in fp32, the cross-correlation: bsig_xcorr_ragged on the kernel template of csrc/xcorr.h
// with every trajectory's own length.
#include "xcorr.h"

using namespace bsig;

extern "C" int bsig_xcorr_ragged(const float* states, const float* actions, const int32_t* lengths, float* out,
                                 int64_t n, int ts, int ta, int sd, int ad, int max_lag, int state_diff,
                                 int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_xcorr_ragged");
  return xcorr::run_any<float, true>("xcorr_ragged", kSummaryGridCap, states, actions, lengths, out, n, ts, ta, sd,
                                     ad, max_lag, state_diff, ld_out, nonfinite, stream);
}
