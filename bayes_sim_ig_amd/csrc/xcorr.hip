// include/bsig_xcorr.h in fp32: the width, cover and group queries (host arithmetic) and bsig_xcorr.
// The kernel, its LDS layout and the launch shape are csrc/xcorr.h.
#include "xcorr.h"

using namespace bsig;

extern "C" int64_t bsig_xcorr_dim(int sd, int ad, int max_lag) { return xcorr::row_width(sd, ad, max_lag); }

static int plan_for(const char* query, int length, int ta, int sd, int ad, int max_lag, int state_diff,
                    int itemsize, xcorr::Plan* p) {
  BSIG_REQUIRE(itemsize == 4 || itemsize == 8, "%s: itemsize %d is not 4 or 8", query, itemsize);
  return xcorr::plan(itemsize == 8 ? "xcorr_f64" : "xcorr", length, ta, sd, ad, max_lag, state_diff, itemsize,
                     p);
}

extern "C" int bsig_xcorr_fits(int length, int ta, int sd, int ad, int max_lag, int state_diff,
                               int itemsize) {
  xcorr::Plan p;
  return plan_for("xcorr_fits", length, ta, sd, ad, max_lag, state_diff, itemsize, &p);
}

extern "C" int bsig_xcorr_group(int length, int ta, int sd, int ad, int max_lag, int state_diff,
                                int itemsize) {
  xcorr::Plan p;
  BSIG_TRY(plan_for("xcorr_group", length, ta, sd, ad, max_lag, state_diff, itemsize, &p));
  return p.group;
}

extern "C" int bsig_xcorr(const float* states, const float* actions, float* out, int64_t n, int ts, int ta,
                          int sd, int ad, int max_lag, int state_diff, int64_t ld_out, int32_t* nonfinite,
                          bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_xcorr");
  return xcorr::run<float>("xcorr", kSummaryGridCap, states, actions, out, n, ts, ta, sd, ad, max_lag,
                           state_diff, ld_out, nonfinite, stream);
}
