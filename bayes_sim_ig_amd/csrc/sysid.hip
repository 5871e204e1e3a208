// include/bsig_sysid.h in fp32: the width, cover and group queries (host arithmetic) and bsig_sysid.
// The kernel, its LDS layout and the launch shape are csrc/sysid.h.
#include "sysid.h"

using namespace bsig;

extern "C" int64_t bsig_sysid_dim(int sd, int ad) { return sysid::row_width(sd, ad); }

static int plan_for(const char* query, int ts, int ta, int sd, int ad, int itemsize, sysid::Plan* p) {
  BSIG_REQUIRE(itemsize == 4 || itemsize == 8, "%s: itemsize %d is not 4 or 8", query, itemsize);
  return sysid::plan(itemsize == 8 ? "sysid_f64" : "sysid", ts, ta, sd, ad, itemsize, p);
}

extern "C" int bsig_sysid_fits(int ts, int ta, int sd, int ad, int itemsize) {
  sysid::Plan p;
  return plan_for("sysid_fits", ts, ta, sd, ad, itemsize, &p);
}

extern "C" int bsig_sysid_group(int ts, int ta, int sd, int ad, int itemsize) {
  sysid::Plan p;
  BSIG_TRY(plan_for("sysid_group", ts, ta, sd, ad, itemsize, &p));
  return p.group;
}

extern "C" int bsig_sysid(const float* states, const float* actions, float* out, int64_t n, int ts, int ta,
                          int sd, int ad, double ridge, int64_t ld_out, int32_t* nonfinite,
                          bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sysid");
  return sysid::run<float>("sysid", kSummaryGridCap, states, actions, out, n, ts, ta, sd, ad, ridge, ld_out,
                           nonfinite, stream);
}
