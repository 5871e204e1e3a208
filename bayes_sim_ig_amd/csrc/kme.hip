// include/bsig_kme.h in fp32: the width, cover and group queries (host arithmetic), bsig_kme_rows,
// bsig_kme_coeff and bsig_kme.  The kernels, the LDS layout and the launch shape are csrc/kme.h.
#include "kme.h"

using namespace bsig;

extern "C" int64_t bsig_kme_row_dim(int sd, int ad, int diff, int time) { return kme::row_dim(sd, ad, diff, time); }

static int plan_for(const char* query, int ts, int ta, int sd, int ad, int m, int diff, int time, int itemsize,
                    kme::Plan* p) {
  BSIG_REQUIRE(itemsize == 4 || itemsize == 8, "%s: itemsize %d is not 4 or 8", query, itemsize);
  return kme::plan(itemsize == 8 ? "kme_f64" : "kme", ts, ta, sd, ad, m, diff, time, itemsize, p);
}

extern "C" int bsig_kme_fits(int ts, int ta, int sd, int ad, int m, int diff, int time, int itemsize) {
  kme::Plan p;
  return plan_for("kme_fits", ts, ta, sd, ad, m, diff, time, itemsize, &p);
}

extern "C" int bsig_kme_group(int ts, int ta, int sd, int ad, int m, int diff, int time, int itemsize) {
  kme::Plan p;
  BSIG_TRY(plan_for("kme_group", ts, ta, sd, ad, m, diff, time, itemsize, &p));
  return p.group;
}

extern "C" int bsig_kme_rows(const float* states, const float* actions, float* rows, int64_t n, int ts, int ta,
                             int sd, int ad, int diff, int time, int64_t ld_rows, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_rows");
  return kme::run_rows<float>("kme_rows", states, actions, rows, n, ts, ta, sd, ad, diff, time, ld_rows, stream);
}

extern "C" int bsig_kme_coeff(const float* freqs, int64_t ld_freqs, const double* inv_std, double kappa,
                              float* coeff, int64_t ld_coeff, int64_t m, int64_t d, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_coeff");
  return kme::run_coeff<float>("kme_coeff", freqs, ld_freqs, inv_std, kappa, coeff, ld_coeff, m, d, stream);
}

extern "C" int bsig_kme(const float* states, const float* actions, const float* coeff, int64_t ld_coeff,
                        float* out, int64_t n, int ts, int ta, int sd, int ad, int m, int diff, int time,
                        int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme");
  return kme::run<float>("kme", kSummaryGridCap, states, actions, coeff, ld_coeff, out, n, ts, ta, sd, ad, m,
                         diff, time, ld_out, nonfinite, stream);
}
