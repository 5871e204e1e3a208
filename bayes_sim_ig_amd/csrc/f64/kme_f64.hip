// include/bsig_kme.h in double: bsig_kme_rows_f64, bsig_kme_coeff_f64 and bsig_kme_f64, the fp64 twins of
// csrc/kme.hip on the same templates (csrc/kme.h), every value a double.
#include "f64.h"
#include "../kme.h"

using namespace bsig;

extern "C" int bsig_kme_rows_f64(const double* states, const double* actions, double* rows, int64_t n, int ts,
                                 int ta, int sd, int ad, int diff, int time, int64_t ld_rows,
                                 bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_rows_f64");
  return kme::run_rows<double>("kme_rows_f64", states, actions, rows, n, ts, ta, sd, ad, diff, time, ld_rows,
                               stream);
}

extern "C" int bsig_kme_coeff_f64(const float* freqs, int64_t ld_freqs, const double* inv_std, double kappa,
                                  double* coeff, int64_t ld_coeff, int64_t m, int64_t d, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_coeff_f64");
  return kme::run_coeff<double>("kme_coeff_f64", freqs, ld_freqs, inv_std, kappa, coeff, ld_coeff, m, d, stream);
}

extern "C" int bsig_kme_f64(const double* states, const double* actions, const double* coeff, int64_t ld_coeff,
                            double* out, int64_t n, int ts, int ta, int sd, int ad, int m, int diff, int time,
                            int64_t ld_out, int32_t* nonfinite, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_f64");
  return kme::run<double>("kme_f64", BSIG_F64_SUMMARY_GRID_CAP, states, actions, coeff, ld_coeff, out, n, ts, ta,
                          sd, ad, m, diff, time, ld_out, nonfinite, stream);
}
