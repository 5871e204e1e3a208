// include/bsig_ragged.h in double, the kernel mean embedding: bsig_kme_ragged_f64 and bsig_kme_rows_ragged_f64,
// the fp64 twins of csrc/kme_ragged.hip on the same templates (csrc/kme.h).
#include "f64.h"
#include "../kme.h"

using namespace bsig;

extern "C" int bsig_kme_ragged_f64(const double* states, const double* actions, const int32_t* lengths,
                                   const double* coeff, int64_t ld_coeff, double* out, int64_t n, int ts, int ta,
                                   int sd, int ad, int m, int diff, int time, int64_t ld_out, int32_t* nonfinite,
                                   bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_ragged_f64");
  return kme::run_any<double, true>("kme_ragged_f64", BSIG_F64_SUMMARY_GRID_CAP, states, actions, lengths, coeff,
                                    ld_coeff, out, n, ts, ta, sd, ad, m, diff, time, ld_out, nonfinite, stream);
}

extern "C" int bsig_kme_rows_ragged_f64(const double* states, const double* actions, const int32_t* lengths,
                                        const int64_t* offsets, double* rows, int64_t n, int ts, int ta, int sd,
                                        int ad, int diff, int time, int64_t ld_rows, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_rows_ragged_f64");
  return kme::run_rows_ragged<double>("kme_rows_ragged_f64", states, actions, lengths, offsets, rows, n, ts, ta, sd,
                                      ad, diff, time, ld_rows, stream);
}
