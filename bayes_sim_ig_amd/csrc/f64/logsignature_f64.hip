// include/bsig_logsignature.h in double: bsig_logsignature_f64, the fp64 twin of csrc/logsignature.hip on
// the same kernel template (csrc/logsignature.h), every value a double.
#include "f64.h"
#include "../logsignature.h"

using namespace bsig;

// the log-signature at the Lyndon words in double
extern "C" int bsig_logsignature_f64(const double* states, const double* actions, const int32_t* channels,
                                     int n_channels, const int32_t* words, double* out, int64_t n,
                                     int length, int sd, int ad, int depth, int64_t ld_out,
                                     bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_logsignature_f64");
  return logsig::run<double>("logsignature_f64", bsig_signature_ex_f64, BSIG_F64_SUMMARY_GRID_CAP, states,
                             actions, channels, n_channels, words, out, n, length, sd, ad, depth, ld_out,
                             stream);
}
