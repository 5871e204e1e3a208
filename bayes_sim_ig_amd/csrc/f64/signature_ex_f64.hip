// include/bsig_signature.h in double: bsig_signature_ex_f64, the fp64 twin of csrc/signature_ex.hip on
// the same kernel template (csrc/signature_ex.h), every value a double.
#include "f64.h"
#include "../signature_ex.h"

using namespace bsig;

// summarizers.py:144-168 under torch.set_default_dtype(torch.float64)
extern "C" int bsig_signature_ex_f64(const double* states, const double* actions, const int32_t* channels,
                                     int n_channels, double* out, int64_t n, int length, int sd, int ad,
                                     int depth, int64_t ld_out, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_signature_ex_f64");
  return sigex::run<double>("signature_ex_f64", bsig_signature_f64, BSIG_F64_SUMMARY_GRID_CAP, states,
                            actions, channels, n_channels, out, n, length, sd, ad, depth, ld_out, stream);
}
