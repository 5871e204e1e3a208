// include/bsig_sysid.h in double: bsig_sysid_f64, the fp64 twin of csrc/sysid.hip on the same kernel
// template (csrc/sysid.h), every value a double.
#include "f64.h"
#include "../sysid.h"

using namespace bsig;

extern "C" int bsig_sysid_f64(const double* states, const double* actions, double* out, int64_t n, int ts,
                              int ta, int sd, int ad, double ridge, int64_t ld_out, int32_t* nonfinite,
                              bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_sysid_f64");
  return sysid::run<double>("sysid_f64", BSIG_F64_SUMMARY_GRID_CAP, states, actions, out, n, ts, ta, sd, ad,
                            ridge, ld_out, nonfinite, stream);
}
