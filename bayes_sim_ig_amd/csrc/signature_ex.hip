// include/bsig_signature.h in fp32: the width and cover queries (host arithmetic) and
// bsig_signature_ex.  The kernel, its LDS layout and the routing are csrc/signature_ex.h.
#include "signature_ex.h"

using namespace bsig;

// summarizers.py:144-168: the width of signatory's output for a path of dimension path_dim
extern "C" int64_t bsig_signature_ex_dim(int path_dim, int depth) {
  return sigex::row_width(path_dim, depth);
}

// summarizers.py:144-168 at any depth: is this shape covered
extern "C" int bsig_signature_ex_fits(int path_dim, int length, int depth, int itemsize) {
  BSIG_REQUIRE(path_dim >= 2, "signature_ex_fits: path_dim %d below 2", path_dim);
  BSIG_REQUIRE(length >= 2, "signature_ex_fits: length %d below 2", length);
  BSIG_REQUIRE(itemsize == 4 || itemsize == 8, "signature_ex_fits: itemsize %d is not 4 or 8", itemsize);
  BSIG_REQUIRE(depth <= BSIG_SIGNATURE_MAX_DEPTH, "signature_ex_fits: depth %d above %d", depth,
               BSIG_SIGNATURE_MAX_DEPTH);
  if (depth <= 0) depth = ref_signature_depth(path_dim);
  sigex::Layout g;
  size_t lds = 0;
  int threads = 0;
  return sigex::plan(itemsize == 8 ? "signature_ex_f64" : "signature_ex", path_dim, length, depth,
                     itemsize, &g, &lds, &threads);
}

// summarizers.py:144-168 in fp32
extern "C" int bsig_signature_ex(const float* states, const float* actions, const int32_t* channels,
                                 int n_channels, float* out, int64_t n, int length, int sd, int ad,
                                 int depth, int64_t ld_out, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_signature_ex");
  return sigex::run<float>("signature_ex", bsig_signature, kSummaryGridCap, states,
                           actions, channels, n_channels, out, n, length, sd, ad, depth, ld_out, stream);
}
