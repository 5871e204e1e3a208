// include/bsig_logsignature.h in fp32: the width and the words table (host arithmetic) and
// bsig_logsignature.  The kernel, its epilogue and the routing are csrc/logsignature.h.
#include "logsignature.h"

using namespace bsig;

// the number of Lyndon words of length 1..depth over path_dim letters
extern "C" int64_t bsig_logsignature_dim(int path_dim, int depth) {
  return logsig::row_width(path_dim, depth);
}

// per output element, the flat offset of its Lyndon word in the signature row
extern "C" int bsig_logsignature_words(int path_dim, int depth, int32_t* words_host, int64_t capacity) {
  const int64_t width = logsig::row_width(path_dim, depth);
  BSIG_REQUIRE(width > 0, "logsignature_words: no log-signature row for path_dim %d, depth %d", path_dim,
               depth);
  BSIG_REQUIRE(words_host, "logsignature_words: null words_host");
  BSIG_REQUIRE(capacity >= width, "logsignature_words: capacity %lld below the width %lld",
               (long long)capacity, (long long)width);
  logsig::fill_words(path_dim, depth, words_host);
  return BSIG_OK;
}

// the log-signature at the Lyndon words in fp32
extern "C" int bsig_logsignature(const float* states, const float* actions, const int32_t* channels,
                                 int n_channels, const int32_t* words, float* out, int64_t n, int length,
                                 int sd, int ad, int depth, int64_t ld_out, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_logsignature");
  return logsig::run<float>("logsignature", bsig_signature_ex, kSummaryGridCap, states,
                            actions, channels, n_channels, words, out, n, length, sd, ad, depth, ld_out,
                            stream);
}
