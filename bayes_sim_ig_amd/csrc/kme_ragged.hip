// include/bsig_ragged.h in fp32, the kernel mean embedding: bsig_kme_ragged and bsig_kme_rows_ragged on the
// templates of csrc/kme.h with every trajectory's own length.
#include "kme.h"

using namespace bsig;

extern "C" int bsig_kme_ragged(const float* states, const float* actions, const int32_t* lengths,
                               const float* coeff, int64_t ld_coeff, float* out, int64_t n, int ts, int ta, int sd,
                               int ad, int m, int diff, int time, int64_t ld_out, int32_t* nonfinite,
                               bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_ragged");
  return kme::run_any<float, true>("kme_ragged", kSummaryGridCap, states, actions, lengths, coeff, ld_coeff, out, n,
                                   ts, ta, sd, ad, m, diff, time, ld_out, nonfinite, stream);
}

extern "C" int bsig_kme_rows_ragged(const float* states, const float* actions, const int32_t* lengths,
                                    const int64_t* offsets, float* rows, int64_t n, int ts, int ta, int sd, int ad,
                                    int diff, int time, int64_t ld_rows, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_kme_rows_ragged");
  return kme::run_rows_ragged<float>("kme_rows_ragged", states, actions, lengths, offsets, rows, n, ts, ta, sd, ad,
                                     diff, time, ld_rows, stream);
}
