// include/bsig_rff_bandwidth.h: the workspace size (host arithmetic), the median bandwidth of fp32 and double rows,
// the selection stage on its own, and the coefficient from the device scalar in both precisions.  The kernels and
// the argument checks are csrc/rff_bandwidth.h.
#include "rff_bandwidth.h"

using namespace bsig;

extern "C" int64_t bsig_rff_bandwidth_workspace_bytes(int64_t n, int64_t width) {
  return rffbw::workspace_bytes(n, width);
}

// scale * median pairwise distance of fp32 rows
extern "C" int bsig_rff_bandwidth_median(const float* x, int64_t ld, int64_t n, int64_t width, double scale,
                                         double* sigma_out, void* workspace, size_t workspace_bytes,
                                         bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_rff_bandwidth_median");
  return rffbw::median_run<float>("rff_bandwidth_median", x, ld, n, width, scale, sigma_out, workspace,
                                  workspace_bytes, as_stream(stream));
}

// ... of double rows
extern "C" int bsig_rff_bandwidth_median_f64(const double* x, int64_t ld, int64_t n, int64_t width, double scale,
                                             double* sigma_out, void* workspace, size_t workspace_bytes,
                                             bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_rff_bandwidth_median_f64");
  return rffbw::median_run<double>("rff_bandwidth_median_f64", x, ld, n, width, scale, sigma_out, workspace,
                                   workspace_bytes, as_stream(stream));
}

// the lower median of non-negative doubles
extern "C" int bsig_rff_bandwidth_select(const double* values, int64_t count, double* out, void* workspace,
                                         size_t workspace_bytes, bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_rff_bandwidth_select");
  return rffbw::select_run("rff_bandwidth_select", values, count, out, workspace, workspace_bytes,
                           as_stream(stream));
}

// coeff = freqs / *sigma_dev, rounded once to fp32
extern "C" int bsig_rff_coeff_dev(const float* freqs, const double* sigma_dev, float* coeff, int64_t m, int64_t d,
                                  int64_t ld, bsig_stream_t stream) {
  return rffbw::coeff_run<float>("rff_coeff_dev", freqs, sigma_dev, coeff, m, d, ld, as_stream(stream));
}

// ... kept in double
extern "C" int bsig_rff_coeff_dev_f64(const float* freqs, const double* sigma_dev, double* coeff, int64_t m,
                                      int64_t d, int64_t ld, bsig_stream_t stream) {
  return rffbw::coeff_run<double>("rff_coeff_dev_f64", freqs, sigma_dev, coeff, m, d, ld, as_stream(stream));
}
