// The log-signature kernel (include/bsig_logsignature.h): the log of the truncated signature of
// X_l = [l+1 | picked channels], read at the Lyndon words, in fp32 (csrc/logsignature.hip) and in
// double (csrc/f64/logsignature_f64.hip) from this one template.
//
// Definition.  log S = sum_{n=1..depth} (-1)^(n+1)/n (S - 1)^(x)n in the truncated tensor algebra; the
// output row is its coefficients at the Lyndon words over 0 < 1 < ... < d-1 (0: the time channel),
// lengths 1..depth, by length, then lexicographically; Witt's formula gives the width.
//
// The kernel is sigex::path_levels (csrc/signature_ex.h) -- the path loop of the general signature
// kernel: its Layout and plan, its chains, one workgroup per trajectory, grid-strided -- with another
// tail.  When a path has ended, all levels lie in LDS, bitwise those signature_ex_kernel would store;
// instead of storing them, threads stride over the Lyndon words.  A word's flat offset into the
// signature row comes from the `words` table (DEVICE int32[width], made on the host by
// bsig_logsignature_words); its level k and letters are recovered by div/mod once (div_small), and
//   (log S)_w = sum over the 2^(k-1) ways to cut w into n >= 1 consecutive non-empty pieces u1..un
//               of (-1)^(n+1)/n S_u1 ... S_un
// is evaluated from the levels: cuts by ascending bit mask (bit j: a cut after letter j), each product
// from the left, its coefficient +-1/n (the rcp slots of the Layout) and the running sum in one fma.  At
// most 32 cuts; the code is specialised by k (add_cuts), so a word's at most 20 proper pieces are read
// from LDS once and the cuts are straight-line arithmetic.  One chain per output, no atomics, one store
// per output.  Mask 0 is S_w itself, so level 1 is the signature's level 1 bit for bit.
//
// LDS.  The tail reads `cur`, `topv` and `rcp` and needs nothing of its own: the LDS need is EXACTLY
// the general signature kernel's, sigex::plan decides for both and bsig_signature_ex_fits answers for
// both.  What plan refuses is BSIG_EUNSUPPORTED here too.
//
// Routing.  depth 1 is bsig_signature_ex[_f64] at depth 1, unchanged (`words` is not read); every other
// call runs this kernel, channels == NULL at depth <= 3 included: signature3_kernel / signature12_kernel
// keep their levels in registers and are not touched.
#pragma once
#include "signature_ex.h"
#include "../../include/bsig_logsignature.h"

namespace bsig {
namespace logsig {

static_assert(BSIG_SIGNATURE_MAX_DEPTH == 6, "LyndonLog switches over the word lengths 2..6");

// The number of Lyndon words of length k over d letters (Witt), d^k below 2^31.
inline int64_t witt(int64_t d, int k) {
  static const int mu[7] = {0, 1, -1, -1, 0, -1, 1};
  int64_t tot = 0;
  for (int e = 1; e <= k; ++e) {
    if (k % e || !mu[e]) continue;
    int64_t p = 1;
    for (int q = 0; q < k / e; ++q) p *= d;
    tot += mu[e] * p;
  }
  return tot / k;
}

// -1 where sigex::row_width is
inline int64_t row_width(int64_t d, int depth) {
  if (sigex::row_width(d, depth) < 0) return -1;
  int64_t tot = 0;
  for (int k = 1; k <= depth; ++k) tot += witt(d, k);
  return tot;
}

// Duval's algorithm: every Lyndon word of length <= depth over d letters, in lexicographic order; a
// word of length k goes to the next free slot of its length's block, so each block is in lexicographic
// order too.  `words` has row_width(d, depth) elements.
inline void fill_words(int d, int depth, int32_t* words) {
  int64_t slot[BSIG_SIGNATURE_MAX_DEPTH + 2] = {}, base[BSIG_SIGNATURE_MAX_DEPTH + 2] = {};
  int64_t p = 1;
  for (int k = 1; k <= depth; ++k) {            // base[k]: where level k starts in the signature row
    slot[k + 1] = slot[k] + witt(d, k);
    base[k + 1] = base[k] + (p *= d);
  }
  int w[BSIG_SIGNATURE_MAX_DEPTH] = {-1};
  int len = 1;
  while (len > 0) {
    ++w[len - 1];
    int64_t idx = 0;
    for (int j = 0; j < len; ++j) idx = idx * d + w[j];
    words[slot[len]++] = (int32_t)(base[len] + idx);
    for (int j = len; j < depth; ++j) w[j] = w[j - len];
    len = depth;
    while (len > 0 && w[len - 1] == d - 1) --len;
  }
}

// x / d for 0 <= x < 2^22 and d >= 2 (x indexes a workgroup's LDS: below 2^16) without the integer
// division: x is exact as a float, rd = 1/d rounded, so the truncated float quotient is off by one at most.
__device__ __forceinline__ int div_small(int x, int d, float rd) {
  const int q = (int)((float)x * rd);
  const int r = x - q * d;
  return q + (r >= d) - (r < 0);
}

// (log S)_w - S_w for a word of K letters, added to `acc` = S_w: the cuts with n >= 2 pieces, by ascending
// mask.  K is a compile-time constant, so the cuts are too: the K (K + 1) / 2 - 1 proper pieces of w are
// read from LDS once, ahead of the arithmetic (a cut's product is the same multiplies from the left
// whether its factors are read again or not), and nothing below branches.  `rem` is w's index in level K.
template <typename T, int K>
__device__ __forceinline__ T add_cuts(T acc, const T* cur, const T* rcp, int rem, int d, float rd) {
  int letter[K], idx[K];                           // (every index static once unrolled: registers)
#pragma unroll
  for (int m = K - 1; m >= 0; --m) {
    const int q = div_small(rem, d, rd);
    letter[m] = rem - q * d;
    rem = q;
    idx[m] = 0;
  }
  T piece[K][K];                                   // piece[s][l - 1]: S at letters s .. s + l - 1, l < K
  int off = 0, pw = d;                             // where level l starts, its size
#pragma unroll
  for (int l = 1; l < K; ++l) {
#pragma unroll
    for (int s = 0; s + l <= K; ++s) {
      idx[s] = idx[s] * d + letter[s + l - 1];
      piece[s][l - 1] = cur[off + idx[s]];
    }
    off += pw;
    pw *= d;
  }
#pragma unroll
  for (int mask = 1; mask < (1 << (K - 1)); ++mask) {
    T prod = (T)1;
    int n = 0, s = 0;
#pragma unroll
    for (int j = 0; j < K; ++j) {
      if (j == K - 1 || ((mask >> j) & 1)) {
        const T f = piece[s][j - s];
        prod = n ? prod * f : f;
        ++n;
        s = j + 1;
      }
    }
    acc = fma(prod, (n & 1) ? rcp[n] : -rcp[n], acc);
  }
  return acc;
}

// The tail of sigex::path_levels that writes the log-signature row (see the top of this file).
template <typename T>
struct LyndonLog {
  const int32_t* __restrict__ words;
  int n_words;

  __device__ __forceinline__ void operator()(T* __restrict__ o, const T* cur, const T* topv, const T* rcp,
                                             const sigex::Layout& g, int tid, int nt) const {
    const int d = g.d, low = g.low;
    const float rd = 1.0f / (float)d;
    for (int e = tid; e < n_words; e += nt) {
      const int at = words[e];
      int k = 1, base = 0, cnt = d;                // level k holds [base, base + d^k) of the row
      while (at >= base + cnt) { base += cnt; cnt *= d; ++k; }
      T acc = at < low ? cur[at] : topv[at - low];           // mask 0: the word itself
      switch (k) {                                 // (the words come by length: a wave mostly takes one case)
        case 2: acc = add_cuts<T, 2>(acc, cur, rcp, at - base, d, rd); break;
        case 3: acc = add_cuts<T, 3>(acc, cur, rcp, at - base, d, rd); break;
        case 4: acc = add_cuts<T, 4>(acc, cur, rcp, at - base, d, rd); break;
        case 5: acc = add_cuts<T, 5>(acc, cur, rcp, at - base, d, rd); break;
        case 6: acc = add_cuts<T, 6>(acc, cur, rcp, at - base, d, rd); break;
        default: break;                            // level 1: S_w
      }
      o[e] = acc;
    }
  }
};

template <typename T>
__global__ __launch_bounds__(sigex::kMaxThreads) void logsignature_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, const int32_t* __restrict__ channels,
    const int32_t* __restrict__ words, int n_words, T* __restrict__ out, int64_t n, int length, int sd,
    int ad, int64_t ld_out, sigex::Layout g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char logsig_smem[];
  sigex::path_levels<T>(logsig_smem, states, actions, channels, out, n, length, sd, ad, ld_out, g,
                        LyndonLog<T>{words, n_words});
}

// The entry point of either precision: the argument checks, the routing, the launch.  `level1` is
// bsig_signature_ex / bsig_signature_ex_f64; `max_grid` the precision's workgroup cap.
template <typename T, typename Level1>
int run(const char* what, Level1 level1, int64_t max_grid, const T* states, const T* actions,
        const int32_t* channels, int n_channels, const int32_t* words, T* out, int64_t n, int length,
        int sd, int ad, int depth, int64_t ld_out, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "%s: bad n=%lld", what, (long long)n);
  BSIG_REQUIRE(depth <= BSIG_SIGNATURE_MAX_DEPTH, "%s: depth %d above %d", what, depth,
               BSIG_SIGNATURE_MAX_DEPTH);
  BSIG_REQUIRE(length >= 2, "%s: length %d below 2", what, length);
  BSIG_REQUIRE(sd >= 1 && ad >= 1, "%s: bad dims sd=%d ad=%d", what, sd, ad);
  BSIG_REQUIRE(states && actions && out, "%s: null pointer", what);
  BSIG_REQUIRE(!channels || n_channels >= 1, "%s: channels given with n_channels=%d", what, n_channels);
  const int64_t d = 1 + (channels ? (int64_t)n_channels : (int64_t)sd + ad);
  BSIG_REQUIRE(d <= INT32_MAX, "%s: path dim %lld too large", what, (long long)d);
  if (depth <= 0) depth = ref_signature_depth(d);
  if (depth <= 1)      // the log-signature is level 1: the signature's depth-1 branch, unchanged
    return level1(states, actions, channels, n_channels, out, n, length, sd, ad, depth, ld_out, stream);
  BSIG_REQUIRE(words, "%s: null words at depth %d", what, depth);
  const int64_t width = row_width(d, depth);
  BSIG_REQUIRE(width < 0 || ld_out >= width, "%s: ld_out %lld below the width %lld", what,
               (long long)ld_out, (long long)width);
  sigex::Layout g;
  size_t lds = 0;
  int threads = 0;
  BSIG_TRY(sigex::plan(what, d, length, depth, (int)sizeof(T), &g, &lds, &threads));
  static LdsRaised raised;
  if (lds > kLdsUnraised) BSIG_TRY(raise_lds_limit(logsignature_kernel<T>, kLdsBytes, &raised));
  hipLaunchKernelGGL((logsignature_kernel<T>), dim3(capped_grid(n, max_grid)),
                     dim3(threads), lds, as_stream(stream), states, actions, channels, words, (int)width,
                     out, n, length, sd, ad, ld_out, g);
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

}  // namespace logsig
}  // namespace bsig
