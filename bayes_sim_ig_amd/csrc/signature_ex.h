// The general signature kernel (include/bsig_signature.h): any depth up to BSIG_SIGNATURE_MAX_DEPTH on
// the path X_l = [l+1 | picked channels] of summarizers.py:144-168, in fp32 (csrc/signature_ex.hip) and
// in double (csrc/f64/signature_ex_f64.hip) from this one template.  Nothing here is tuned: the depth
// <= 3 launches of the default path stay on signature3_kernel / signature12_kernel.
//
// One workgroup per trajectory, grid-strided.  All levels of the trajectory live in LDS for the whole
// path.  Per segment l with increment D, Chen's identity S <- S (x) exp(D), level by level in the
// Horner form signature3_kernel's comment gives for k = 3:
//   S_k[i1..ik] += (...((D[i1]/k + S_1[i1]) D[i2]/(k-1) + S_2[i1,i2]) D[i3]/(k-2) ...) D[ik]
// The unit of work is a ROW: a level k and a prefix (i1..i_(k-1)); its thread evaluates the bracket
// once (k-1 steps, two LDS reads each) and adds bracket * D[ik] to the d terms of the row.  There are
// 1 + d + ... + d^(depth-1) rows and threads stride over them.  The bracket reads the levels below k
// as they were BEFORE this segment, so those levels exist twice: a segment reads one copy and writes
// the other, the top level (which no bracket reads) is updated in place, and ONE barrier per segment
// separates the roles.  Every output is one chain in ascending segment order; no atomics.
//
// LDS of a workgroup (Layout): levels 1..depth-1 [low] twice | level depth [top] | increments
// [(length-1) d] | reciprocals 1/1..1/6 | per row: its level and the digits of its prefix, 8 bits each
// (computed once per workgroup: a row costs no integer division per segment) | channel of each path
// column.  Access: a row's d terms are consecutive, rows of neighbouring lanes lie d elements apart --
// conflict free for odd d, a gcd(d, 32)-way conflict in fp32 for even d (left as it is); D[ik] is
// the same address in every lane (broadcast).
#pragma once
#include <algorithm>
#include <climits>

#include "common.h"
#include "../../include/bsig_signature.h"

namespace bsig {
namespace sigex {

constexpr int kMaxThreads = 1024;

struct Layout {          // byte offsets into the dynamic LDS, each a multiple of 16
  int d = 0, depth = 0, low = 0, top = 0, rows = 0;
  int off_b = 0, off_top = 0, off_delta = 0, off_rcp = 0, off_rows = 0, off_src = 0;
};

inline int64_t row_width(int64_t d, int depth) {
  if (d < 2 || d > INT32_MAX || depth < 1 || depth > BSIG_SIGNATURE_MAX_DEPTH) return -1;
  int64_t tot = 0, p = 1;
  for (int q = 1; q <= depth; ++q) {
    p *= d;                               // (p and d are below 2^31 here)
    tot += p;
    if (tot > INT32_MAX) return -1;
  }
  return tot;
}

// The launch shape of the general kernel, or why there is none.  depth in 1..MAX, d >= 2, length >= 2.
inline int plan(const char* what, int64_t d, int length, int depth, int itemsize, Layout* g,
                size_t* lds, int* threads) {
  if (depth == 1) {
    g->d = (int)d; g->depth = 1;
    *lds = 0;
    *threads = (int)std::min<int64_t>(round_up<int64_t>(d, 64), 256);
    return BSIG_OK;
  }
  const int64_t width = row_width(d, depth);
  int64_t top = 1;
  if (width > 0) for (int q = 0; q < depth; ++q) top *= d;
  // (a prefix digit is stored in 8 bits; d^2 elements alone exceed the LDS long before d = 256)
  if (width < 0 || d > 255 || width * itemsize > (int64_t)kLdsBytes) {
    set_error("%s: depth %d on path dim %lld needs more than a workgroup's %zu B of LDS for its levels",
              what, depth, (long long)d, kLdsBytes);
    return BSIG_EUNSUPPORTED;
  }
  const int64_t low = width - top, rows = low + 1;
  auto r16 = [](int64_t b) { return (b + 15) & ~(int64_t)15; };
  const int64_t off_b = r16(low * itemsize);
  const int64_t off_top = off_b + r16(low * itemsize);
  const int64_t off_delta = off_top + r16(top * itemsize);
  const int64_t off_rcp = off_delta + r16((int64_t)(length - 1) * d * itemsize);
  const int64_t off_rows = off_rcp + r16(8 * itemsize);
  const int64_t off_src = off_rows + r16(rows * 8);
  const int64_t bytes = off_src + r16(d * 4);
  if (bytes > (int64_t)kLdsBytes) {
    set_error("%s: %lld B of LDS needed for depth %d on path dim %lld, length %d (%zu in a workgroup)",
              what, (long long)bytes, depth, (long long)d, length, kLdsBytes);
    return BSIG_EUNSUPPORTED;
  }
  g->d = (int)d; g->depth = depth; g->low = (int)low; g->top = (int)top; g->rows = (int)rows;
  g->off_b = (int)off_b; g->off_top = (int)off_top; g->off_delta = (int)off_delta;
  g->off_rcp = (int)off_rcp; g->off_rows = (int)off_rows; g->off_src = (int)off_src;
  *lds = (size_t)bytes;
  *threads = (int)std::min<int64_t>(round_up<int64_t>(rows, 64), kMaxThreads);
  return BSIG_OK;
}

// What a workgroup does with a trajectory's levels once its path has ended: the signature's own tail
// stores them, levels 1..depth concatenated.  (csrc/logsignature.h has the other tail.)
template <typename T>
struct StoreLevels {
  __device__ __forceinline__ void operator()(T* __restrict__ o, const T* cur, const T* topv, const T*,
                                             const Layout& g, int tid, int nt) const {
    const int low = g.low, width = g.low + g.top;
    for (int e = tid; e < width; e += nt) o[e] = e < low ? cur[e] : topv[e - low];
  }
};

// The path loop at depth >= 2, shared by every kernel that needs the levels of a trajectory: the LDS
// of the Layout, the set-up once per workgroup, the trajectories grid-strided, one barrier per segment.
// When a path has ended, `tail(o, cur, topv, rcp, g, tid, nt)` finds levels 1..depth-1 in `cur`, level
// depth in `topv`, the reciprocals in `rcp`, all of them stable until the whole workgroup has left it
// (the barrier that opens the next trajectory), and writes the trajectory's output row `o`.
template <typename T, typename Tail>
__device__ __forceinline__ void path_levels(
    unsigned char* sigex_smem, const T* __restrict__ states, const T* __restrict__ actions,
    const int32_t* __restrict__ channels, T* __restrict__ out, int64_t n, int length, int sd, int ad,
    int64_t ld_out, const Layout& g, Tail tail) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int d = g.d, depth = g.depth;
  T* buf_a = reinterpret_cast<T*>(sigex_smem);                  // levels 1..depth-1
  T* buf_b = reinterpret_cast<T*>(sigex_smem + g.off_b);        // levels 1..depth-1, the other copy
  T* topv = reinterpret_cast<T*>(sigex_smem + g.off_top);       // level depth
  T* delta = reinterpret_cast<T*>(sigex_smem + g.off_delta);    // [(length-1) * d]
  T* rcp = reinterpret_cast<T*>(sigex_smem + g.off_rcp);        // rcp[m] = 1/m
  uint64_t* rowinfo = reinterpret_cast<uint64_t*>(sigex_smem + g.off_rows);
  int32_t* src = reinterpret_cast<int32_t*>(sigex_smem + g.off_src);   // channel of path column 1 + c
  const int low = g.low, top = g.top, nrows = g.rows;

  // ---- once per workgroup
  for (int c = tid; c < d - 1; c += nt) src[c] = channels ? channels[c] : c;
  if (tid < 8)
    rcp[tid] = tid == 2 ? (T)0.5 : tid == 3 ? (T)1 / (T)3 : tid == 4 ? (T)0.25
             : tid == 5 ? (T)1 / (T)5 : tid == 6 ? (T)1 / (T)6 : (T)1;
  for (int r = tid; r < nrows; r += nt) {
    int k = 1, base = 0, cnt = 1;                  // level k holds rows [base, base + d^(k-1))
    while (r >= base + cnt) { base += cnt; cnt *= d; ++k; }
    int rem = r - base;
    uint64_t digits = 0;                           // i1 in the low byte
    for (int m = 1; m < k; ++m) {
      digits = (digits << 8) | (uint64_t)(rem % d);
      rem /= d;
    }
    rowinfo[r] = digits | ((uint64_t)k << 48);
  }

  for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
    const T* s = states + traj * (int64_t)length * sd;
    const T* a = actions + traj * (int64_t)length * ad;
    T* o = out + traj * ld_out;
    __syncthreads();              // the set-up above / the trajectory before is done with the levels
    for (int e = tid; e < (length - 1) * d; e += nt) {
      const int l = e / d, c = e - l * d;
      T v = (T)1;                                  // the time channel: (l + 2) - (l + 1)
      if (c > 0) {
        const int ch = src[c - 1];
        if (ch < sd) {
          const T* q = s + (int64_t)l * sd + ch;
          v = q[sd] - q[0];
        } else {
          const T* q = a + (int64_t)l * ad + (ch - sd);
          v = q[ad] - q[0];
        }
      }
      delta[e] = v;
    }
    for (int e = tid; e < low; e += nt) buf_a[e] = (T)0;
    for (int e = tid; e < top; e += nt) topv[e] = (T)0;
    __syncthreads();
    T* cur = buf_a;
    T* nxt = buf_b;
    for (int l = 0; l + 1 < length; ++l) {
      const T* dl = delta + l * d;
      for (int r = tid; r < nrows; r += nt) {
        uint64_t dg = rowinfo[r];
        const int k = (int)(dg >> 48);
        T t = (T)1;
        int idx = 0, off = 0, pw = d;              // prefix (i1..im), where level m starts, its size
        for (int m = 1; m < k; ++m) {
          const int i = (int)(dg & 0xff);
          dg >>= 8;
          idx = idx * d + i;
          t = fma(t * dl[i], rcp[k - m + 1], cur[off + idx]);
          off += pw;
          pw *= d;
        }
        const T* from = k < depth ? cur + off + idx * d : topv + idx * d;
        T* to = k < depth ? nxt + off + idx * d : topv + idx * d;
        for (int j = 0; j < d; ++j) to[j] = fma(t, dl[j], from[j]);
      }
      __syncthreads();
      T* sw = cur; cur = nxt; nxt = sw;
    }
    tail(o, cur, topv, rcp, g, tid, nt);
  }
}

template <typename T>
__global__ __launch_bounds__(kMaxThreads) void signature_ex_kernel(
    const T* __restrict__ states, const T* __restrict__ actions, const int32_t* __restrict__ channels,
    T* __restrict__ out, int64_t n, int length, int sd, int ad, int64_t ld_out, Layout g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char sigex_smem[];
  const int tid = threadIdx.x, nt = blockDim.x;
  const int d = g.d, depth = g.depth;
  if (depth == 1) {                      // last - first point (time channel: L-1); no LDS
    for (int64_t traj = blockIdx.x; traj < n; traj += gridDim.x) {
      const T* s = states + traj * (int64_t)length * sd;
      const T* a = actions + traj * (int64_t)length * ad;
      T* o = out + traj * ld_out;
      for (int c = tid; c < d; c += nt) {
        T v;
        if (c == 0) {
          v = (T)(length - 1);
        } else {
          const int ch = channels ? channels[c - 1] : c - 1;
          v = ch < sd ? s[(int64_t)(length - 1) * sd + ch] - s[ch]
                      : a[(int64_t)(length - 1) * ad + ch - sd] - a[ch - sd];
        }
        o[c] = v;
      }
    }
    return;
  }
  path_levels<T>(sigex_smem, states, actions, channels, out, n, length, sd, ad, ld_out, g,
                 StoreLevels<T>());
}

// The entry point of either precision: the argument checks, the routing of include/bsig_signature.h,
// the launch.  `legacy` is bsig_signature / bsig_signature_f64; `max_grid` the precision's workgroup cap.
template <typename T, typename Legacy>
int run(const char* what, Legacy legacy, int64_t max_grid, const T* states, const T* actions,
        const int32_t* channels, int n_channels, T* out, int64_t n, int length, int sd, int ad,
        int depth, int64_t ld_out, bsig_stream_t stream) {
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
  if (!channels && depth <= 3)
    return legacy(states, actions, out, n, length, sd, ad, depth, ld_out, stream);
  const int64_t width = row_width(d, depth);
  BSIG_REQUIRE(width < 0 || ld_out >= width, "%s: ld_out %lld below the width %lld", what,
               (long long)ld_out, (long long)width);
  Layout g;
  size_t lds = 0;
  int threads = 0;
  BSIG_TRY(plan(what, d, length, depth, (int)sizeof(T), &g, &lds, &threads));
  static LdsRaised raised;
  if (lds > kLdsUnraised) BSIG_TRY(raise_lds_limit(signature_ex_kernel<T>, kLdsBytes, &raised));
  hipLaunchKernelGGL((signature_ex_kernel<T>), dim3(capped_grid(n, max_grid)),
                     dim3(threads), lds, as_stream(stream), states, actions, channels, out, n, length,
                     sd, ad, ld_out, g);
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

}  // namespace sigex
}  // namespace bsig
