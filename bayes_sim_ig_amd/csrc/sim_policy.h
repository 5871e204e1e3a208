// The MLP policy of include/bsig_sim_policy.h as the Policy parameter of rollout_kernel (csrc/sim.h): what the
// kernel asks of it is stage() once per workgroup, the block's replace marks, and action() in the walk of
// phase 2.  Every operation is double and uncontracted, in the header's order: z_j = b_j, then for k ascending
// z_j = z_j + (W_jk * x_k).
//
// The design points.
// Weights: staged ONCE per workgroup into the dynamic LDS, before the first episode batch; the first barrier of
//   the step-block loop orders the staging before any use.  A hidden layer is stored TRANSPOSED, [in][outp] with
//   outp = out rounded up to kUnits and the padding zero, its bias [outp] behind it; the output layer is its
//   row [in] and its bias.  Every lane reads a weight at the SAME address, a broadcast without a bank conflict;
//   the kUnits weights of one term lie side by side, 32 bytes on a 32-byte boundary.
// Units side by side: kUnits = BSIG_SIM_POLICY_UNITS = 4 units of a layer are formed together: their
//   accumulators are compile-time registers, an input x_k is read once for the four, and four independent
//   add chains are in flight (one chain alone would wait a double add's latency per term).  The order of
//   roundings INSIDE a unit is untouched.  A unit at or beyond the width (the padding) is formed from zeros and
//   never used.
// Layer vectors: no per-thread array is indexed at run time, so nothing goes to scratch.  The observation and
//   the four accumulators are registers.  The LAST hidden layer is never stored: unit j is consumed the moment
//   it is formed, by the output's z = z + (W_j * h_j), which wants its terms in exactly that order.  Only with
//   two hidden layers is the first one stored, in LDS as [unit][lane] (consecutive lanes on consecutive 8-byte
//   words: no bank conflict; a lane reads only what it wrote itself, so no barrier).
// LDS size: from the widths (layout() below, shared by the host's launch and the kernel), not from the cap: the
//   weights, h0p * 64 doubles of layer vector when there are two hidden layers, and the replace marks of a step
//   block (64 * 8 bytes).  At (64, 64) on CartPole that is 36 360 + 32 768 + 512 bytes on top of the kernel's
//   static staging rows; at () it is 40 + 512.
// Divergence: a lane whose step is replaced, or whose episode has ended, skips action()'s evaluation.  Nothing
//   in it is a barrier and every trip count is a function of the widths alone.
#pragma once
#include "../../include/bsig_sim_policy.h"
#include "sim.h"

namespace bsig {
namespace sim {

constexpr int kUnits = BSIG_SIM_POLICY_UNITS;

struct MlpPolicy {
  static constexpr bool kOn = true;
  const double* packed;     // W_0, b_0, W_1, b_1, ... row-major (DEVICE)
  const uint8_t* replace;   // [N, Ta] or null
  int nl, h0, h1, act;

  // Offsets into the dynamic LDS, in doubles: the layers, the stored layer vector, the replace marks; bytes.
  struct Layout { int l0, l1, out, hid, marks, bytes; };
  __host__ __device__ Layout layout(int sd) const {
    Layout y;
    const int h0p = round_up(h0, kUnits), h1p = round_up(h1, kUnits);
    y.l0 = 0;
    y.l1 = nl >= 1 ? sd * h0p + h0p : 0;
    y.out = nl == 2 ? y.l1 + h0 * h1p + h1p : y.l1;
    const int last = nl == 0 ? sd : (nl == 1 ? h0 : h1);
    y.hid = round_up(y.out + last + 1, 2);                   // (a 16-byte boundary)
    y.marks = y.hid + (nl == 2 ? h0p * kEpisodes : 0);
    y.bytes = y.marks * (int)sizeof(double) + kEpisodes * kBlock;
    return y;
  }
  __host__ __device__ int lds_bytes(int sd) const { return layout(sd).bytes; }
  // what a launch asks the runtime for once it needs more than kLdsUnraised: above (64, 64) on CartPole, 69 648
  static constexpr int kMaxLdsBytes = 72 * 1024;

  // One hidden layer W [out, in], b [out] of the packed array -> [in][outp], b [outp] at dst.
  __device__ static void stage_hidden(double* dst, const double* __restrict__ src, int in, int out, int lane) {
    const int outp = round_up(out, kUnits);
    for (int i = lane; i < in * outp; i += kEpisodes) {
      const int k = i / outp, j = i - k * outp;
      dst[i] = j < out ? src[j * in + k] : 0.0;
    }
    for (int j = lane; j < outp; j += kEpisodes) dst[in * outp + j] = j < out ? src[out * in + j] : 0.0;
  }

  __device__ void stage(double* lds, int sd, int lane) const {
    const Layout y = layout(sd);
    const double* src = packed;
    int last = sd;
    if (nl >= 1) {
      stage_hidden(lds + y.l0, src, sd, h0, lane);
      src += sd * h0 + h0;
      last = h0;
    }
    if (nl == 2) {
      stage_hidden(lds + y.l1, src, h0, h1, lane);
      src += h0 * h1 + h1;
      last = h1;
    }
    for (int k = lane; k < last + 1; k += kEpisodes) lds[y.out + k] = src[k];     // the row and its bias
  }

  __device__ double activate(double z) const {
    if (act == BSIG_SIM_ACT_RELU) return z < 0.0 ? 0.0 : z;      // (a NaN compares false: it passes)
    if (act == BSIG_SIM_ACT_TANH) return tanh(z);
    return z;
  }

  // pi(o): the observation o [sd] in registers, the staged policy at lds.
  template <int sd>
  __device__ double eval(const double* o, double* lds, int lane) const {
#pragma clang fp contract(off)
    const Layout y = layout(sd);
    const double* wo = lds + y.out;
    if (nl == 0) {
      double z = wo[sd];
#pragma unroll
      for (int k = 0; k < sd; ++k) z = z + wo[k] * o[k];
      return z;
    }
    const int h0p = round_up(h0, kUnits);
    const double* w0 = lds + y.l0;
    const double* b0 = w0 + sd * h0p;
    if (nl == 1) {
      double out = wo[h0];
      for (int j0 = 0; j0 < h0; j0 += kUnits) {
        double z[kUnits];
#pragma unroll
        for (int u = 0; u < kUnits; ++u) z[u] = b0[j0 + u];
#pragma unroll
        for (int k = 0; k < sd; ++k) {
#pragma unroll
          for (int u = 0; u < kUnits; ++u) z[u] = z[u] + w0[k * h0p + j0 + u] * o[k];
        }
#pragma unroll
        for (int u = 0; u < kUnits; ++u) {
          if (j0 + u < h0) out = out + wo[j0 + u] * activate(z[u]);
        }
      }
      return out;
    }
    // two hidden layers: the first into LDS [unit][lane] (its padding too: zeros, never read), the second
    // consumed by the output as it is formed
    double* hid = lds + y.hid + lane;
    for (int j0 = 0; j0 < h0; j0 += kUnits) {
      double z[kUnits];
#pragma unroll
      for (int u = 0; u < kUnits; ++u) z[u] = b0[j0 + u];
#pragma unroll
      for (int k = 0; k < sd; ++k) {
#pragma unroll
        for (int u = 0; u < kUnits; ++u) z[u] = z[u] + w0[k * h0p + j0 + u] * o[k];
      }
#pragma unroll
      for (int u = 0; u < kUnits; ++u) hid[(j0 + u) * kEpisodes] = activate(z[u]);
    }
    const int h1p = round_up(h1, kUnits);
    const double* w1 = lds + y.l1;
    const double* b1 = w1 + h0 * h1p;
    double out = wo[h1];
    for (int j0 = 0; j0 < h1; j0 += kUnits) {
      double z[kUnits];
#pragma unroll
      for (int u = 0; u < kUnits; ++u) z[u] = b1[j0 + u];
      for (int k = 0; k < h0; ++k) {
        const double x = hid[k * kEpisodes];
#pragma unroll
        for (int u = 0; u < kUnits; ++u) z[u] = z[u] + w1[k * h1p + j0 + u] * x;
      }
#pragma unroll
      for (int u = 0; u < kUnits; ++u) {
        if (j0 + u < h1) out = out + wo[j0 + u] * activate(z[u]);
      }
    }
    return out;
  }
};

// The entry point of either type: bsig_sim_rollout's checks and the policy's, the LDS the widths ask for.
template <typename T>
int run_policy(const char* what, int task, const T* params, const T* init, const T* actions,
               const uint8_t* replace, const double* policy, int n_hidden, int h0, int h1, int activation,
               T* states, T* actions_out, int32_t* lengths, int64_t n, int steps, int ta, int terminate,
               int32_t* nonfinite, bsig_stream_t stream) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(policy, "%s: null policy", what);
  BSIG_REQUIRE(n_hidden >= 0 && n_hidden <= BSIG_SIM_POLICY_MAX_HIDDEN, "%s: n_hidden %d outside 0..%d", what,
               n_hidden, BSIG_SIM_POLICY_MAX_HIDDEN);
  BSIG_REQUIRE(n_hidden < 1 || (h0 >= 1 && h0 <= BSIG_SIM_POLICY_MAX_WIDTH), "%s: h0 %d outside 1..%d", what, h0,
               BSIG_SIM_POLICY_MAX_WIDTH);
  BSIG_REQUIRE(n_hidden < 2 || (h1 >= 1 && h1 <= BSIG_SIM_POLICY_MAX_WIDTH), "%s: h1 %d outside 1..%d", what, h1,
               BSIG_SIM_POLICY_MAX_WIDTH);
  BSIG_REQUIRE(activation == BSIG_SIM_ACT_IDENTITY || activation == BSIG_SIM_ACT_RELU ||
                   activation == BSIG_SIM_ACT_TANH,
               "%s: unknown activation %d", what, activation);
  MlpPolicy pol;
  pol.packed = policy;
  pol.replace = replace;
  pol.nl = n_hidden;
  pol.h0 = n_hidden >= 1 ? h0 : 0;
  pol.h1 = n_hidden == 2 ? h1 : 0;
  pol.act = activation;
  return run<T, MlpPolicy>(what, task, params, init, actions, states, actions_out, lengths, n, steps, ta,
                           terminate, nonfinite, stream, pol);
}

}  // namespace sim
}  // namespace bsig
