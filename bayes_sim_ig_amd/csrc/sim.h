// The rollouts of include/bsig_sim.h with fp32 data (csrc/sim.hip) and with double data
// (csrc/f64/sim_f64.hip) from this one template: T is the type of the inputs and outputs only, the state and
// every operation of a step are double in both, so the fp32 outputs are the double ones rounded once.
//
// A workgroup is ONE wavefront: thread e carries episode base + e through its steps, a serial chain a double
// sine and cosine deep.  32 000 episodes are then 500 workgroups, two for most of the 256 CUs; a 256-thread
// workgroup would leave half of them without a wavefront.  At most BSIG_SIM_GRID_CAP workgroups stride over
// the episodes.
// The state indices 0..T are walked in blocks of kBlock.  Per block, a barrier between each phase:
//   1. the block's actions (index min(t, T - 1, Ta - 1)) come into lds_a [e][j], consecutive lanes on
//      consecutive addresses of an episode's run;
//   2. every thread walks its episode: it records its observation into lds_s [e][j][c], then steps with
//      lds_a[e][j]; an ended episode records the held observation again and overwrites lds_a[e][j] with the
//      held action instead.  No barrier inside: the walk is the thread's own;
//   3. lds_s and lds_a go out: an episode's run of nb * sd (nb) contiguous elements at a time, consecutive
//      lanes on consecutive addresses, in 16-byte pieces where every run of the launch starts and ends on
//      one (the host decides that from the pointers and the row's bytes; it holds for CartPole's states
//      always, for Pendulum's when (T + 1) * 3 elements are a multiple of 16 bytes), else by elements.
// An LDS row is padded by 16 bytes: it stays aligned for the 16-byte reads of phase 3, and the threads of
// phase 2, a row apart, spread over the banks four at a time instead of meeting on one.
// Nothing here depends on an episode's end but that episode's own thread: the barriers and the loops' trip
// counts are functions of n and T alone.
//
// Policy is the kernel's third parameter.  NoPolicy (bsig_sim_rollout*) is the open-loop launch: every policy
// line below is behind `if constexpr (Policy::kOn)`, so those instantiations hold nothing of it.  With
// MlpPolicy (csrc/sim_policy.h, include/bsig_sim_policy.h) the workgroup stages the weights in the dynamic LDS
// once, phase 1 brings the block's replace marks in beside the exploration terms, and in phase 2 the thread
// keeps its observation in double (before any rounding to T), forms a_t from it, steps with that double and
// records its rounding in lds_a[e][j].
//
// Draws is the fourth parameter.  NoDraws is every launch above: each draw line below is behind
// `if constexpr (Draws::kOn)`.  With EpisodeDraws (csrc/sim_draws.h, include/bsig_sim_draws.h) phase 1 goes away
// -- the launch reads no [N, Ta] array: the thread makes theta and the initial state of its own episode before
// step 0 (they leave through lds_s and lds_a, an episode's run at a time), and e_t and r_t at step t, in
// registers; the recordings of a block are staged in lds_e and lds_m beside lds_a and leave the same way.
#pragma once
#include <climits>
#include <cmath>

#include "../../include/bsig_sim.h"
#include "common.h"

namespace bsig {
namespace sim {

constexpr int kEpisodes = BSIG_SIM_EPISODES;
constexpr int kBlock = BSIG_SIM_STEP_BLOCK;
static_assert(kEpisodes == kWave, "a workgroup is one wavefront");

struct alignas(16) Piece { uint32_t w[4]; };

// (a comparison with a NaN is false: it passes through, as numpy.clip passes it)
__device__ inline double clip(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// The tasks: the episode's parameters and internal state, one step, the observation, the end condition.
// Every line of step() is the header's, one rounding an operation: no contraction.
struct Pendulum {
  static constexpr int pd = 2, id = 2, sd = 3;
  double th, thdot, k_sin, k_u;
  template <typename T>
  __device__ void load(const T* p, const T* s0) {
#pragma clang fp contract(off)
    const double l = (double)p[0], m = (double)p[1];
    k_sin = -30.0 / (2.0 * l);        // -3 g / (2 l)
    k_u = 3.0 / (m * (l * l));
    th = (double)s0[0];
    thdot = (double)s0[1];
  }
  __device__ void step(double a) {
#pragma clang fp contract(off)
    const double u = clip(2.0 * a, -2.0, 2.0);
    const double w = thdot + (k_sin * sin(th + 3.141592653589793) + k_u * u) * 0.05;
    th = th + w * 0.05;
    thdot = clip(w, -8.0, 8.0);
  }
  __device__ void observe(double* o) const {
    double s, c;
    sincos(th, &s, &c);
    o[0] = c;
    o[1] = s;
    o[2] = thdot;
  }
  __device__ bool ended() const { return false; }
};

struct CartPole {
  static constexpr int pd = 3, id = 4, sd = 4;
  double x, xdot, th, thdot, mp, l, mt, mpl;
  template <typename T>
  __device__ void load(const T* p, const T* s0) {
#pragma clang fp contract(off)
    mp = (double)p[0];
    l = (double)p[1];
    mt = mp + (double)p[2];
    mpl = mp * l;
    x = (double)s0[0];
    xdot = (double)s0[1];
    th = (double)s0[2];
    thdot = (double)s0[3];
  }
  __device__ void step(double a) {
#pragma clang fp contract(off)
    const double force = 10.0 * clip(a, -1.0, 1.0);
    double s, c;
    sincos(th, &s, &c);
    const double tmp = (force + (mpl * (thdot * thdot)) * s) / mt;
    const double tha = (9.8 * s - c * tmp) / (l * (4.0 / 3.0 - (mp * (c * c)) / mt));
    const double xa = tmp - ((mpl * tha) * c) / mt;
    const double x1 = x + 0.02 * xdot, xdot1 = xdot + 0.02 * xa;
    const double th1 = th + 0.02 * thdot, thdot1 = thdot + 0.02 * tha;
    x = x1;
    xdot = xdot1;
    th = th1;
    thdot = thdot1;
  }
  __device__ void observe(double* o) const {
    o[0] = x;
    o[1] = xdot;
    o[2] = th;
    o[3] = thdot;
  }
  __device__ bool ended() const {
    constexpr double th_limit = 12.0 * 2.0 * 3.141592653589793 / 360.0;
    return fabs(x) > 2.4 || fabs(th) > th_limit;
  }
};

// lds rows [ne][row] -> an episode's run of `run` elements at dst + (base + e) * pitch: by 16-byte pieces
// (`vec`: every run starts and ends on one) or by elements.
template <typename T>
__device__ inline void write_runs(T* __restrict__ dst, const T* lds, int row, int64_t base, int64_t pitch, int ne,
                                  int run, bool vec, int lane) {
  constexpr int per = 16 / (int)sizeof(T);
  if (vec) {
    const int q = run / per;
    for (int i = lane; i < ne * q; i += kEpisodes) {
      const int e = i / q, c = i - e * q;
      *reinterpret_cast<Piece*>(dst + (base + e) * pitch + c * per) =
          *reinterpret_cast<const Piece*>(lds + e * row + c * per);
    }
  } else {
    for (int i = lane; i < ne * run; i += kEpisodes) {
      const int e = i / run, c = i - e * run;
      dst[(base + e) * pitch + c] = lds[e * row + c];
    }
  }
}

// The open-loop launch: no policy.
struct NoPolicy {
  static constexpr bool kOn = false;
  __host__ __device__ int lds_bytes(int) const { return 0; }
};

// Every launch whose numbers are the caller's: no draws.
struct NoDraws {
  static constexpr bool kOn = false;
};

template <typename T, typename Task, typename Policy = NoPolicy, typename Draws = NoDraws>
__global__ __launch_bounds__(kEpisodes) void rollout_kernel(const T* __restrict__ params,
                                                            const T* __restrict__ init,
                                                            const T* __restrict__ actions, T* __restrict__ states,
                                                            T* __restrict__ actions_out,
                                                            int32_t* __restrict__ lengths, int64_t n, int steps,
                                                            int ta, int terminate, int vec_s, int vec_a,
                                                            int32_t* __restrict__ nonfinite, Policy pol,
                                                            Draws drw) {
  constexpr int sd = Task::sd;
  constexpr int per = 16 / (int)sizeof(T);
  constexpr int row_s = kBlock * sd + per, row_a = kBlock + per;
  __shared__ __attribute__((aligned(16))) T lds_s[kEpisodes * row_s];
  __shared__ __attribute__((aligned(16))) T lds_a[kEpisodes * row_a];
  const int lane = threadIdx.x;
  const int ts = steps + 1;
  [[maybe_unused]] double* pol_lds = nullptr;       // the staged policy, and the block's replace marks [e][j]
  [[maybe_unused]] uint8_t* lds_r = nullptr;
  if constexpr (Policy::kOn) {
    extern __shared__ __attribute__((aligned(16))) double sim_policy_smem[];
    pol_lds = sim_policy_smem;
    lds_r = reinterpret_cast<uint8_t*>(sim_policy_smem + pol.layout(sd).marks);
    pol.stage(pol_lds, sd, lane);                   // (the first barrier below orders it before its use)
  }
  [[maybe_unused]] T* lds_e = nullptr;              // the block's recordings: e_t [e][j] and r_t [e][j]
  [[maybe_unused]] uint8_t* lds_m = nullptr;
  if constexpr (Draws::kOn) {
    __shared__ __attribute__((aligned(16))) T sim_draws_e[kEpisodes * row_a];
    __shared__ __attribute__((aligned(16))) uint8_t sim_draws_m[kEpisodes * kBlock];
    lds_e = sim_draws_e;
    lds_m = sim_draws_m;
  }

  for (int64_t base = (int64_t)blockIdx.x * kEpisodes; base < n; base += (int64_t)gridDim.x * kEpisodes) {
    const int ne = (int)(n - base < kEpisodes ? n - base : kEpisodes);
    const bool active = lane < ne;
    Task task;
    T obs[sd];
    bool ended = false, bad = false;
    int len = ts;
    T held = (T)0;
    [[maybe_unused]] double od[Policy::kOn ? sd : 1];     // the observation unrounded: the policy's input
    [[maybe_unused]] uint64_t g = 0;                      // the episode's global index: its draws' counter
    if constexpr (Draws::kOn) __syncthreads();            // the batch before has left the LDS
    if (active) {
      if constexpr (Draws::kOn) {
        g = drw.first + (uint64_t)(base + lane);
        T p[Task::pd], s0[Task::id];
        drw.template episode<Task::pd, Task::id>(g, params, init, base + lane, p, s0);
        task.load(p, s0);
#pragma unroll
        for (int c = 0; c < Task::pd; ++c) lds_s[lane * row_s + c] = p[c];
#pragma unroll
        for (int c = 0; c < Task::id; ++c) lds_a[lane * row_a + c] = s0[c];
      } else {
        task.load(params + (base + lane) * Task::pd, init + (base + lane) * Task::id);
      }
      double o[sd];
      task.observe(o);
#pragma unroll
      for (int c = 0; c < sd; ++c) {
        obs[c] = (T)o[c];
        bad |= !isfinite(obs[c]);
        if constexpr (Policy::kOn) od[c] = o[c];
      }
    }
    if constexpr (Draws::kOn) {       // what the episodes run with: a row of pd and of id elements each
      static_assert(Task::pd <= row_s && Task::id <= row_a, "theta and the initial state fit the staging rows");
      __syncthreads();
      write_runs(drw.params_out, lds_s, row_s, base, (int64_t)Task::pd, ne, Task::pd, false, lane);
      write_runs(drw.init_out, lds_a, row_a, base, (int64_t)Task::id, ne, Task::id, false, lane);
    }
    for (int t0 = 0; t0 < ts; t0 += kBlock) {
      const int nb = ts - t0 < kBlock ? ts - t0 : kBlock;
      __syncthreads();          // the block before has left the LDS
      if constexpr (!Draws::kOn) {
        for (int i = lane; i < ne * nb; i += kEpisodes) {
          const int e = i / nb, j = i - e * nb;
          const int t = min(min(t0 + j, steps - 1), ta - 1);
          lds_a[e * row_a + j] = actions[(base + e) * ta + t];
          if constexpr (Policy::kOn) lds_r[e * kBlock + j] = pol.replace ? pol.replace[(base + e) * ta + t] : 0;
        }
        __syncthreads();
      }
      if (active) {
        T* ms = lds_s + lane * row_s;
        T* ma = lds_a + lane * row_a;
        for (int j = 0; j < nb; ++j) {
#pragma unroll
          for (int c = 0; c < sd; ++c) ms[j * sd + c] = obs[c];
          if (ended) {
            ma[j] = held;
            if constexpr (Draws::kOn) {                   // an ended episode draws nothing more
              lds_e[lane * row_a + j] = (T)0;
              lds_m[lane * kBlock + j] = 0;
            }
          } else if (t0 + j < steps) {
            T a;
            [[maybe_unused]] bool mark = false;
            if constexpr (Draws::kOn) {
              a = drw.template step<Policy::kOn>(g, t0 + j, &mark);      // e_t (v_t without a policy) and r_t
              lds_e[lane * row_a + j] = a;
              lds_m[lane * kBlock + j] = mark;
            } else {
              a = ma[j];
            }
            if constexpr (Policy::kOn) {
              double av = (double)a;                      // e_t; a_t = e_t where replaced, else pi(o_t) + e_t
              if constexpr (!Draws::kOn) mark = lds_r[lane * kBlock + j];
              if (!mark) av = pol.template eval<sd>(od, pol_lds, lane) + av;
              a = (T)av;
              ma[j] = a;
              held = a;                                   // (state T repeats it: what was loaded there is e)
              task.step(av);
            } else {
              if constexpr (Draws::kOn) {
                ma[j] = a;
                held = a;                                 // (state T repeats it: nothing was loaded there)
              }
              task.step((double)a);
            }
            double o[sd];
            task.observe(o);
#pragma unroll
            for (int c = 0; c < sd; ++c) {
              obs[c] = (T)o[c];
              bad |= !isfinite(obs[c]);
              if constexpr (Policy::kOn) od[c] = o[c];
            }
            if (terminate && task.ended()) {
              ended = true;
              len = t0 + j + 2;       // the state just formed is the last valid one
              held = a;
            }
          } else if constexpr (Policy::kOn || Draws::kOn) {
            ma[j] = held;             // state T of an episode that runs on: the action of step T - 1
          }
        }
      }
      __syncthreads();
      write_runs(states + (int64_t)t0 * sd, lds_s, row_s, base, (int64_t)ts * sd, ne, nb * sd,
                 vec_s && (nb * sd) % per == 0, lane);
      write_runs(actions_out + t0, lds_a, row_a, base, (int64_t)ts, ne, nb, vec_a && nb % per == 0, lane);
      if constexpr (Draws::kOn) {       // the recordings hold T steps, not T + 1 states
        const int nbe = steps - t0 < nb ? steps - t0 : nb;
        if (drw.explore_out && nbe > 0) {
          write_runs(drw.explore_out + t0, lds_e, row_a, base, (int64_t)steps, ne, nbe,
                     drw.vec_e && nbe % per == 0, lane);
        }
        if (drw.replace_out && nbe > 0) {
          write_runs(drw.replace_out + t0, lds_m, kBlock, base, (int64_t)steps, ne, nbe, false, lane);
        }
      }
    }
    if (active) {
      lengths[base + lane] = len;
      if (bad && nonfinite) atomicOr(nonfinite, 1);
    }
  }
}

inline int dims(int task, int* pd, int* id, int* sd) {
  BSIG_REQUIRE(task == BSIG_SIM_PENDULUM || task == BSIG_SIM_CARTPOLE, "sim_dims: unknown task %d", task);
  const bool pend = task == BSIG_SIM_PENDULUM;
  if (pd) *pd = pend ? Pendulum::pd : CartPole::pd;
  if (id) *id = pend ? Pendulum::id : CartPole::id;
  if (sd) *sd = pend ? Pendulum::sd : CartPole::sd;
  return BSIG_OK;
}

// The entry point of either type: the argument checks, which runs go out in 16-byte pieces, the launch.
template <typename T, typename Policy = NoPolicy, typename Draws = NoDraws>
int run(const char* what, int task, const T* params, const T* init, const T* actions, T* states, T* actions_out,
        int32_t* lengths, int64_t n, int steps, int ta, int terminate, int32_t* nonfinite, bsig_stream_t stream,
        Policy pol = Policy(), Draws drw = Draws()) {
  if (n == 0) return BSIG_OK;
  BSIG_REQUIRE(n > 0, "%s: bad n=%lld", what, (long long)n);
  BSIG_REQUIRE(task == BSIG_SIM_PENDULUM || task == BSIG_SIM_CARTPOLE, "%s: unknown task %d", what, task);
  BSIG_REQUIRE(steps >= 1 && steps < INT_MAX / 8, "%s: T %d outside 1..%d", what, steps, INT_MAX / 8 - 1);
  BSIG_REQUIRE(ta >= 1, "%s: Ta %d below 1", what, ta);
  BSIG_REQUIRE(terminate == 0 || terminate == 1, "%s: terminate %d is not 0 or 1", what, terminate);
  if constexpr (!Draws::kOn) {      // (run_drawn has checked its own pointers, each by name)
    BSIG_REQUIRE(params && init && actions && states && actions_out && lengths, "%s: null pointer", what);
  }
  const int sd = task == BSIG_SIM_PENDULUM ? Pendulum::sd : CartPole::sd;
  const int64_t ts = (int64_t)steps + 1;
  const int vec_s = aligned(states, 16) && (ts * sd * (int64_t)sizeof(T)) % 16 == 0;
  const int vec_a = aligned(actions_out, 16) && (ts * (int64_t)sizeof(T)) % 16 == 0;
  const dim3 grid(capped_grid(ceil_div<int64_t>(n, kEpisodes), BSIG_SIM_GRID_CAP)), block(kEpisodes);
  // (the dynamic LDS is the policy's alone: none without one)
  const size_t lds = (size_t)pol.lds_bytes(sd);
  if constexpr (Policy::kOn) {
    if (lds > kLdsUnraised) {
      static LdsRaised raised[2];
      if (task == BSIG_SIM_PENDULUM) {
        BSIG_TRY(raise_lds_limit(rollout_kernel<T, Pendulum, Policy, Draws>, Policy::kMaxLdsBytes, &raised[0]));
      } else {
        BSIG_TRY(raise_lds_limit(rollout_kernel<T, CartPole, Policy, Draws>, Policy::kMaxLdsBytes, &raised[1]));
      }
    }
  }
  if (task == BSIG_SIM_PENDULUM) {
    hipLaunchKernelGGL((rollout_kernel<T, Pendulum, Policy, Draws>), grid, block, lds, as_stream(stream), params,
                       init, actions, states, actions_out, lengths, n, steps, ta, terminate, vec_s, vec_a,
                       nonfinite, pol, drw);
  } else {
    hipLaunchKernelGGL((rollout_kernel<T, CartPole, Policy, Draws>), grid, block, lds, as_stream(stream), params,
                       init, actions, states, actions_out, lengths, n, steps, ta, terminate, vec_s, vec_a,
                       nonfinite, pol, drw);
  }
  BSIG_CHECK_LAUNCH(what);
  return BSIG_OK;
}

}  // namespace sim
}  // namespace bsig
