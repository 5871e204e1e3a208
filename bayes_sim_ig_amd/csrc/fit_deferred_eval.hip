// Held-out evaluations BEHIND the persistent update launch of the linear heads (fit_persistent.hip, SNAP
// instantiation): the launch leaves a snapshot of every weight tile (and of the biases) at each evaluation
// point; these ordinary, grid-sized kernels -- no workgroup waits for another -- evaluate from the snapshots,
// on the same stream, directly behind the launch.  An evaluation is forward-only and feeds nothing back into
// the weights: inside the launch it sat on the update chain (every update next to one was ~8 us longer).
//
// The arithmetic is the in-launch evaluation's, function for function (persist_linear_device.h), in the same
// thread layout, so the logs are the same bits:
//   products  one workgroup per (evaluation, tile slot): snapshot tile -> LDS, u_eval_products -> the
//             evaluation's buffer of partial products [pass][k_slice][B][NhP];
//   rows      one workgroup per (evaluation, evaluation owner): u_eval_rows -> the owner's row sums and its
//             sum of exp over the sigma columns;
//   nll       one workgroup per (evaluation, owner): the cross-owner sum of the exp sums in slot order
//             (granule_slot_sum), u_eval_nll -> the owner's sum of log-likelihoods;
//   log       one wavefront, the evaluations in order: cross-owner sum in slot order, u_eval_log.
// The cross-owner sums that are granule gathers inside the launch are kernel boundaries here.  The evaluations
// of a launch run in groups, so that the partial products stay bounded (kDeferredGroupBytes).  A launch that
// gave up (time-out bit in the flag word) leaves snapshots nobody may read: every kernel returns at once.
#include "persist.h"

#include <algorithm>
#include <cstdlib>

#include "persist_linear_device.h"

namespace bsig {

// A group of evaluations e0 .. e0 + n of the launch and its buffers (entry y of the group: blockIdx.y)
struct DArgs {
  int e0, n_ev_chunk;                // first evaluation of the launch in the group; evaluations per chunk
  float* slabs; int64_t slab_stride; // [group][eval_passes][k_slices][B][NhP]
  float* rows; int row_floats;       // [group][NE][RE * per_wave]  the owners' row sums
  float* sx; float* sl;              // [group][NE] sum exp / sum of log-likelihoods per owner
};

// evaluation `gidx` of the launch: of which chunk, and which of that chunk's
__device__ __forceinline__ UEval d_eval_of(const UArgs& p, const DArgs& d, int gidx) {
  const int c = p.chunks ? gidx / d.n_ev_chunk : 0;
  return u_eval_of(p, c, gidx - c * d.n_ev_chunk);
}
__device__ __forceinline__ bool d_gave_up(const UArgs& p) {
  return (__hip_atomic_load(p.state + ST_FLAGS, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & kFlagTimeout) != 0;
}
// sum of vals[0 .. n) in the order a granule gather sums slots (whole wavefront)
__device__ __forceinline__ float d_slot_sum(const float* vals, int n, int lane) {
  float v[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) v[u] = lane + 64 * u < n ? vals[lane + 64 * u] : 0.f;
  return granule_slot_sum(v);
}

template <int NT>
__global__ __launch_bounds__(kUT) void deferred_eval_products_kernel(UArgs p, DArgs d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
#ifndef BSIG_HOST_SAN_BUILD
  if (d_gave_up(p)) return;
  constexpr int NBW = 16 * NT;
  float* Wl = smem;                            // [NBW][WP]
  float* biasl = Wl + NBW * p.WP;              // [NBW]
  const int tid = threadIdx.x;
  const int slot = blockIdx.x, gidx = d.e0 + blockIdx.y;
  const int ks = slot / p.n_blocks, nb = slot - ks * p.n_blocks;
  const float* src = p.snap + ((int64_t)gidx * p.G + slot) * u_snap_slot_floats(NT, p.WP);
  const int quads = NBW * p.WP / 4 + (ks == 0 ? NBW / 4 : 0);      // (the biases lie behind the tile, here and there)
  for (int i = tid; i < quads; i += kUT)
    *reinterpret_cast<f32x4*>(Wl + 4 * i) = *reinterpret_cast<const f32x4*>(src + 4 * i);
  __syncthreads();
  u_eval_products<NT>(p, Wl, biasl, ks, nb * NBW, ks * p.KS, d_eval_of(p, d, gidx), d.slabs + blockIdx.y * d.slab_stride);
#endif
}

__global__ __launch_bounds__(kUT) void deferred_eval_rows_kernel(UArgs p, DArgs d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
#ifndef BSIG_HOST_SAN_BUILD
  if (d_gave_up(p)) return;
  float* XS = smem;                            // [RE][per_wave]
  float* red = XS + d.row_floats;              // [64]
  const int tid = threadIdx.x;
  const int eo = blockIdx.x, y = blockIdx.y;
  for (int i = tid; i < d.row_floats; i += kUT) XS[i] = 0.f;
  __syncthreads();
  const float sx = u_eval_rows(p, d.slabs + y * d.slab_stride, XS, red, eo, d_eval_of(p, d, d.e0 + y), tid);
  if (tid == 0) d.sx[y * p.NE + eo] = sx;
  float* out = d.rows + ((int64_t)y * p.NE + eo) * d.row_floats;
  for (int i = tid; i < d.row_floats; i += kUT) out[i] = XS[i];
#endif
}

__global__ __launch_bounds__(kUT) void deferred_eval_nll_kernel(UArgs p, DArgs d) {
  extern __shared__ __attribute__((aligned(16))) float smem[];
#ifndef BSIG_HOST_SAN_BUILD
  if (d_gave_up(p)) return;
  float* XS = smem;
  float* red = XS + d.row_floats;
  const int tid = threadIdx.x, lane = tid & 63;
  const int eo = blockIdx.x, y = blockIdx.y;
  const float* in = d.rows + ((int64_t)y * p.NE + eo) * d.row_floats;
  for (int i = tid; i < d.row_floats; i += kUT) XS[i] = in[i];
  __syncthreads();
  bool bad;
  const float sl = u_eval_nll(p, XS, red, eo, d_eval_of(p, d, d.e0 + y), u_head_args(p), tid,
                              [&] { return d_slot_sum(d.sx + y * p.NE, p.NE, lane); }, bad);
  if (tid == 0) d.sl[y * p.NE + eo] = sl;
  if (bad) atomicOr(p.state + ST_FLAGS, kFlagNonfinite);
#endif
}

// (one wavefront: a one-chunk call's evaluations take the log slots in order, from the state block's counter)
__global__ __launch_bounds__(64) void deferred_eval_log_kernel(UArgs p, DArgs d, int n) {
#ifndef BSIG_HOST_SAN_BUILD
  if (d_gave_up(p)) return;
  const int lane = threadIdx.x;
  for (int y = 0; y < n; ++y) {
    const float sum = d_slot_sum(d.sl + y * p.NE, p.NE, lane);
    if (lane == 0) u_eval_log(p, d_eval_of(p, d, d.e0 + y), sum, p.state + ST_FLAGS);
  }
#endif
}

// ---------------------------------------------------------------- host side
namespace {
struct DLayout { size_t snap_off, snap_bytes, slab_off, rows_off, sx_off, sl_off, total; int group; size_t slab_stride; int row_floats; };

DLayout d_layout(const UGeom& g, int n_evals) {
  DLayout L{};
  L.snap_off = 256;                            // (the copy of the state block in front)
  L.snap_bytes = round_up<size_t>(deferred_eval_snapshot_bytes(g, n_evals), 256);
  L.slab_stride = (size_t)std::max(g.eval_passes, 1) * g.slab_floats;
  L.group = (int)std::max<size_t>(1, std::min<size_t>({(size_t)n_evals, (size_t)64,
                                                      kDeferredGroupBytes / std::max<size_t>(L.slab_stride * sizeof(float), 1)}));
  L.row_floats = (int)round_up(g.RE * g.per_wave, 4);
  L.slab_off = L.snap_off + L.snap_bytes;
  L.rows_off = L.slab_off + round_up<size_t>((size_t)L.group * L.slab_stride * sizeof(float), 256);
  L.sx_off = L.rows_off + round_up<size_t>((size_t)L.group * g.NE * L.row_floats * sizeof(float), 256);
  L.sl_off = L.sx_off + round_up<size_t>((size_t)L.group * g.NE * sizeof(float), 256);
  L.total = L.sl_off + round_up<size_t>((size_t)L.group * g.NE * sizeof(float), 256);
  return L;
}
}  // namespace

size_t deferred_eval_snapshot_bytes(const UGeom& g, int n_evals) {
  return (size_t)n_evals * g.G * (size_t)u_snap_slot_floats(g.NT, g.WP) * sizeof(float);
}

bool deferred_eval_reserve(const UGeom& g, int n_evals, DeferredEval* d) {
  if (n_evals < 1 || g.eval_passes < 1) return false;
  size_t cap = kDeferredSnapCapBytes;
  if (const char* e = getenv("BSIG_DEFERRED_EVAL_CAP_MB")) cap = (size_t)std::max(atoll(e), 0ll) << 20;
  if (deferred_eval_snapshot_bytes(g, n_evals) > cap) return false;
  if (d->mem && d->n_evals >= n_evals) return true;
  const DLayout L = d_layout(g, n_evals);
  if (d->mem) {      // (a launch with more evaluations than any before: work enqueued on the old block ends first)
    if (hipDeviceSynchronize() != hipSuccess || hipFree(d->mem) != hipSuccess) return false;
    *d = DeferredEval{};
  }
  void* mem = nullptr;
  if (hipMalloc(&mem, L.total) != hipSuccess) {
    (void)hipGetLastError();                   // (no memory: the evaluations stay inside the launch)
    return false;
  }
  d->mem = mem; d->bytes = L.total; d->n_evals = n_evals;
  return true;
}

void deferred_eval_free(DeferredEval* d) {
  if (d->mem) (void)hipFree(d->mem);
  *d = DeferredEval{};
}

int deferred_eval_run(const PersistShape& s, const UGeom& g, const PersistBuffers& b, int n, hipStream_t st) {
  BSIG_REQUIRE(b.deferred && b.do_eval && n >= 1, "deferred evaluations: not a launch with snapshots");
  UArgs p;
  BSIG_TRY(persist_fill_args(s, g, b, n, &p));
  const int n_ev_chunk = (int)count_logging_points(n);
  const int n_evals = n_ev_chunk * (b.chunks ? b.n_chunks : 1);
  const DLayout L = d_layout(g, n_evals);      // (of THIS launch: a block reserved for more is laid out for fewer)
  char* base = reinterpret_cast<char*>(b.deferred);
  DArgs d{};
  d.n_ev_chunk = n_ev_chunk;
  d.slabs = reinterpret_cast<float*>(base + L.slab_off); d.slab_stride = (int64_t)L.slab_stride;
  d.rows = reinterpret_cast<float*>(base + L.rows_off); d.row_floats = L.row_floats;
  d.sx = reinterpret_cast<float*>(base + L.sx_off); d.sl = reinterpret_cast<float*>(base + L.sl_off);
  const size_t lds_tile = (size_t)u_snap_slot_floats(g.NT, g.WP) * sizeof(float);
  const size_t lds_rows = ((size_t)L.row_floats + 64) * sizeof(float);
  BSIG_REQUIRE(lds_tile <= kLdsUnraised && lds_rows <= kLdsUnraised, "deferred evaluations: tile or rows beyond 64 KB of LDS");
  for (int e0 = 0; e0 < n_evals; e0 += L.group) {
    const int ne = std::min(L.group, n_evals - e0);
    d.e0 = e0;
    if (g.NT == 1)
      hipLaunchKernelGGL((deferred_eval_products_kernel<1>), dim3(g.G, ne), dim3(kUT), lds_tile, st, p, d);
    else
      hipLaunchKernelGGL((deferred_eval_products_kernel<2>), dim3(g.G, ne), dim3(kUT), lds_tile, st, p, d);
    BSIG_CHECK_LAUNCH("deferred_eval_products");
    hipLaunchKernelGGL(deferred_eval_rows_kernel, dim3(g.NE, ne), dim3(kUT), lds_rows, st, p, d);
    BSIG_CHECK_LAUNCH("deferred_eval_rows");
    hipLaunchKernelGGL(deferred_eval_nll_kernel, dim3(g.NE, ne), dim3(kUT), lds_rows, st, p, d);
    BSIG_CHECK_LAUNCH("deferred_eval_nll");
    hipLaunchKernelGGL(deferred_eval_log_kernel, dim3(1), dim3(64), 0, st, p, d, ne);
    BSIG_CHECK_LAUNCH("deferred_eval_log");
  }
  return BSIG_OK;
}

}  // namespace bsig
