// fp32 GEMM on the CDNA4 matrix cores (v_mfma_f32_32x32x2_f32: exact fp32
// fma chain at the 157 TFLOP/s vector rate; gfx950 has no xf32/TF32 path) with
// fused epilogues.  Serves every dense contraction of the estimator:
//   RFF projection  x @ (freqs/sigma)^T -> a*[cos|sin]     rff.py:128-132
//   nn.Linear forward / backward of trunk and heads        mdnn.py:68-86,108-119
// C[m,n] = epi( sum_k A(m,k) * B(n,k) ); each operand is either k-contiguous
// (rows of a [rows, K] matrix, optionally gathered by an index vector — the
// minibatch gather of mdnn.py:222 fused into the loader) or k-major
// (the contraction index is the slow dimension: the transposed operands of
// the backward products dW = dY^T X and dX = dY W).
//
// Tiling: BK = 32; block = WM x WN waves, each wave owns TM x TN 32x32 MFMA
// tiles.  LDS images: k-contiguous operands as [rows][BK+4] (ds_read_b128 of
// 4 consecutive k per lane, conflict-free at pitch 36), k-major operands as
// [BK][rows] (ds_read_b32, 32 consecutive rows per half-wave).  Lane l of an
// MFMA supplies row (l & 31) and k-slot (l >> 5); within an 8-wide k group the
// half h = l>>5 takes k = 4h..4h+3, one per MFMA step — the k order is a
// permutation of 0..7, identical for A and B.
// Split-K (gridDim.z) writes fp32 partial slabs and a second kernel reduces
// them in a fixed order and applies the epilogue: bitwise reproducible.
#include <cstdlib>
#include "gemm_kernel.h"
#include "gemm_lean.h"
#include "gemm_split_bf16.h"
#include "../../include/bsig_matmul.h"
#include "gemm_wide.h"

namespace bsig {

__global__ __launch_bounds__(256) void gemm_reduce_kernel(GemmParams p) {
  const int64_t total = (int64_t)p.m * p.n;
  const int64_t slab = p.partial_ld ? p.partial_slab : total;
  float exp_acc = 0.f;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / p.n), col = (int)(e % p.n);
    const int64_t pe = p.partial_ld ? (int64_t)row * p.partial_ld + col : e;   // (pitched slabs: gemm_wide.h)
    float v = 0.f;
    int z = 0;
    for (; z + 16 <= p.splits; z += 16) {   // 16 slab loads in flight, summed in slab order
      float q[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) q[u] = p.partial[(int64_t)(z + u) * slab + pe];
#pragma unroll
      for (int u = 0; u < 16; ++u) v += q[u];
    }
    if (z + 8 <= p.splits) {
      float q[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) q[u] = p.partial[(int64_t)(z + u) * slab + pe];
#pragma unroll
      for (int u = 0; u < 8; ++u) v += q[u];
      z += 8;
    }
    for (; z < p.splits; ++z) v += p.partial[(int64_t)z * slab + pe];
    epilogue_store(p, row, col, v);
    if (p.expsum && p.epilogue == BSIG_EPI_BIAS && col >= p.expsum_col0 &&
        col < p.expsum_col0 + p.expsum_ncols)
      exp_acc += expf(v + p.bias[col]);
  }
  if (p.expsum) {
    __shared__ float red[8];
    const float s = block_sum(exp_acc, red);
    if (threadIdx.x == 0) p.expsum[blockIdx.x] = s;
  }
}

// The same reduction for a fused Adam step (EPI_ADAM: dW slabs -> one optimizer step on the weights),
// four adjacent columns per thread: 16-byte loads of the slabs and of the optimizer state, all in
// flight before the first dependent instruction.  Same arithmetic per element as epilogue_store's
// EPI_ADAM branch (slab order, then the identical expressions): bit-identical to the scalar kernel.
template <bool ADAM>   // (false: BSIG_EPI_NONE, the plain sum -- a data-parallel rank's gradients)
__global__ __launch_bounds__(256) void gemm_reduce_adam4_kernel(GemmParams p) {
  const int n4 = p.n >> 2;
  const int64_t total4 = (int64_t)p.m * n4;
  const int64_t slab = p.partial_ld ? p.partial_slab : (int64_t)p.m * p.n;
  float ss = 0.f, ib = 0.f;
  if constexpr (ADAM) { ss = p.adam_dyn[0]; ib = p.adam_dyn[1]; }
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total4;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / n4), col = (int)(e % n4) * 4;
    const int64_t pe = p.partial_ld ? (int64_t)row * p.partial_ld + col : (int64_t)row * p.n + col;
    const int64_t ce = (int64_t)row * p.ldc + col;
    F4 g{{0.f, 0.f, 0.f, 0.f}};
    F4 pm{{0.f, 0.f, 0.f, 0.f}}, pv = pm, pp = pm;
    if constexpr (ADAM) { pm = ld4(p.adam_m + ce); pv = ld4(p.adam_v + ce); pp = ld4(p.c + ce); }
    int z = 0;
    for (; z + 4 <= p.splits; z += 4) {
      F4 q[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) q[u] = ld4(p.partial + (int64_t)(z + u) * slab + pe);
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int c = 0; c < 4; ++c) g.v[c] += q[u].v[c];
    }
    for (; z < p.splits; ++z) {
      const F4 q = ld4(p.partial + (int64_t)z * slab + pe);
#pragma unroll
      for (int c = 0; c < 4; ++c) g.v[c] += q.v[c];
    }
    if constexpr (!ADAM) { st4(p.c + ce, g); continue; }
    if (p.grad_out) st4(p.grad_out + ce, g);
    F4 m1, v1, p1;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      m1.v[c] = pm.v[c] + (g.v[c] - pm.v[c]) * (1.0f - p.beta1);
      v1.v[c] = pv.v[c] * p.beta2 + (1.0f - p.beta2) * g.v[c] * g.v[c];
      p1.v[c] = pp.v[c] - ss * (m1.v[c] / (sqrtf(v1.v[c]) * ib + p.adam_eps));
    }
    st4(p.adam_m + ce, m1); st4(p.adam_v + ce, v1); st4(p.c + ce, p1);
    if (col == 0 && p.bias_p) {
      // (partial sums in index order, 16 loads in flight: one lane of a wavefront does this while the
      // others wait -- a load per iteration made it 64 dependent round trips)
      float bg = 0.f;
      for (int q0 = 0; q0 < max(p.bias_g_n, 1); q0 += 16) {
        float t[16];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          t[u] = p.bias_g[(int64_t)min(q0 + u, max(p.bias_g_n, 1) - 1) * p.bias_g_stride + row];
#pragma unroll
        for (int u = 0; u < 16; ++u)
          if (q0 + u < max(p.bias_g_n, 1)) bg += t[u];
      }
      const float bm = p.bias_m[row] + (bg - p.bias_m[row]) * (1.0f - p.beta1);
      const float bv = p.bias_v[row] * p.beta2 + (1.0f - p.beta2) * bg * bg;
      p.bias_m[row] = bm;
      p.bias_v[row] = bv;
      p.bias_p[row] = p.bias_p[row] - ss * (bm / (sqrtf(bv) * ib + p.adam_eps));
    }
  }
}

// (the reduce of a split product: the 16-byte kernel where it applies)
static int launch_reduce(const GemmParams& p, hipStream_t st, int* n_expsum) {
  const int64_t total = (int64_t)p.m * p.n;
  auto al = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  const bool quads = (p.n & 3) == 0 && (p.ldc & 3) == 0 && (p.partial_ld & 3) == 0 && (p.partial_slab & 3) == 0 &&
                     al(p.partial) && al(p.c) && getenv("BSIG_GEMM_NO_ADAM4") == nullptr;
  const bool adam4 = quads && p.epilogue == EPI_ADAM && al(p.adam_m) && al(p.adam_v) && (!p.grad_out || al(p.grad_out));
  BSIG_REQUIRE(!(p.bias_g_n > 1 && !adam4), "gemm: partial bias sums need the 16-byte reduce + Adam kernel");
  if (adam4 || (quads && p.epilogue == BSIG_EPI_NONE && total >= (1 << 18))) {
    const int blocks = (int)std::min<int64_t>(ceil_div<int64_t>(total / 4, 256), 2048);
    if (adam4) hipLaunchKernelGGL(gemm_reduce_adam4_kernel<true>, dim3(blocks), dim3(256), 0, st, p);
    else hipLaunchKernelGGL(gemm_reduce_adam4_kernel<false>, dim3(blocks), dim3(256), 0, st, p);
    BSIG_CHECK_LAUNCH("gemm_reduce_adam4");
    return BSIG_OK;
  }
  const int blocks = (int)std::min<int64_t>(ceil_div<int64_t>(total, 256), 2048);
  hipLaunchKernelGGL(gemm_reduce_kernel, dim3(blocks), dim3(256), 0, st, p);
  BSIG_CHECK_LAUNCH("gemm_reduce");
  if (n_expsum && p.expsum) *n_expsum = blocks;
  return BSIG_OK;
}

// Debug instantiation (BSIG_DEBUG_F64_ACC_MIN_K=<k>): a product whose contraction is at least <k>
// long is formed by one thread per output element with the products and their sum in fp64, rounded
// to fp32 once -- the value every fp32 summation order of the same operands approximates.  Same
// operand addressing (gathers, k-major operands, device-resolved row offsets), same epilogues and
// side outputs as the MFMA kernel; 100x slower.  SURVEY.md section 7 ("hard parts") asks for it to
// extend the horizon of the ill-conditioned wide first layers (cfg/anymal.yaml: 56 402 terms per
// output, cfg/shadow_hand_more.yaml: 105 002): with it the per-phase path's chunk stays with the
// fp64 chunk where fp32 accumulation orders leave each other
// (tests/test_gpu_fit.py::test_wide_chunk_with_fp64_first_layer_sums_stays_with_fp64).
__global__ __launch_bounds__(256) void gemm_f64acc_kernel(GemmParams p) {
  const int64_t total = (int64_t)p.m * p.n;
  const int64_t dstep = p.dyn ? (int64_t)(p.dyn[0] + p.dyn_delta) : 0;
  const int64_t a_off = dstep * p.a_dyn_stride + p.a_dyn_base, b_off = dstep * p.b_dyn_stride + p.b_dyn_base;
  float exp_acc = 0.f;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int row = (int)(e / p.n), col = (int)(e % p.n);
    // k-contiguous operand: the gathered dimension is its row; k-major: its contraction index
    const int64_t ar = p.a_kmajor ? 0 : (p.a_rows ? p.a_rows[row + a_off] : row + a_off);
    const int64_t br = p.b_kmajor ? 0 : (p.b_rows ? p.b_rows[col + b_off] : col + b_off);
    double acc = 0.0;
    for (int kk = 0; kk < p.k; ++kk) {
      const float av = p.a_kmajor ? p.a[(p.a_rows ? (int64_t)p.a_rows[kk + a_off] : kk + a_off) * p.lda + row]
                                  : p.a[ar * p.lda + kk];
      const float bv = p.b_kmajor ? p.b[(p.b_rows ? (int64_t)p.b_rows[kk + b_off] : kk + b_off) * p.ldb + col]
                                  : p.b[br * p.ldb + kk];
      acc += (double)av * (double)bv;
    }
    const float v = (float)acc;
    epilogue_store(p, row, col, v);
    if (p.expsum && p.epilogue == BSIG_EPI_BIAS && col >= p.expsum_col0 &&
        col < p.expsum_col0 + p.expsum_ncols)
      exp_acc += expf(v + p.bias[col]);
  }
  if (p.expsum) {
    __shared__ float red[8];
    const float s = block_sum(exp_acc, red);
    if (threadIdx.x == 0) p.expsum[blockIdx.x] = s;
  }
}

enum { TILE_64 = 0, TILE_128 = 1, TILE_128x32 = 2, TILE_128x64 = 3, TILE_128x96 = 4,
       TILE_96x128 = 5, TILE_128x288 = 6, TILE_288x128 = 7, N_TILES = 8 };
// One entry per tile shape, indexed by the enum (= BSIG_GEMM_TILE): its launcher of gemm_mfma_kernel (null: not
// in this build) and of gemm_lean_kernel (null: the lean loop is not instantiated for the shape).
struct GemmTile {
  int m, n;
  int (*mfma)(const GemmParams&, bool akm, bool bkm, int avec, int bvec, hipStream_t);
  int (*lean)(const GemmParams&, bool akm, bool bkm, hipStream_t);
};
static const GemmTile kTiles[N_TILES] = {
    {64, 64, launch_tile_64, launch_lean_64},         {128, 128, launch_tile_128, launch_lean_128},
    {128, 32, launch_tile_128x32, launch_lean_128x32}, {128, 64, launch_tile_128x64, launch_lean_128x64},
    {128, 96, launch_tile_128x96, launch_lean_128x96}, {96, 128, launch_tile_96x128, launch_lean_96x128},
#ifdef BSIG_WITH_WIDE_TILES
    {128, 288, launch_tile_128x288, nullptr},          {288, 128, launch_tile_288x128, nullptr},
#else
    {128, 288, nullptr, nullptr},                      {288, 128, nullptr, nullptr},
#endif
};
struct GemmPlan { int tile; int splits; int k_chunk; };

static int env_int(const char* name, int dflt) {
  const char* v = getenv(name);
  return v ? atoi(v) : dflt;
}

// Tile / split-K choice.  Large problems: 128x128 tiles, no split.  Minibatch
// sized M (<= 128 rows): 128x32 tiles so the big operand (weights / RFF
// coefficients) is streamed exactly once, split-K until ~4 workgroups per CU.
// Large-minibatch shapes (the scaled-batch fit: thousands of rows per update, or a
// contraction over thousands of rows): pick the tile with the least padded area -- a
// head of 260 outputs on 128-wide tiles wastes a third of every block -- and split K
// until there are ~3 workgroups per CU: one 256-thread workgroup per CU hides neither
// the global nor the LDS latency (8192 x 260 x 4096 ran at 34 TFLOP/s on 192 unsplit
// 128 x 128 tiles).
static bool plan_gemm_large(int64_t m, int64_t n, int64_t k, size_t ws_bytes, GemmPlan* pl) {
  if (!((m >= 4096 || k >= 4096) && m * n >= ((int64_t)1 << 20) && k >= 1024 && m > 128)) return false;
  static const int cand[] = {TILE_128, TILE_128x96, TILE_96x128, TILE_128x64, TILE_64, TILE_128x288, TILE_288x128};
  // per-flop cost of the tile shape (a whole-width tile streams the long operand once)
  static const double cost[] = {1.00, 1.04, 1.04, 1.15, 1.40, 0.98, 0.98};
  // (measured on the scaled-batch fit, tools/scaled_tile_ab.py / profiles/r03_scaled_tile_ab.txt: the
  // whole-width tiles run the forward product at 0.52 and dW at 0.51-0.58 of the fp32 MFMA peak, no
  // better than the 96-wide ones -- one wavefront per SIMD does not hide the operand latency -- so
  // they stay opt-in: BSIG_GEMM_WIDE_TILE=1)
  // (and they are only in a library built with BSIG_BUILD_WIDE_TILES=1 ./build.sh: each of the two
  // takes 3.5 minutes to compile, longer than the rest of the library together)
#ifdef BSIG_WITH_WIDE_TILES
  const bool wide_ok = env_int("BSIG_GEMM_WIDE_TILE", 0) != 0;
#else
  const bool wide_ok = false;
#endif
  double best = 0.0;
  int best_t = -1;
  int64_t best_tiles = 0;
  for (int i = 0; i < 7; ++i) {
    const int t = cand[i];
    if (!wide_ok && (t == TILE_128x288 || t == TILE_288x128)) continue;
    const int64_t tm = ceil_div<int64_t>(m, kTiles[t].m), tn = ceil_div<int64_t>(n, kTiles[t].n);
    const double padded = (double)(tm * kTiles[t].m) * (double)(tn * kTiles[t].n) * cost[i];
    if (best_t < 0 || padded < best) { best = padded; best_t = t; best_tiles = tm * tn; }
  }
  int64_t splits = 1;
  if (best_t == TILE_128x288 || best_t == TILE_288x128) {
    // 60 KB of LDS and 9 accumulators per wave: at most two workgroups per CU -- one round of 256..512
    splits = std::max<int64_t>(env_int("BSIG_GEMM_WIDE_WGS", 256) / best_tiles, 1);
    splits = std::min<int64_t>(splits, std::max<int64_t>(k / (8 * BK), 1));
  } else if (best_tiles < 640) {
    splits = ceil_div<int64_t>(768, best_tiles);
    splits = std::min<int64_t>(splits, std::max<int64_t>(k / (8 * BK), 1));
    splits = std::min<int64_t>(splits, 32);
  }
  const int64_t max_by_ws = (int64_t)(ws_bytes / (sizeof(float) * (size_t)(m * n)));
  splits = std::max<int64_t>(std::min(splits, max_by_ws), 1);
  const int64_t chunk = round_up<int64_t>(ceil_div<int64_t>(k, splits), BK);
  pl->tile = best_t;
  pl->splits = (int)ceil_div<int64_t>(k, chunk);
  pl->k_chunk = (int)chunk;
  return true;
}

// lean_ok: gemm_lean_kernel will run this product (both operands move as aligned 16-byte items)
static GemmPlan plan_gemm(int64_t m, int64_t n, int64_t k, size_t ws_bytes, bool lean_ok) {
  GemmPlan pl;
  if (env_int("BSIG_GEMM_TILE", -1) < 0 && env_int("BSIG_GEMM_SPLITS", 0) <= 0 &&
      env_int("BSIG_GEMM_NO_LARGE_PLAN", 0) == 0 && plan_gemm_large(m, n, k, ws_bytes, &pl))
    return pl;
  const int64_t t128 = ceil_div<int64_t>(m, 128) * ceil_div<int64_t>(n, 128);
  int64_t tiles, target, min_splits = 1;
  const int64_t t12864 = ceil_div<int64_t>(m, 128) * ceil_div<int64_t>(n, 64);
  if (m >= 256 && n >= 128 && t128 >= 192) {
    pl.tile = TILE_128; tiles = t128; target = 256;
  } else if (m >= 256 && n >= 128 && t12864 >= 160 && t12864 <= 512) {
    // mid-sized (a chunk's RFF projection: 1000 x 2048 x 2310 -- training and held-out rows in one
    // launch).  With the lean loop (two LDS images: four 64 x 64 workgroups per CU) the unsplit 64 x 64
    // tiling is the fastest of the sweep (profiles/r05_rff_chunk_sweep.txt: 1000 rows = 16 x 32 = 512
    // workgroups, two per CU, 90 us against 97 for 128 x 64 tiles in two K halves; 800 rows 95 = 95).
    // (round 2-4, gemm_mfma_kernel: 128x64 tiles in two k-halves, 101-104 us against 118-135.)
    // That measurement holds for the LEAN kernel only: operands that are not 16-byte aligned still run
    // gemm_mfma_kernel, where unsplit 64 x 64 tiles measured 118-135 us against 101-104 for the old plan
    // -- they keep 128 x 64 tiles in two K halves (round-5 advisor finding).
    if (lean_ok) { pl.tile = TILE_64; tiles = ceil_div<int64_t>(m, 64) * ceil_div<int64_t>(n, 64); target = 0; }
    else { pl.tile = TILE_128x64; tiles = t12864; target = 0; min_splits = 2; }
  } else if (m <= 128 && n >= 64) {
    pl.tile = TILE_128x32; tiles = ceil_div<int64_t>(n, 32); target = 512;
  } else {
    pl.tile = TILE_64; tiles = ceil_div<int64_t>(m, 64) * ceil_div<int64_t>(n, 64); target = 512;
  }
  const int forced_tile = env_int("BSIG_GEMM_TILE", -1);
  if (forced_tile >= 0) {
    pl.tile = forced_tile;   // (as given: route_generic refuses one that names no built tile)
    const GemmTile& t = kTiles[forced_tile % N_TILES];
    tiles = ceil_div<int64_t>(m, t.m) * ceil_div<int64_t>(n, t.n);
  }
  int64_t splits = 1;
  if (tiles < target && tiles < 256) {   // fewer workgroups than CUs: split K
    splits = ceil_div<int64_t>(target, tiles);
    const int64_t max_by_k = k / (4 * BK) > 0 ? k / (4 * BK) : 1;   // >= PD K steps per block
    if (splits > max_by_k) splits = max_by_k;
    if (splits > 64) splits = 64;
  }
  if (forced_tile < 0 && splits < min_splits && k / (4 * BK) >= min_splits) splits = min_splits;
  const int forced = env_int("BSIG_GEMM_SPLITS", 0);
  if (forced > 0) splits = forced;
  const int64_t max_by_ws = (int64_t)(ws_bytes / (sizeof(float) * (size_t)(m * n)));
  if (splits > max_by_ws) splits = max_by_ws;
  if (splits < 1) splits = 1;
  // (k = 0, which only bsig_gemm_workspace_bytes brings here: one empty slice, not a division by zero)
  int64_t chunk = std::max<int64_t>(round_up<int64_t>(ceil_div<int64_t>(k, splits), BK), BK);
  splits = std::max<int64_t>(ceil_div<int64_t>(k, chunk), 1);
  pl.splits = (int)splits;
  pl.k_chunk = (int)chunk;
  return pl;
}

// ---- routing: facts -> route -> launch.  What a route depends on, without pointers: gemm_run fills it from
// its operands (gemm_facts), the report bsig_debug_gemm_path from its arguments (gemm_facts_dense).  Wherever
// the two answer differently for one shape, it is those two builders that differ.
struct GemmFacts {
  int64_t m = 0, n = 0, k = 0;
  bool a_kmajor = false, b_kmajor = false;
  int epilogue = BSIG_EPI_NONE, math = 0;
  size_t ws_bytes = 0;        // 0: no workspace
  struct Operand {
    bool vec4 = false;        // moves as aligned 16-byte items (pitch % 4 == 0, storage 16-byte aligned)
    // k-contiguous rows that are not (the cross-correlation widths S*A + 2) and can still move in quads, at any
    // 4-byte address, the row's last one shifted into place
    bool unal = false;
    bool gathered = false, offset = false;   // through an index vector; at a device-resolved row offset
  } a, b;
  bool lda_ceil16 = false;    // lda == ceil16(m): the pitch the whole-width gradient takes dO at
  bool partial_bias = false, expsum = false;   // bias_g_n > 1; the exp side output is asked for
  // the whole-width forward may combine its K slices in the launch: a ticket for every 64-row tile (those beyond
  // the caller's buffer are somebody else's memory -- a head whose width is a multiple of 16 keeps ldc == wide at
  // ANY row count) and c 16-byte aligned at a pitch that holds the padded width
  bool combine_ok = false;
};

struct GemmRoute {
  int path = GEMM_PATH_MFMA;
  int tile = -1, tile_m = 0, tile_n = 0;   // tile: index of kTiles (the generic kernels only)
  int splits = 1, k_chunk = 0;
  int64_t workgroups = 0;
  int64_t slab = 0;                        // the whole-width kernels: floats per K slice of slabs
  bool reduce = false;                     // raw slabs: launch_reduce sums them and applies the epilogue ...
  bool combine = false;                    // ... or the whole-width forward does, inside its launch
  bool a_unal = false, b_unal = false;     // gemm_mfma_kernel fetches the operand in unaligned quads
  int declined = 0;                        // split-bf16 asked for: 1 the kernel does not cover the call, 2 left to fp32 by rule
};

static GemmFacts::Operand operand_facts(const float* ptr, int64_t ld, bool kmajor, int64_t k, bool gathered, bool offset) {
  GemmFacts::Operand o;
  o.vec4 = ld % 4 == 0 && aligned(ptr, 16);
  o.unal = !kmajor && !o.vec4 && ld >= 4 && k >= 4;
  o.gathered = gathered; o.offset = offset;   // (offsets are whole rows: they change the alignment of nothing)
  return o;
}

static GemmFacts gemm_facts(const GemmParams& p, const void* workspace, size_t workspace_bytes) {
  GemmFacts f;
  f.m = p.m; f.n = p.n; f.k = p.k; f.a_kmajor = p.a_kmajor != 0; f.b_kmajor = p.b_kmajor != 0;
  f.epilogue = p.epilogue; f.math = p.math;
  f.ws_bytes = workspace ? workspace_bytes : 0;
  f.a = operand_facts(p.a, p.lda, f.a_kmajor, p.k, p.a_rows != nullptr, p.a_dyn_stride || p.a_dyn_base);
  f.b = operand_facts(p.b, p.ldb, f.b_kmajor, p.k, p.b_rows != nullptr, p.b_dyn_stride || p.b_dyn_base);
  f.lda_ceil16 = p.lda == round_up<int64_t>(p.m, 16);
  f.partial_bias = p.bias_g_n > 1; f.expsum = p.expsum != nullptr;
  f.combine_ok = p.combine_tickets && ceil_div(p.m, 64) <= p.combine_capacity && p.ldc >= round_up(p.n, 16) &&
                 (p.ldc & 3) == 0 && aligned(p.c, 16);
  return f;
}

// The report's operands: dense and 16-byte aligned, A [m, k] or k-major [k, ceil16(m)], B [n, k] or k-major [k, n];
// no unaligned quads, offsets, side output, partial bias sums or tickets.  Its one `gathered` bit speaks for X[ids]
// of the whole-width gradient only (B where both operands are k-major): the forward, which needs B direct, never sees it.
static GemmFacts gemm_facts_dense(int64_t m, int64_t n, int64_t k, bool akm, bool bkm, bool gathered, int epilogue,
                                  size_t ws_bytes, int math) {
  GemmFacts f;
  f.m = m; f.n = n; f.k = k; f.a_kmajor = akm; f.b_kmajor = bkm;
  f.epilogue = epilogue; f.math = math; f.ws_bytes = ws_bytes;
  f.a.vec4 = (akm ? round_up<int64_t>(m, 16) : k) % 4 == 0;
  f.b.vec4 = (bkm ? n : k) % 4 == 0;
  f.b.gathered = gathered && akm && bkm;
  f.lda_ceil16 = true;
  return f;
}

// The one class of shapes the split-bf16 mode leaves on the fp32 kernels (profiles/split_bf16_NOTES.md): the
// two head products of a LARGE minibatch -- a few-hundred-wide head the whole-width kernels are built for,
// against thousands of rows.  Measured at 8192 x 260 x 4096: the split kernel's 64 x 64 tiles spend more
// vector-ALU time on splitting the operands than the whole-width fp32 kernels spend on their MFMAs
// (forward 255 us against 168, gradient 344 against 162).  bsig_debug_gemm_path reports the rule (out[6] = 2).
// (BSIG_SPLIT_BF16_EVERYWHERE=1 switches the rule off: tools/split_bf16_timing.py measures what it rests on)
static bool split_bf16_leaves_to_fp32(const GemmFacts& f) {
  if (env_int("BSIG_SPLIT_BF16_EVERYWHERE", 0)) return false;
  if (!f.a_kmajor && !f.b_kmajor) return f.m >= 4096 && f.k >= 1024 && gemm_wide_covers((int)f.n);
  if (f.a_kmajor && f.b_kmajor) return f.k >= 4096 && f.n >= 1024 && gemm_wide_covers((int)f.m);
  return false;
}

// dW = dO^T X[ids] on the whole-width gradient kernel (the workspace aside: a caller asks before it issues the product)
static bool wide_gradient_rule(const GemmFacts& f) {
  return f.a_kmajor && f.b_kmajor && !f.a.gathered && !f.a.offset && f.b.gathered && f.k >= 2048 && f.k % BK == 0 &&
         gemm_wide_covers((int)f.m) && f.lda_ceil16 && f.n % 64 == 0 && f.a.vec4 && f.b.vec4 && env_int("BSIG_GEMM_WIDE", 1);
}

bool gemm_wide_gradient_applies(int64_t m, int64_t n, int64_t k, int64_t lda, int64_t ldb, const float* a,
                                const float* b, bool gathered) {
  GemmFacts f;
  f.m = m; f.n = n; f.k = k; f.a_kmajor = f.b_kmajor = true;
  f.a = operand_facts(a, lda, true, k, false, false);
  f.b = operand_facts(b, ldb, true, k, gathered, false);
  f.lda_ceil16 = lda == round_up<int64_t>(m, 16);
  return wide_gradient_rule(f);
}

// K slices of a whole-width product of `tiles` narrow tiles into slabs of r->slab floats.  One workgroup per CU at a
// time (123 KB of LDS): the launch takes ceil(tiles * s / 256) rounds of 1 / s of a tile's K loop each, plus a
// slab's worth of traffic per slice -- e.g. 313 row tiles (a 20000-row evaluation): unsplit 2 rounds of the whole
// K loop, in 4 slices 5 rounds of a quarter.  False: the workspace does not hold one slab.
static bool wide_slices(const GemmFacts& f, int64_t tiles, GemmRoute* r) {
  const int64_t smax = std::min<int64_t>(std::min<int64_t>(8, std::max<int64_t>(f.k / (8 * BK), 1)),
                                         (int64_t)(f.ws_bytes / (sizeof(float) * (size_t)r->slab)));
  if (smax < 1) return false;
  int64_t s = 1;
  double best = 1e30;
  for (int64_t c = 1; c <= smax; ++c) {
    const double cost = (double)ceil_div<int64_t>(tiles * c, 256) / (double)c + 0.02 * (double)c;
    if (cost < best - 1e-9) { best = cost; s = c; }
  }
  r->k_chunk = (int)round_up<int64_t>(ceil_div<int64_t>(f.k, s), BK);
  r->splits = (int)ceil_div<int64_t>(f.k, r->k_chunk);
  r->workgroups = tiles * r->splits;
  return true;
}

// The generic kernels: the lean main loop (gemm_lean.h: bit-identical, no vector-ALU work in the K loop) wherever
// both operands move as aligned 16-byte items and the tile has one, gemm_mfma_kernel elsewhere.
static int route_generic(const GemmFacts& f, GemmRoute* r) {
  const int declined = r->declined;
  *r = GemmRoute();   // (whatever a whole-width route that did not come about left in it)
  r->declined = declined;
  BSIG_REQUIRE(f.k >= 1, "gemm: an empty contraction (k = 0) on the fp32 MFMA kernels");
  const bool lean_ok = f.a.vec4 && f.b.vec4;
  // (the plan does not depend on BSIG_GEMM_LEAN: the two kernels are compared on the SAME plan)
  const GemmPlan pl = plan_gemm(f.m, f.n, f.k, f.ws_bytes, lean_ok);
  int built = 0;
  while (built < N_TILES && kTiles[built].mfma) ++built;
  BSIG_REQUIRE(pl.tile >= 0 && pl.tile < built, "gemm: BSIG_GEMM_TILE=%d names no tile of this build (0..%d)",
               pl.tile, built - 1);
  const GemmTile& t = kTiles[pl.tile];
  const bool unal = (f.a.unal || f.b.unal) && getenv("BSIG_GEMM_NO_UNALIGNED") == nullptr;
  r->a_unal = unal && f.a.unal; r->b_unal = unal && f.b.unal;
  const int lean = env_int("BSIG_GEMM_LEAN", 1);   // (read per call: tests compare the two kernels)
  r->path = lean && lean_ok && t.lean ? GEMM_PATH_LEAN : GEMM_PATH_MFMA;
  r->tile = pl.tile; r->tile_m = t.m; r->tile_n = t.n;
  r->splits = pl.splits; r->k_chunk = pl.k_chunk; r->reduce = pl.splits > 1;
  r->workgroups = ceil_div<int64_t>(f.m, t.m) * ceil_div<int64_t>(f.n, t.n) * pl.splits;
  return BSIG_OK;
}

// Which kernel runs a product: host arithmetic on the facts and the environment switches (read per call: tests
// flip them between calls).  gemm_run launches what it says, bsig_debug_gemm_path reports it.
static int gemm_route(const GemmFacts& f, GemmRoute* r) {
  *r = GemmRoute();
  // debug (BSIG_DEBUG_F64_ACC_MIN_K=<k>): a contraction at least <k> long is summed in fp64, gemm_f64acc_kernel
  const int f64_min_k = env_int("BSIG_DEBUG_F64_ACC_MIN_K", 0);
  if (f64_min_k > 0 && f.k >= f64_min_k) {
    r->path = GEMM_PATH_F64ACC; r->k_chunk = (int)f.k;
    r->workgroups = std::min<int64_t>(ceil_div<int64_t>(f.m * f.n, 256), 2048);
    return BSIG_OK;
  }
  // The opt-in matmul precision (include/bsig_matmul.h): the split-bf16 kernel wherever it covers the
  // call -- every operand form; a fused Adam step needs room for its slabs.  No size threshold; one
  // measured class of shapes stays on the fp32 kernels (split_bf16_leaves_to_fp32).
  if (f.math == BSIG_MATMUL_SPLIT_BF16) {
    SplitBf16Plan sp;
    // (an unsplit launch writes one exp partial per workgroup; the reduce at most 2048: a product of more
    // tiles than that with the side output and no K slices -- a head on a narrow trunk over tens of
    // thousands of rows -- keeps the fp32 kernels, whose planner the callers' partial arrays are sized for)
    if (split_bf16_leaves_to_fp32(f)) {
      r->declined = 2;
    } else if (split_bf16_plan(f.m, f.n, f.k, f.epilogue, f.partial_bias, f.ws_bytes, &sp) &&
               !(f.expsum && !sp.slabs && sp.workgroups > 2048)) {
      r->path = GEMM_PATH_SPLIT_BF16; r->tile_m = r->tile_n = sp.tile;
      r->splits = sp.splits; r->k_chunk = sp.k_chunk; r->workgroups = sp.workgroups; r->reduce = sp.slabs != 0;
      return BSIG_OK;
    } else {
      r->declined = 1;
    }
  }
  // Large-minibatch products of a few-hundred-wide head (the scaled-batch update): whole-width tiles
  // of 16x16x4 MFMAs (gemm_wide.h) -- forward O = X[ids] W^T and the gradient dW = dO^T X[ids] with
  // dO at a pitch of ceil16(Nh) floats -- in K slices of slabs, one round of ~256 workgroups.
  if (env_int("BSIG_GEMM_WIDE", 1) && f.ws_bytes > 0 && f.k >= 1024 && f.k % BK == 0) {
    r->reduce = true;
    if (!f.a_kmajor && !f.b_kmajor && !f.b.gathered && !f.b.offset && f.m >= 2048 && gemm_wide_covers((int)f.n) &&
        f.a.vec4 && f.b.vec4 && (f.epilogue == BSIG_EPI_NONE || f.epilogue == BSIG_EPI_BIAS)) {
      r->path = GEMM_PATH_WIDE_FORWARD; r->tile_m = 64; r->tile_n = (int)round_up<int64_t>(f.n, 16);
      r->slab = f.m * r->tile_n;
      if (wide_slices(f, ceil_div<int64_t>(f.m, 64), r)) {
        r->combine = f.combine_ok && f.epilogue == BSIG_EPI_BIAS && r->slab < ((int64_t)1 << 31) &&
                     env_int("BSIG_GEMM_NO_COMBINE", 0) == 0;
        r->reduce = !r->combine;
        return BSIG_OK;
      }
    } else if (wide_gradient_rule(f)) {
      r->path = GEMM_PATH_WIDE_GRADIENT; r->tile_m = (int)round_up<int64_t>(f.m, 16); r->tile_n = 64;
      r->slab = f.m * f.n;
      if (wide_slices(f, f.n / 64, r)) return BSIG_OK;
    }
  }
  return route_generic(f, r);
}

// One launch per path id.  BSIG_EUNSUPPORTED: the launcher hands the call back, nothing was launched (gemm_run).
static int launch_route(GemmParams& p, const GemmFacts& f, const GemmRoute& r, hipStream_t st) {
  static const int xcd = [] { const char* e = getenv("BSIG_GEMM_XCD"); return e ? atoi(e) : 1; }();
  p.xcd_swz = xcd;
  p.splits = r.splits; p.k_chunk = r.k_chunk;
  p.partial_ld = p.partial_slab = 0;
  WideParams wp;
  wp.dyn = p.dyn; wp.dyn_delta = p.dyn_delta; wp.k = p.k; wp.k_chunk = r.k_chunk; wp.splits = r.splits;
  wp.out = p.partial; wp.slab = r.slab;
  switch (r.path) {
    case GEMM_PATH_F64ACC:
      hipLaunchKernelGGL(gemm_f64acc_kernel, dim3((int)r.workgroups), dim3(256), 0, st, p);
      BSIG_CHECK_LAUNCH("gemm_f64acc");
      return BSIG_OK;
    case GEMM_PATH_SPLIT_BF16: {
      SplitBf16Plan sp;
      sp.tile = r.tile_m; sp.splits = r.splits; sp.k_chunk = r.k_chunk; sp.slabs = r.reduce; sp.workgroups = r.workgroups;
      return launch_split_bf16(p, sp, st);
    }
    case GEMM_PATH_WIDE_FORWARD:
      wp.wide = p.b; wp.ld_wide = p.ldb; wp.n_wide = p.n;
      wp.x = p.a; wp.ldx = p.lda; wp.ids = p.a_rows; wp.n_narrow = p.m;
      wp.dyn_stride = p.a_dyn_stride; wp.dyn_base = p.a_dyn_base;
      wp.ld_out = r.tile_n;
      if (r.combine) {
        wp.tickets = p.combine_tickets; wp.bias = p.bias; wp.final_out = p.c; wp.ld_final = p.ldc;
        wp.expsum = p.expsum; wp.expsum_col0 = p.expsum_col0; wp.expsum_ncols = p.expsum_ncols;
      } else {   // launch_reduce reads slabs at the padded width
        p.partial_ld = r.tile_n; p.partial_slab = r.slab;
      }
      return gemm_wide_forward(wp, st);
    case GEMM_PATH_WIDE_GRADIENT:
      wp.wide = p.a; wp.ld_wide = p.lda; wp.n_wide = p.m;
      wp.x = p.b; wp.ldx = p.ldb; wp.ids = p.b_rows; wp.n_narrow = p.n;
      wp.dyn_stride = p.b_dyn_stride; wp.dyn_base = p.b_dyn_base;
      wp.ld_out = p.n;
      return gemm_wide_gradient(wp, st);
    default: {
      BSIG_REQUIRE(!f.partial_bias, "gemm: partial bias sums outside the whole-width gradient path");
      p.a_unal = r.a_unal; p.b_unal = r.b_unal;
      const int rc = r.path == GEMM_PATH_LEAN
                         ? kTiles[r.tile].lean(p, f.a_kmajor, f.b_kmajor, st)
                         : kTiles[r.tile].mfma(p, f.a_kmajor, f.b_kmajor, (f.a.vec4 || r.a_unal) ? 4 : 1,
                                               (f.b.vec4 || r.b_unal) ? 4 : 1, st);
      if (rc == BSIG_OK) BSIG_CHECK_LAUNCH("gemm_mfma");
      return rc;
    }
  }
}

int gemm_run(GemmParams p, void* workspace, size_t workspace_bytes, hipStream_t st,
             int* n_expsum) {
  BSIG_REQUIRE(p.a && p.b && p.c, "gemm: null pointer");
  BSIG_REQUIRE(p.m >= 0 && p.n >= 0 && p.k >= 0, "gemm: bad dims");
  const int e = p.epilogue;
  BSIG_REQUIRE((e >= BSIG_EPI_NONE && e <= BSIG_EPI_MUL_DACT) || e == EPI_ADAM,
               "gemm: bad epilogue");
  BSIG_REQUIRE(!((e == BSIG_EPI_BIAS || e == BSIG_EPI_BIAS_ACT || e == BSIG_EPI_COS_OFF) &&
                 !p.bias), "gemm: epilogue needs bias");
  BSIG_REQUIRE(!(e == BSIG_EPI_MUL_DACT && !p.aux), "gemm: epilogue needs aux");
  BSIG_REQUIRE(!(e == EPI_ADAM && !(p.adam_m && p.adam_v && p.adam_dyn)),
               "gemm: Adam epilogue needs its state");
  BSIG_REQUIRE(p.ldc >= (e == BSIG_EPI_COS_SIN ? 2 * (int64_t)p.n : (int64_t)p.n),
               "gemm: ldc too small");
  if (n_expsum) *n_expsum = 0;
  BSIG_REQUIRE(!(p.expsum && e != BSIG_EPI_BIAS), "gemm: expsum needs the bias epilogue");
  if (p.m == 0 || p.n == 0) return BSIG_OK;
  const GemmFacts f = gemm_facts(p, workspace, workspace_bytes);
  GemmRoute r;
  BSIG_TRY(gemm_route(f, &r));
  p.partial = reinterpret_cast<float*>(workspace);
  int rc = launch_route(p, f, r, st);
  // The one fallback.  A launcher may hand its call back: the whole-width launchers on guards of their own that
  // the facts do not carry (a workspace that is not 16-byte aligned), launch_lean for a gathered k-major operand
  // on a tile where LeanLoader::kSame is false (96 rows).  The call then runs one step down: a whole-width product
  // on the generic kernels' own plan, a lean one as gemm_mfma_kernel on the same plan, bit-identical by construction.
  if (rc == BSIG_EUNSUPPORTED && (r.path == GEMM_PATH_WIDE_FORWARD || r.path == GEMM_PATH_WIDE_GRADIENT)) {
    BSIG_TRY(route_generic(f, &r));
    rc = launch_route(p, f, r, st);
  }
  if (rc == BSIG_EUNSUPPORTED && r.path == GEMM_PATH_LEAN) {
    r.path = GEMM_PATH_MFMA;
    rc = launch_route(p, f, r, st);
  }
  if (rc != BSIG_OK) return rc;
  if (r.reduce) return launch_reduce(p, st, n_expsum);
  // (one exp partial per workgroup of an unsplit launch, per 64-row tile of a combining one)
  if (n_expsum && p.expsum) *n_expsum = (int)(r.workgroups / r.splits);
  return BSIG_OK;
}

int gemm_f32(const float* a, int64_t lda, int a_kmajor, const int32_t* a_rows,
             const float* b, int64_t ldb, int b_kmajor, const int32_t* b_rows, float* c,
             int64_t ldc, int64_t m, int64_t n, int64_t k, int epilogue, int act,
             const float* bias, const float* aux, int64_t ldaux, float alpha,
             void* workspace, size_t workspace_bytes, hipStream_t st, int math = 0) {
  BSIG_REQUIRE(math == BSIG_MATMUL_FP32 || math == BSIG_MATMUL_SPLIT_BF16, "gemm: unknown matmul precision %d", math);
  BSIG_REQUIRE(m >= 0 && n >= 0 && k >= 0 && m < (1 << 30) && n < (1 << 30) && k < (1 << 30),
               "gemm: bad dims");
  BSIG_REQUIRE(epilogue >= BSIG_EPI_NONE && epilogue <= BSIG_EPI_MUL_DACT, "gemm: bad epilogue");
  GemmParams p;
  p.a = a; p.lda = lda; p.a_rows = a_rows; p.a_kmajor = a_kmajor;
  p.b = b; p.ldb = ldb; p.b_rows = b_rows; p.b_kmajor = b_kmajor;
  p.c = c; p.ldc = ldc;
  p.m = (int)m; p.n = (int)n; p.k = (int)k;
  p.epilogue = epilogue; p.act = act; p.bias = bias; p.aux = aux; p.ldaux = ldaux;
  p.alpha = alpha; p.math = math;
  return gemm_run(p, workspace, workspace_bytes, st);
}

__global__ __launch_bounds__(256) void rff_coeff_kernel(const float* __restrict__ freqs,
                                                        const float* __restrict__ sigma,
                                                        float* __restrict__ coeff,
                                                        int64_t m_feat, int64_t in_dim,
                                                        int64_t ld) {
  const int64_t total = m_feat * ld;
  for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
       e += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = e / ld, c = e % ld;
    coeff[e] = c < in_dim ? freqs[r * in_dim + c] / sigma[c] : 0.f;
  }
}

}  // namespace bsig

using namespace bsig;

extern "C" size_t bsig_gemm_workspace_bytes(int64_t m, int64_t n, int64_t k) {
  size_t need = (size_t)64 * (size_t)m * (size_t)n * sizeof(float) <= ((size_t)256 << 20)
                    ? (size_t)64 * (size_t)m * (size_t)n * sizeof(float)
                    : plan_gemm(m, n, k, (size_t)1 << 40, false).splits * (size_t)m * (size_t)n * sizeof(float);
  // the whole-width products (gemm_wide.h): up to 8 K slices of slabs at the padded head width
  if (m >= 2048 && gemm_wide_covers((int)n))
    need = std::max(need, (size_t)8 * (size_t)m * (size_t)round_up<int64_t>(n, 16) * sizeof(float));
  if (k >= 2048 && gemm_wide_covers((int)m))
    need = std::max(need, (size_t)8 * (size_t)m * (size_t)n * sizeof(float));
  return need;
}

extern "C" int bsig_gemm_f32(const float* a, int64_t lda, int a_kmajor,
                             const int32_t* a_rows, const float* b, int64_t ldb,
                             int b_kmajor, const int32_t* b_rows, float* c, int64_t ldc,
                             int64_t m, int64_t n, int64_t k, int epilogue, int act,
                             const float* bias, const float* aux, int64_t ldaux, float alpha,
                             void* workspace, size_t workspace_bytes, bsig_stream_t stream) {
  return gemm_f32(a, lda, a_kmajor, a_rows, b, ldb, b_kmajor, b_rows, c, ldc, m, n, k,
                  epilogue, act, bias, aux, ldaux, alpha, workspace, workspace_bytes,
                  as_stream(stream));
}

extern "C" int bsig_rff_coeff(const float* freqs, const float* sigma, float* coeff,
                              int64_t m_feat, int64_t in_dim, int64_t ld_coeff,
                              bsig_stream_t stream) {
  BSIG_REQUIRE(freqs && sigma && coeff && ld_coeff >= in_dim, "rff_coeff: bad args");
  const int64_t total = m_feat * ld_coeff;
  if (total == 0) return BSIG_OK;
  const int blocks = (int)std::min<int64_t>(ceil_div<int64_t>(total, 256), 4096);
  hipLaunchKernelGGL(rff_coeff_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), freqs,
                     sigma, coeff, m_feat, in_dim, ld_coeff);
  BSIG_CHECK_LAUNCH("rff_coeff");
  return BSIG_OK;
}

extern "C" int bsig_rff_project(const float* x, int64_t ldx, const int32_t* x_rows,
                                const float* coeff, int64_t ld_coeff, const float* offset,
                                float* feats, int64_t ld_feats, int64_t batch,
                                int64_t in_dim, int64_t m_feat, float a, int cos_only,
                                void* workspace, size_t workspace_bytes,
                                bsig_stream_t stream) {
  bsig::Range roctx_range("bsig_rff_project");
  BSIG_REQUIRE(!(cos_only && !offset), "rff_project: cos-only features need an offset");
  return gemm_f32(x, ldx, 0, x_rows, coeff, ld_coeff, 0, nullptr, feats, ld_feats, batch,
                  m_feat, in_dim, cos_only ? BSIG_EPI_COS_OFF : BSIG_EPI_COS_SIN, 0, offset,
                  nullptr, 0, a, workspace, workspace_bytes, as_stream(stream));
}

// ---- include/bsig_matmul.h
extern "C" int bsig_gemm_f32_ex(const float* a, int64_t lda, int a_kmajor,
                                const int32_t* a_rows, const float* b, int64_t ldb,
                                int b_kmajor, const int32_t* b_rows, float* c, int64_t ldc,
                                int64_t m, int64_t n, int64_t k, int epilogue, int act,
                                const float* bias, const float* aux, int64_t ldaux, float alpha,
                                void* workspace, size_t workspace_bytes, bsig_stream_t stream, int matmul) {
  return gemm_f32(a, lda, a_kmajor, a_rows, b, ldb, b_kmajor, b_rows, c, ldc, m, n, k,
                  epilogue, act, bias, aux, ldaux, alpha, workspace, workspace_bytes,
                  as_stream(stream), matmul);
}

extern "C" int bsig_rff_project_ex(const float* x, int64_t ldx, const int32_t* x_rows,
                                   const float* coeff, int64_t ld_coeff, const float* offset,
                                   float* feats, int64_t ld_feats, int64_t batch,
                                   int64_t in_dim, int64_t m_feat, float a, int cos_only,
                                   void* workspace, size_t workspace_bytes,
                                   bsig_stream_t stream, int matmul) {
  bsig::Range roctx_range("bsig_rff_project");
  BSIG_REQUIRE(!(cos_only && !offset), "rff_project: cos-only features need an offset");
  return gemm_f32(x, ldx, 0, x_rows, coeff, ld_coeff, 0, nullptr, feats, ld_feats, batch,
                  m_feat, in_dim, cos_only ? BSIG_EPI_COS_OFF : BSIG_EPI_COS_SIN, 0, offset,
                  nullptr, 0, a, workspace, workspace_bytes, as_stream(stream), matmul);
}

// gemm_run's route for a product of dense, 16-byte aligned operands (gemm_facts_dense), as host arithmetic
extern "C" int bsig_debug_gemm_path(int64_t m, int64_t n, int64_t k, int a_kmajor, int b_kmajor,
                                    int gathered, int epilogue, size_t workspace_bytes, int matmul,
                                    int32_t* out) {
  BSIG_REQUIRE(out, "gemm path: null pointer");
  for (int i = 0; i < 8; ++i) out[i] = 0;
  BSIG_REQUIRE(m >= 1 && n >= 1 && k >= 0 && m < (1 << 30) && n < (1 << 30) && k < (1 << 30), "gemm path: bad dims");
  BSIG_REQUIRE((epilogue >= BSIG_EPI_NONE && epilogue <= BSIG_EPI_MUL_DACT) || epilogue == EPI_ADAM,
               "gemm path: bad epilogue %d", epilogue);
  BSIG_REQUIRE(matmul == BSIG_MATMUL_FP32 || matmul == BSIG_MATMUL_SPLIT_BF16,
               "gemm path: unknown matmul precision %d", matmul);
  GemmRoute r;
  BSIG_TRY(gemm_route(gemm_facts_dense(m, n, k, a_kmajor != 0, b_kmajor != 0, gathered != 0, epilogue,
                                       workspace_bytes, matmul), &r));
  out[0] = r.path; out[1] = r.tile_m; out[2] = r.tile_n; out[3] = r.splits; out[4] = r.k_chunk;
  out[5] = (int32_t)std::min<int64_t>(r.workgroups, INT32_MAX);
  out[6] = r.declined;
  return BSIG_OK;
}
