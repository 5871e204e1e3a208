// Split-bf16 GEMM: C[m,n] = epi( sum_k A(m,k) * B(n,k) ) on v_mfma_f32_32x32x16_bf16 -- the opt-in
// matmul precision BSIG_MATMUL_SPLIT_BF16 (include/bsig_matmul.h).  gfx950's fp32 MFMAs issue at the
// vector rate (157 TFLOP/s) and there is no xf32 form; its bf16 matrix pipes do 16 x that.
//
// Arithmetic.  An fp32 element x is split into p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1)
// (round to nearest even, v_cvt_pk_bf16_f32; the subtractions are exact in fp32), so p0 + p1 + p2 == x
// for normal x.  Of the nine piece products the six with i + j <= 2 are kept -- each exact in the fp32
// accumulator (8 x 8 significant bits); the dropped ones are below 2.01 * 2^-24 |x||y| per term.  One
// accumulation chain per output and K slice: ascending k in steps of 16, within a step the small
// terms first -- (0,2) (1,1) (2,0) (0,1) (1,0) (0,0).  K slices are summed in slice order by
// gemm_reduce_kernel.  Nothing atomic: two runs are bitwise equal.
// Edge behaviour: a non-finite operand element gives non-finite outputs (NaN where fp32 gives inf:
// inf - inf occurs in the split); |x| above the largest bf16 (3.39e38) rounds p0 to inf; p2 of
// |x| < 2^-100 may underflow, the result then carries fewer than 24 bits of that element.
//
// Kernel.  2 x 2 wavefronts, each TM x TN 32x32 tiles (workgroup tile 64 x 64 or 128 x 128), BK = 32.
// The loader fetches fp32 (16-byte loads at any 4-byte address: k-contiguous rows of any pitch,
// gathered rows, device-resolved row offsets; the last items of a row that would leave its pitch are
// fetched element by element), splits each element ONCE per workgroup and stores the three bf16 planes
// to LDS as [rows][32 + 8]: a lane reads its 8-element fragment of a k16 step (row l & 31,
// k = 8 (l >> 5) ..) in one ds_read_b128, and the 80-byte pitch puts the 16 lanes of every
// ds_read_b128 group on 16 distinct 16-byte slots of the 256-byte bank row.  k-major operands are
// transposed on the way: a thread takes two consecutive k of four rows and stores one packed pair per
// row and plane.  Epilogues: the shared tile epilogues of gemm_kernel.h (32x32x16 has the C/D layout of
// 32x32x2), raw slabs when K is split.
#include "gemm_kernel.h"
#include "gemm_split_bf16.h"

namespace bsig {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

constexpr int SPB = BK + 8;   // LDS row pitch in bf16 elements (80 bytes)

struct Pieces { unsigned short p0, p1, p2; };
__device__ inline Pieces split3(float x) {
  const __bf16 h0 = (__bf16)x;
  const float r1 = x - (float)h0;
  const __bf16 h1 = (__bf16)r1;
  const float r2 = r1 - (float)h1;
  const __bf16 h2 = (__bf16)r2;
  return Pieces{__builtin_bit_cast(unsigned short, h0), __builtin_bit_cast(unsigned short, h1),
                __builtin_bit_cast(unsigned short, h2)};
}

// One operand tile of ROWS rows x BK contraction elements: fp32 in registers, three bf16 planes in LDS.
template <int ROWS, bool KMAJOR>
struct SplitLoader {
  // k-contiguous: an item is four consecutive k of one row; k-major: two consecutive k of four rows
  static constexpr int kItems = KMAJOR ? ROWS / 64 : ROWS / 32;
  static constexpr int kVals = KMAJOR ? 8 : 4;
  static_assert(ROWS % 64 == 0, "tile rows");
  struct Regs { float r[kItems][kVals]; };
  int64_t srow[kItems];   // k-contiguous: element offset of each item's (gathered) source row
  int64_t off;

  __device__ inline void init(const int32_t* __restrict__ idx, int row0, int nrows, int tid, int64_t ld,
                              int64_t row_off) {
    off = row_off;
    if constexpr (!KMAJOR) {
#pragma unroll
      for (int it = 0; it < kItems; ++it) {
        const int64_t gr = min(row0 + (tid + it * 256) / 8, nrows - 1) + row_off;
        srow[it] = (idx ? (int64_t)idx[gr] : gr) * ld;
      }
    }
  }

  __device__ inline void fetch(Regs& t, const float* __restrict__ g, int64_t ld,
                               const int32_t* __restrict__ idx, int row0, int k0, int kend, int ktot,
                               int tid) const {
    if constexpr (!KMAJOR) {
      const int gk = k0 + (tid & 7) * 4;
#pragma unroll
      for (int it = 0; it < kItems; ++it) {
        const float* src = g + srow[it];
        if (gk + 4 <= ld) {
          const f32x4u q = *reinterpret_cast<const f32x4u*>(src + gk);
          t.r[it][0] = q.x; t.r[it][1] = q.y; t.r[it][2] = q.z; t.r[it][3] = q.w;
        } else {
#pragma unroll
          for (int v = 0; v < 4; ++v) t.r[it][v] = src[min((int64_t)gk + v, ld - 1)];
        }
#pragma unroll
        for (int v = 0; v < 4; ++v)
          if (gk + v >= kend) t.r[it][v] = 0.f;
      }
    } else {
      constexpr int per_k = ROWS / 4;
#pragma unroll
      for (int it = 0; it < kItems; ++it) {
        const int item = tid + it * 256;
        const int kk = k0 + 2 * (item / per_k);
        const int r0 = row0 + (item % per_k) * 4;
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int64_t gkc = min(kk + u, ktot - 1) + off;
          const float* src = g + (idx ? (int64_t)idx[gkc] : gkc) * ld;
          if (r0 + 4 <= ld) {
            const f32x4u q = *reinterpret_cast<const f32x4u*>(src + r0);
            t.r[it][4 * u + 0] = q.x; t.r[it][4 * u + 1] = q.y; t.r[it][4 * u + 2] = q.z; t.r[it][4 * u + 3] = q.w;
          } else {
#pragma unroll
            for (int v = 0; v < 4; ++v) t.r[it][4 * u + v] = src[min((int64_t)r0 + v, ld - 1)];
          }
          if (kk + u >= kend) {
#pragma unroll
            for (int v = 0; v < 4; ++v) t.r[it][4 * u + v] = 0.f;
          }
        }
      }
    }
  }

  // planes: [3][ROWS][SPB] bf16
  __device__ inline void commit(const Regs& t, unsigned short* __restrict__ lds, int tid) const {
#pragma unroll
    for (int it = 0; it < kItems; ++it) {
      const int item = tid + it * 256;
      if constexpr (!KMAJOR) {
        const int o = (item / 8) * SPB + (item % 8) * 4;
        Pieces s[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) s[v] = split3(t.r[it][v]);
        auto pack = [](unsigned short lo, unsigned short hi) { return (uint32_t)lo | ((uint32_t)hi << 16); };
        *reinterpret_cast<uint2*>(lds + o) = make_uint2(pack(s[0].p0, s[1].p0), pack(s[2].p0, s[3].p0));
        *reinterpret_cast<uint2*>(lds + ROWS * SPB + o) = make_uint2(pack(s[0].p1, s[1].p1), pack(s[2].p1, s[3].p1));
        *reinterpret_cast<uint2*>(lds + 2 * ROWS * SPB + o) = make_uint2(pack(s[0].p2, s[1].p2), pack(s[2].p2, s[3].p2));
      } else {
        constexpr int per_k = ROWS / 4;
        const int kp = item / per_k, r0 = (item % per_k) * 4;
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const Pieces lo = split3(t.r[it][v]), hi = split3(t.r[it][4 + v]);
          const int o = (r0 + v) * SPB + 2 * kp;
          *reinterpret_cast<uint32_t*>(lds + o) = (uint32_t)lo.p0 | ((uint32_t)hi.p0 << 16);
          *reinterpret_cast<uint32_t*>(lds + ROWS * SPB + o) = (uint32_t)lo.p1 | ((uint32_t)hi.p1 << 16);
          *reinterpret_cast<uint32_t*>(lds + 2 * ROWS * SPB + o) = (uint32_t)lo.p2 | ((uint32_t)hi.p2 << 16);
        }
      }
    }
  }
};

template <int TM, int TN, bool AKM, bool BKM>
__global__ __launch_bounds__(256) void gemm_split_bf16_kernel(GemmParams p) {
#ifndef BSIG_HOST_SAN_BUILD
  constexpr int BM = 2 * TM * 32, BN = 2 * TN * 32;
  constexpr int kAh = 3 * BM * SPB, kBh = 3 * BN * SPB;          // bf16 elements
  constexpr int kOps = (kAh + kBh) / 2, kEpi = 4 * 32 * 32;     // floats
  __shared__ __attribute__((aligned(16))) float smem[kOps > kEpi ? kOps : kEpi];
  unsigned short* As = reinterpret_cast<unsigned short*>(smem);
  unsigned short* Bs = As + kAh;

  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  const int l31 = lane & 31, h = lane >> 5;
  // workgroup -> tile: an XCD works on a contiguous run of tiles (gemm_mfma_kernel; a bijection on [0, nwg))
  int bx = blockIdx.x, by = blockIdx.y, bz = blockIdx.z;
  if (p.xcd_swz) {
    const int gx = gridDim.x, gy = gridDim.y, nwg = gx * gy * (int)gridDim.z;
    const int lin = bx + gx * (by + gy * bz);
    const int xcd = lin & 7, q = nwg >> 3, r = nwg & 7;
    const int wgid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (lin >> 3);
    bx = wgid % gx; by = (wgid / gx) % gy; bz = wgid / (gx * gy);
  }
  p.bid_z = bz;
  const int m0 = by * BM, n0 = bx * BN;
  const int kbeg = bz * p.k_chunk;
  const int kend = min(p.k, kbeg + p.k_chunk);
  // a fused Adam step always leaves through a raw slab (split_bf16_plan): the shared epilogue code
  // reads "p.splits > 1" as "store the slab of slice bid_z"
  if (p.epilogue == EPI_ADAM && p.splits < 2) p.splits = 2;

  floatx16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][j][q] = 0.f;

  SplitLoader<BM, AKM> la;
  SplitLoader<BN, BKM> lb;
  typename SplitLoader<BM, AKM>::Regs ra;
  typename SplitLoader<BN, BKM>::Regs rb;
  const int nkt = (kend - kbeg + BK - 1) / BK;
  const int64_t dstep = p.dyn ? (int64_t)(p.dyn[0] + p.dyn_delta) : 0;
  la.init(p.a_rows, m0, p.m, tid, p.lda, dstep * p.a_dyn_stride + p.a_dyn_base);
  lb.init(p.b_rows, n0, p.n, tid, p.ldb, dstep * p.b_dyn_stride + p.b_dyn_base);
  if (nkt > 0) {
    la.fetch(ra, p.a, p.lda, p.a_rows, m0, kbeg, kend, p.k, tid);
    lb.fetch(rb, p.b, p.ldb, p.b_rows, n0, kbeg, kend, p.k, tid);
  }
  for (int kt = 0; kt < nkt; ++kt) {
    la.commit(ra, As, tid);
    lb.commit(rb, Bs, tid);
    __syncthreads();
    if (kt + 1 < nkt) {   // the next tile's loads fly over this tile's MFMAs
      const int k0 = kbeg + (kt + 1) * BK;
      la.fetch(ra, p.a, p.lda, p.a_rows, m0, k0, kend, p.k, tid);
      lb.fetch(rb, p.b, p.ldb, p.b_rows, n0, k0, kend, p.k, tid);
    }
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {
      bf16x8 af[TM][3], bf[TN][3];
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          af[i][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(
              As + pl * BM * SPB + ((wm * TM + i) * 32 + l31) * SPB + ks * 16 + h * 8));
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          bf[j][pl] = __builtin_bit_cast(bf16x8, *reinterpret_cast<const uint4*>(
              Bs + pl * BN * SPB + ((wn * TN + j) * 32 + l31) * SPB + ks * 16 + h * 8));
      // small terms first: (0,2) (1,1) (2,0) (0,1) (1,0) (0,0)
#define BSIG_SPLIT_MFMA(PA, PB)                                                                       \
  _Pragma("unroll") for (int i = 0; i < TM; ++i) _Pragma("unroll") for (int j = 0; j < TN; ++j)       \
      acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i][PA], bf[j][PB], acc[i][j], 0, 0, 0);
      BSIG_SPLIT_MFMA(0, 2) BSIG_SPLIT_MFMA(1, 1) BSIG_SPLIT_MFMA(2, 0)
      BSIG_SPLIT_MFMA(0, 1) BSIG_SPLIT_MFMA(1, 0) BSIG_SPLIT_MFMA(0, 0)
#undef BSIG_SPLIT_MFMA
    }
    __syncthreads();
  }

  // Epilogue: as gemm_mfma_kernel's (each wavefront bounces one 32 x 32 tile at a time through its LDS patch)
  float adam_ss = 0.f, adam_ib = 0.f;   // (unused: EPI_ADAM leaves through slabs)
  float* patch = smem + wid * (32 * 32);
  float exp_acc = 0.f;
  const bool vec_epi = epilogue_vec_ok(p);
#define BSIG_TILE_EPILOGUE(I, J)                                                          \
  if constexpr ((I) < TM && (J) < TN) {                                                   \
    _Pragma("unroll") for (int q = 0; q < 16; ++q)                                        \
        patch[((q & 3) + 8 * (q >> 2) + 4 * h) * 32 + l31] = acc[I][J][q];                \
    __builtin_amdgcn_wave_barrier();                                                      \
    run_tile_epilogue(p, patch, m0 + (wm * TM + (I)) * 32, n0 + (wn * TN + (J)) * 32,     \
                      lane, vec_epi, exp_acc, adam_ss, adam_ib);                          \
    __builtin_amdgcn_wave_barrier();                                                      \
  }
  BSIG_TILE_EPILOGUE(0, 0) BSIG_TILE_EPILOGUE(0, 1)
  BSIG_TILE_EPILOGUE(1, 0) BSIG_TILE_EPILOGUE(1, 1)
#undef BSIG_TILE_EPILOGUE
  static_assert(TM <= 2 && TN <= 2, "extend the tile enumeration");
  if (p.expsum && p.splits == 1) {   // one partial per workgroup, fixed order
    __syncthreads();
    const float s = block_sum(exp_acc, smem);
    if (tid == 0) p.expsum[by * gridDim.x + bx] = s;
  }
#endif
}

bool split_bf16_plan(int64_t m, int64_t n, int64_t k, int epilogue, bool partial_bias, size_t ws_bytes,
                     SplitBf16Plan* pl) {
  if (m < 1 || n < 1) return false;
  // the tile: 128 x 128 where that still gives every CU most of a workgroup and pads little more than
  // 64 x 64 does (a head of 260 outputs: 384 against 320 columns)
  const int64_t t128 = ceil_div<int64_t>(m, 128) * ceil_div<int64_t>(n, 128);
  const int64_t t64 = ceil_div<int64_t>(m, 64) * ceil_div<int64_t>(n, 64);
  const bool big = t128 >= 192 && (double)t128 * 4.0 <= 1.15 * (double)t64;
  pl->tile = big ? 128 : 64;
  const int64_t tiles = big ? t128 : t64;
  // K slices: until there are ~3 workgroups per CU, each with at least four K steps
  int64_t splits = 1;
  if (tiles < 512) {
    splits = ceil_div<int64_t>(768, tiles);
    splits = std::min<int64_t>(splits, std::max<int64_t>(k / (4 * BK), 1));
    splits = std::min<int64_t>(splits, 32);
  }
  const int64_t max_by_ws = (int64_t)(ws_bytes / (sizeof(float) * (size_t)(m * n)));
  const int64_t min_slabs = epilogue == EPI_ADAM ? (partial_bias ? 2 : 1) : 0;
  if (max_by_ws < min_slabs) return false;
  if (min_slabs == 2 && k < 2 * BK) return false;
  splits = std::max<int64_t>(std::min(splits, std::max<int64_t>(max_by_ws, 1)), std::min<int64_t>(min_slabs, 2));
  splits = std::max<int64_t>(splits, 1);
  const int64_t chunk = std::max<int64_t>(round_up<int64_t>(ceil_div<int64_t>(k, splits), BK), BK);
  pl->k_chunk = (int)chunk;
  pl->splits = (int)std::max<int64_t>(ceil_div<int64_t>(k, chunk), 1);
  if (pl->splits < min_slabs) return false;
  pl->slabs = pl->splits > 1 || min_slabs > 0;
  pl->workgroups = tiles * pl->splits;
  return true;
}

template <int T>
static int launch_split_tile(const GemmParams& p, hipStream_t st) {
  const dim3 grid(ceil_div(p.n, 64 * T), ceil_div(p.m, 64 * T), p.splits), block(256);
  const bool akm = p.a_kmajor != 0, bkm = p.b_kmajor != 0;
  if (!akm && !bkm) hipLaunchKernelGGL((gemm_split_bf16_kernel<T, T, false, false>), grid, block, 0, st, p);
  else if (!akm && bkm) hipLaunchKernelGGL((gemm_split_bf16_kernel<T, T, false, true>), grid, block, 0, st, p);
  else if (akm && !bkm) hipLaunchKernelGGL((gemm_split_bf16_kernel<T, T, true, false>), grid, block, 0, st, p);
  else hipLaunchKernelGGL((gemm_split_bf16_kernel<T, T, true, true>), grid, block, 0, st, p);
  BSIG_CHECK_LAUNCH("gemm_split_bf16");
  return BSIG_OK;
}

int launch_split_bf16(const GemmParams& p, const SplitBf16Plan& pl, hipStream_t st) {
  BSIG_REQUIRE(ceil_div<int64_t>(p.m, pl.tile) <= 65535 && pl.splits <= 65535, "gemm_split_bf16: grid too large");
  return pl.tile == 128 ? launch_split_tile<2>(p, st) : launch_split_tile<1>(p, st);
}

}  // namespace bsig
