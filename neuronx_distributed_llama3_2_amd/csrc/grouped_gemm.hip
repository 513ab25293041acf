// Grouped (ragged-M) bf16 GEMMs for the dropless MoE expert MLPs on gfx950 MFMA: the 128 x 128-tile
// forward / input-gradient kernel that takes the shapes csrc/grouped_rowgemm.hip does not -- a
// reduction length that is not a multiple of 32 (any multiple of 8 works here) -- or every shape
// with NXD_GG_ROW=0.  The expert weight gradients run on csrc/wgrad_gemm.hip (grouped mode).
//
// Tokens are sorted by expert on the device (argsort of the router's top-k choices); expert e
// owns rows offs[e] .. offs[e+1] of the sorted activations.  The group sizes never travel to the
// host: every launch is sized for the worst case (ceil(M / 128) + E row tiles) and each workgroup
// finds its (expert, row tile) from the device-resident offsets, so the MoE layer has no
// device->host sync and can be captured in a hipGraph (reference: modules/moe/expert_mlps.py
// :169-265 runs every token through every expert, or drops by capacity; this computes only the
// chosen rows).
//
// Two products, one kernel template (C = A.B, reduction over k):
//   FWD   y[m, n]     = x[m, :]  . W[e][:, n]        A row-major [M][K],  B = W[e] stored [K][N]
//   DGRAD dx[m, k]    = dy[m, :] . W[e][k, :]^T      A row-major [M][N],  B = W[e] stored [K][N] read as [n][k]
// Workgroup = 4 waves, 128 x 128 output tile (2 x 2 waves of 64 x 64 = 2 x 2 v_mfma_f32_32x32x16_bf16
// tiles each), K-step 64, two LDS buffers (64 KiB): full reduction tiles go global -> LDS by
// LDS-DMA (tile t+1 in flight while tile t runs its 16 MFMAs per wave), a ragged reduction tail
// by zero-filling register staging; workgroups walk the tile grid in L2-sized bands
// (band_raster).  Mixtral shapes: 0.55-0.74 -> 0.80-0.84 PF/s fwd / dgrad
// (profiles/r2_moe_layer_v1.md, which also holds the VGPR-staged and 256 x 256-tile variants that
// were dropped).  Operands consumed along their contiguous axis are read with
// ds_read_b128 from a [row][64] image (16-B chunk XOR (row>>1)&7: conflict-free over 16 lanes);
// operands stored reduction-major are read with the hardware transpose ds_read_b64_tr_b16 from a
// [k][128] image (chunk XOR (k&3)<<2: the four rows of one transposed read and the two column
// blocks of a 32-lane half land on disjoint banks).
#include "gemm_tile.h"

#include <cstdlib>

namespace nxd {
namespace gg {

constexpr int BM = 128, BN = 128, BK = 64, NT = 256;
constexpr int TILE_BYTES = BM * BK * 2;   // 16 KiB: one operand tile (both images)

enum Mode { FWD = 0, DGRAD = 1 };

struct Params {
  const uint16_t* a;
  const uint16_t* b;
  void* c;
  const int* offs;      // [E + 1] device offsets of the expert groups in the sorted rows
  int E;
  int M;                // rows of the sorted activations
  int K;                // reduction length (FWD: in features, DGRAD: out features of W)
  int N;                // output columns
  int lda, ldb, ldc;
  int64_t b_estride;    // elements between experts' weights
  int n_tiles, r_tiles; // output tiles along N, row-tile slots
  int band;             // row tiles per raster band (band_raster)
};

// byte offsets inside one 16 KiB image
__device__ __forceinline__ int row_img(int r, int c) { return r * 128 + 16 * (c ^ ((r >> 1) & 7)); }   // [128][64]
__device__ __forceinline__ int tr_img(int k, int c) { return k * 256 + 16 * (c ^ ((k & 3) << 2)); }     // [64][128]

// Stage a [128 rows][64 k] tile whose rows are contiguous along k: 1024 16-B chunks, 4 per thread.
__device__ __forceinline__ void load_rows(u32x4_t* v, const uint16_t* base, int ld, int rows_valid, int k0, int K) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = t + NT * i, r = idx >> 3, c = idx & 7;
    const int k = k0 + 8 * c;
    v[i] = u32x4_t{0, 0, 0, 0};
    if (r < rows_valid && k < K) v[i] = *reinterpret_cast<const u32x4_t*>(base + (int64_t)r * ld + k);
  }
}
__device__ __forceinline__ void store_rows(char* img, const u32x4_t* v) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = t + NT * i, r = idx >> 3, c = idx & 7;
    *reinterpret_cast<u32x4_t*>(img + row_img(r, c)) = v[i];
  }
}
// Stage a [64 k][128 cols] tile stored k-major (rows contiguous along the output columns).
__device__ __forceinline__ void load_tr(u32x4_t* v, const uint16_t* base, int ld, int k_valid, int c0, int C) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = t + NT * i, k = idx >> 4, c = idx & 15;
    const int col = c0 + 8 * c;
    v[i] = u32x4_t{0, 0, 0, 0};
    if (k < k_valid && col < C) v[i] = *reinterpret_cast<const u32x4_t*>(base + (int64_t)k * ld + col);
  }
}
__device__ __forceinline__ void store_tr(char* img, const u32x4_t* v) {
  const int t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int idx = t + NT * i, k = idx >> 4, c = idx & 15;
    *reinterpret_cast<u32x4_t*>(img + tr_img(k, c)) = v[i];
  }
}

// LDS-DMA staging (global_load_lds_dwordx4: 1 KiB per wave-instruction, written lane-linearly at
// M0): the XOR swizzle of the LDS images is applied to each lane's SOURCE address instead, so the
// tile never passes through VGPRs or the ds_write path (whose VGPR->LDS transfer, ~79 B/clk/CU,
// cost more LDS cycles per k-step than the MFMA fragment reads).  Issued from inline asm so the
// compiler does not wait for it before every transposed LDS read; completion is a manual
// vmcnt(0) before the k-step's barrier.  Rows / columns past the valid range re-read a valid
// chunk (their outputs are never stored); reduction tails take the zero-filling VGPR path.
// [128 rows][64 k] row image: piece P (1 KiB) = rows 8P .. 8P + 7; lane l -> row 8P + l / 8, slot l % 8.
__device__ __forceinline__ void dma_rows(uint32_t img, const uint16_t* base, int ld, int rows_valid, int k0) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = w * 4 + i, r = piece * 8 + (l >> 3), c = (l & 7) ^ ((r >> 1) & 7);
    const int rr = min(r, rows_valid - 1);
    dma16(base + (int64_t)rr * ld + k0 + 8 * c, __builtin_amdgcn_readfirstlane(img + piece * 1024));
  }
}
// [64 k][128 cols] k-major image: piece P = k rows 4P .. 4P + 3; lane l -> k 4P + l / 16, slot l % 16.
__device__ __forceinline__ void dma_tr(uint32_t img, const uint16_t* base, int ld, int c0, int C) {
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int piece = w * 4 + i, k = piece * 4 + (l >> 4), c = (l & 15) ^ ((k & 3) << 2);
    const int col = min(c0 + 8 * c, C - 8);
    dma16(base + (int64_t)k * ld + col, __builtin_amdgcn_readfirstlane(img + piece * 1024));
  }
}

// 32x32x16 operand fragment of rows [rbase, rbase + 32), k-step s: lane (r = l & 31, h = l >> 5)
// needs element j = 0..7 at (row rbase + r, k 16 s + 8 h + j).
__device__ __forceinline__ bf16x8_t frag_rows(const char* img, int rbase, int s) {
  const int l = threadIdx.x & 63;
  return __builtin_bit_cast(bf16x8_t, *reinterpret_cast<const u32x4_t*>(img + row_img(rbase + (l & 31), 2 * s + (l >> 5))));
}
// Same fragment from a k-major image: two transposed reads of 4 k-rows x 16 columns per 16-lane
// group; lane 4q + p of group g supplies (k row 16 s + 8 h + q (+4), column rbase + 16 (g & 1) + 4 p).
__device__ __forceinline__ bf16x8_t frag_tr(const char* img, int rbase, int s) {
  const int l = threadIdx.x & 63, g = l >> 4, i = l & 15, q = i >> 2, p = i & 3;
  const int h = g >> 1;
  const int col = rbase + 16 * (g & 1) + 4 * p;
  const int k = 16 * s + 8 * h + q;
  const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_short4_t*)(img + tr_img(k, col >> 3) + 8 * (p & 1)));
  const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16(
      (lds_short4_t*)(img + tr_img(k + 4, col >> 3) + 8 * (p & 1)));
  const short __attribute__((ext_vector_type(8))) a8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, a8);
}

template <int MODE>
__global__ void __launch_bounds__(NT) grouped_gemm_kernel(Params p) {
  __shared__ __attribute__((aligned(16))) char smem[4 * TILE_BYTES];   // [buf][A | B]
  const int nwg = gridDim.x;
  const int id = xcd_remap(blockIdx.x, nwg);
  const int wid = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int wm = wid >> 1, wn = wid & 1;

  int e = -1, row0 = 0, row_end = 0, n0 = 0;
  {
    int slot, ct;
    band_raster(id, p.r_tiles, p.n_tiles, p.band, slot, ct);
    n0 = ct * BN;
    // locate (expert, row tile) of this slot from the device offsets (E scalar iterations)
    int acc = 0, prev = 0;
    for (int x = 0; x < p.E; ++x) {
      int lo = min(max(p.offs[x], prev), p.M), hi = min(max(p.offs[x + 1], lo), p.M);
      prev = hi;
      const int tiles = (hi - lo + BM - 1) / BM;
      if (slot < acc + tiles) {
        e = x;
        row0 = lo + (slot - acc) * BM;
        row_end = hi;
        break;
      }
      acc += tiles;
    }
    if (e < 0) return;                        // past the last real tile: the whole workgroup exits
  }

  const uint16_t* a_base;
  const uint16_t* b_base;
  if (MODE == FWD) {
    a_base = p.a + (int64_t)row0 * p.lda;                  // x rows, contiguous along k
    b_base = p.b + (int64_t)e * p.b_estride;               // W[e] [K][N], k-major
  } else {
    a_base = p.a + (int64_t)row0 * p.lda;                  // dy rows, contiguous along n (= reduction)
    b_base = p.b + (int64_t)e * p.b_estride + (int64_t)n0 * p.ldb;   // W[e] rows = output columns
  }
  const int rows_valid = row_end - row0;

  f32x16_t acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x16_t{0};

  const int n_k = (p.K + BK - 1) / BK;
  u32x4_t va[4], vb[4];
  auto load = [&](int t) {
    const int k0 = t * BK;
    load_rows(va, a_base, p.lda, rows_valid, k0, p.K);
    if (MODE == FWD) load_tr(vb, b_base + (int64_t)k0 * p.ldb, p.ldb, p.K - k0, n0, p.N);
    else load_rows(vb, b_base, p.ldb, p.N - n0, k0, p.K);
  };
  auto store = [&](int buf) {
    char* ia = smem + buf * 2 * TILE_BYTES;
    char* ib = ia + TILE_BYTES;
    store_rows(ia, va);
    if (MODE == DGRAD) store_rows(ib, vb); else store_tr(ib, vb);
  };
  // full reduction tile t straight into LDS buffer `buf`
  auto dma = [&](int t, int buf) {
    const int k0 = t * BK;
    const uint32_t ia = lds_addr(smem + buf * 2 * TILE_BYTES), ib = ia + TILE_BYTES;
    dma_rows(ia, a_base, p.lda, rows_valid, k0);
    if (MODE == FWD) dma_tr(ib, b_base + (int64_t)k0 * p.ldb, p.ldb, n0, p.N);
    else dma_rows(ib, b_base, p.ldb, p.N - n0, k0);
  };
  // tiles [0, n_full) cover BK full reduction steps; a ragged last tile is zero-filled through VGPRs
  const int n_full = p.K / BK;

  if (n_k > 0) {
    if (n_full > 0) {
      dma(0, 0);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    } else {
      load(0);
      store(0);
    }
    __syncthreads();
  }
  for (int t = 0; t < n_k; ++t) {
    const int buf = t & 1;
    const bool next_dma = t + 1 < n_full, next_stage = t + 1 < n_k && !next_dma;
    if (next_dma) dma(t + 1, buf ^ 1);
    if (next_stage) load(t + 1);
    const char* ia = smem + buf * 2 * TILE_BYTES;
    const char* ib = ia + TILE_BYTES;
#pragma unroll
    for (int s = 0; s < BK / 16; ++s) {
      bf16x8_t af[2], bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        af[i] = frag_rows(ia, wm * 64 + 32 * i, s);
        bfr[i] = (MODE == DGRAD) ? frag_rows(ib, wn * 64 + 32 * i, s) : frag_tr(ib, wn * 64 + 32 * i, s);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[i], bfr[j], acc[i][j], 0, 0, 0);
    }
    if (next_stage) store(buf ^ 1);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
  }

  // epilogue: acc element v of tile (i, j) is (row (v & 3) + 8 (v >> 2) + 4 (lane >> 5), col lane & 31)
  const int ccol = lane & 31, rsub = 4 * (lane >> 5);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = n0 + wn * 64 + 32 * j + ccol;
      if (col >= p.N) continue;
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = wm * 64 + 32 * i + (v & 3) + 8 * (v >> 2) + rsub;
        if (r >= rows_valid) continue;
        const int64_t grow = row0 + r;
        reinterpret_cast<uint16_t*>(p.c)[grow * p.ldc + col] = f2bf(acc[i][j][v]);
      }
    }
}

static int band_rows() {
  static const int b = [] {
    const char* e = getenv("NXD_GG_BAND");
    const int v = e ? atoi(e) : 8;
    return v > 0 ? v : 8;
  }();
  return b;
}

}  // namespace gg

// mode 0 FWD:   a = x [M, K], b = W [E, K, N], c = y [M, N] bf16
// mode 1 DGRAD: a = dy [M, N], b = W [E, K, N], c = dx [M, K] bf16        (launch N := K, K := N)
// All inner dims multiples of 8 elements and 16-byte aligned rows (checked by the binding).
int grouped_gemm_launch(int mode, const void* a, const void* b, void* c, const int* offs, int E, int M, int K, int N,
                        hipStream_t stream) {
  if (E <= 0 || K <= 0 || N <= 0 || M < 0 || (K % 8) || (N % 8)) return -1;
  if (mode != gg::FWD && mode != gg::DGRAD) return -1;
  gg::Params p{};
  p.a = static_cast<const uint16_t*>(a);
  p.b = static_cast<const uint16_t*>(b);
  p.c = c;
  p.offs = offs;
  p.E = E;
  p.M = M;
  p.band = gg::band_rows();
  p.b_estride = (int64_t)K * N;
  if (mode == gg::FWD) {
    p.K = K; p.N = N; p.lda = K; p.ldb = N; p.ldc = N;
  } else {
    // dx [M, K] = dy [M, N] . W[e]^T : reduction over N, output columns K
    p.K = N; p.N = K; p.lda = N; p.ldb = N; p.ldc = K;
  }
  p.n_tiles = ceil_div(p.N, gg::BN);
  p.r_tiles = ceil_div(M, gg::BM) + E;
  if (M == 0) return 0;
  const int64_t nwg = (int64_t)p.n_tiles * p.r_tiles;
  if (nwg > INT32_MAX) return -2;
  if (mode == gg::FWD)
    hipLaunchKernelGGL(gg::grouped_gemm_kernel<gg::FWD>, dim3((unsigned)nwg), dim3(gg::NT), 0, stream, p);
  else
    hipLaunchKernelGGL(gg::grouped_gemm_kernel<gg::DGRAD>, dim3((unsigned)nwg), dim3(gg::NT), 0, stream, p);
  return hipGetLastError() == hipSuccess ? 0 : -3;
}

}  // namespace nxd
