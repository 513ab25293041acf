// MXFP4 weight-only decode on MFMA weight tiles: y[M, N] = x[M, K] @ deq(W)[Nw, K]^T for 1 <= M <= 16,
// dense or for every expert of a stack (blockIdx.y = expert), reading the 4-bit weights directly.
// ops.gemv.mx_linear routes to the dense form; the expert form (mx_experts_gemm) is built, tested and
// benchmarked as a kernel, but the MoE model does not call it yet.
// The format is that of gemv_mx.hip / ops/gemv.py.  The VALU form there re-reads all M activation
// rows per wave and its converts + v_dot2c grow with M; here the arithmetic does not depend on M.
//
// A wave owns NT tiles of 16 weight rows.  Lane l works on weight row n0 + (l & 15) and, in iteration
// i of its K slice, on block kb = kb0 + 4 i + (l >> 4) of that row: one 16-byte load is the block and
// cvt8 of dword d of the block is exactly the 8 bf16 of the B operand of MFMA d.  The A operand of
// the same lane is x[l & 15][32 kb + 8 d .. + 7].  Both operands of a lane carry the same 8
// k-indices and v_mfma_f32_16x16x32_bf16 sums over all lanes' k, so "lane group g takes block
// 4 i + g" is a legal permutation of k: one iteration is 4 MFMAs per tile, 16 rows x 128 k.  The
// activation loads of an iteration are shared by the wave's NT tiles (one tile alone would pull 4x
// the weight bytes of x through L2).  C: lane l holds rows m = 4 (l >> 4) + r of column l & 15.
//
// The kernel is bound by the number of load instructions, not by bytes or arithmetic (measured by
// taking loads out, profiles/LOG.md), so everything but the weight load itself is made cheap: the
// activations are loaded 64 contiguous bytes per row and transposed over the lane groups with
// v_permlane swaps (mma), the scales as one dword per lane for 4 iterations (load_scales).  The
// weight loads are plain, not non-temporal: an instruction reads 64 bytes of each of 16 rows, half a
// 128-byte line, and the other half follows one iteration later; non-temporal loads were 8-10 %
// slower at every wide shape (measured; that they drop the half-used line early is a guess, no
// counters were taken).
//
// Lane groups whose block is past the slice contribute exact zeros on both operands and do not load;
// activation rows m >= M read row M - 1 (an A row only feeds its own C row, which is not stored);
// weight rows past N are clamped and their columns not stored.  GLU keeps a gate tile and the up
// tile of the same 16 columns as two accumulators, so the epilogue is lane-local.  KS waves of a
// workgroup split K and are summed through LDS in slice order: no atomics, the bits are reproducible.
#include <type_traits>

#include "common.h"

namespace nxd {
namespace gemv_mx_mfma {

struct Params {
  const uint16_t* x;     // [M, K] bf16, rows ldx elements apart
  int64_t ldx;
  const uint8_t* w;      // [Nw, K/2] packed codes, rows ldw bytes apart
  int64_t ldw;
  const uint8_t* scale;  // [Nw, K/32] E8M0, rows lds bytes apart
  int64_t lds;
  const uint16_t* bias;  // [Nw] (nullable; added before the GLU)
  uint16_t* y;
  int64_t ldy;
  int M, N, K;           // N = output columns (GLU: the up rows start at weight row N)
  // expert blockIdx.y: codes / scales that many bytes on, x / y that many elements on (x: 0 = shared)
  int64_t w_estride, s_estride, x_estride, y_estride;
};
static_assert(std::is_trivially_copyable<Params>::value && sizeof(Params) <= 4096, "kernel-argument struct");

// 8 codes of one dword (element 2j = low nibble of byte j) times the block scale -> 8 bf16, in k order
__device__ __forceinline__ bf16x8_t cvt8(uint32_t d, float s) {
  u32x4_t q;
  q[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0));
  q[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1));
  q[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2));
  q[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3));
  return __builtin_bit_cast(bf16x8_t, q);
}

// T output tiles of 16 columns per wave (GLU: T gate + T up weight tiles), KS waves per tile group
template <int T, int KS, bool GLU>
__global__ void __launch_bounds__(256) mx_mfma_kernel(Params p) {
  constexpr int NT = GLU ? 2 * T : T;   // weight tiles (accumulators) per wave
  constexpr int G = 4 / KS;             // tile groups per workgroup
  __shared__ f32x4_t part[KS > 1 ? 4 : 1][NT][64];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rg = wid / KS, ks = wid % KS;
  const int c = lane & 15, g = lane >> 4;
  const int64_t e = blockIdx.y;
  const int tile0 = ((int)blockIdx.x * G + rg) * T;
  const bool active = (int64_t)tile0 * 16 < p.N;   // wave-uniform

  const uint8_t* wr[NT];
  const uint8_t* sr[NT];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t n = min((int64_t)(tile0 + t) * 16 + c, (int64_t)p.N - 1);   // rows past N are clamped (and not stored)
    wr[t] = p.w + e * p.w_estride + n * p.ldw;
    sr[t] = p.scale + e * p.s_estride + n * p.lds;
    if (GLU) {
      wr[T + t] = wr[t] + (int64_t)p.N * p.ldw;
      sr[T + t] = sr[t] + (int64_t)p.N * p.lds;
    }
  }
  const uint16_t* xr = p.x + e * p.x_estride + (int64_t)min(c, p.M - 1) * p.ldx;

  // this wave's K slice, in blocks; slices start at multiples of 4 blocks
  const int KB = p.K >> 5;
  const int per = ((KB + KS - 1) / KS + 3) & ~3;
  const int kb0 = min(ks * per, KB), kb1 = min(KB, kb0 + per);
  const int nit = active ? (kb1 - kb0 + 3) >> 2 : 0;

  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  struct Round {
    u32x4_t x[4];
    u32x4_t w[NT];
  };
  // Scales: a byte load per lane and tile in every iteration is an instruction that touches 16 lines
  // for 64 bytes, and cost a quarter of the kernel's time.  Instead, once per 4 iterations lane
  // (c, g) loads the 4 scale bytes of iteration 4 I + g of its row as one dword (any alignment);
  // iteration 4 I + q then takes byte g of the dword of lane (c, q) with one ds_bpermute.  A dword
  // that would pass the end of the row is put together from the bytes inside it.
  struct Scales {
    uint32_t v[NT];
  };
  auto load_scales = [&](Scales& sc, int I) {
    const int b = kb0 + 16 * I + 4 * g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      uint32_t v = 0x7f7f7f7fu;
      if (b + 3 < KB) {
        __builtin_memcpy(&v, sr[t] + b, 4);
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (b + j < KB) v = (v & ~(0xffu << (8 * j))) | ((uint32_t)sr[t][b + j] << (8 * j));
      }
      sc.v[t] = v;
    }
  };
  auto load = [&](Round& r, int it) {
    // activations, coalesced: load j takes chunk g of block 4 it + j, so the four lane groups read
    // 64 contiguous bytes of a row (loading this lane's own block, chunk d in load d, would touch
    // 64 separate 64-byte segments per instruction).  mma() turns them into the operands.  Blocks
    // past the slice are zeros, not loads, and the test is wave-uniform.
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int kbj = kb0 + 4 * it + j;
      r.x[j] = u32x4_t{0u, 0u, 0u, 0u};
      if (kbj < kb1) r.x[j] = *reinterpret_cast<const u32x4_t*>(xr + (int64_t)kbj * 32 + 8 * g);
    }
    const int kb = kb0 + 4 * it + g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {   // idle lane group: +0 codes (its activations are the zero blocks above)
      r.w[t] = u32x4_t{0u, 0u, 0u, 0u};
      if (kb < kb1) r.w[t] = *reinterpret_cast<const u32x4_t*>(wr[t] + (int64_t)kb * 16);
    }
  };
  auto mma = [&](const Round& r, const Scales& sc, int it) {
    const bool idle = kb0 + 4 * it + g >= kb1;   // scale 1 for the zero codes of an idle lane group
    const int src = c + 16 * (it & 3);
    // 4 x 4 transpose of 16-byte chunks over (load j, lane group g): afterwards register d of lane
    // group g holds chunk d of block 4 it + g.  v_permlane32_swap exchanges lane groups 2, 3 of its
    // first operand with groups 0, 1 of its second, v_permlane16_swap odd groups with even groups.
    u32x4_t x[4] = {r.x[0], r.x[1], r.x[2], r.x[3]};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      u32x2_t a = __builtin_amdgcn_permlane32_swap(x[0][q], x[2][q], false, false);
      u32x2_t b = __builtin_amdgcn_permlane32_swap(x[1][q], x[3][q], false, false);
      const u32x2_t lo = __builtin_amdgcn_permlane16_swap(a[0], b[0], false, false);
      const u32x2_t hi = __builtin_amdgcn_permlane16_swap(a[1], b[1], false, false);
      x[0][q] = lo[0];
      x[1][q] = lo[1];
      x[2][q] = hi[0];
      x[3][q] = hi[1];
    }
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint32_t sv = (uint32_t)__shfl((int)sc.v[t], src, 64);
      const float s = idle ? 1.f : e8m0((uint8_t)(sv >> (8 * g)));
#pragma unroll
      for (int d = 0; d < 4; ++d)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x[d]), cvt8(r.w[t][d], s), acc[t], 0, 0, 0);
    }
  };
  // two load rounds in flight: rounds 0 and 1 go out first; after the MFMAs of round i its buffer
  // takes round i + 2
  Round ra, rb;
  Scales sc, sn;
  if (nit > 0) {
    load_scales(sc, 0);
    load(ra, 0);
  }
  if (nit > 1) load(rb, 1);
#pragma unroll 1
  for (int it = 0; it < nit; it += 4) {
    if (it + 4 < nit) load_scales(sn, (it >> 2) + 1);
    mma(ra, sc, it);
    if (it + 2 < nit) load(ra, it + 2);
    if (it + 1 < nit) {
      mma(rb, sc, it + 1);
      if (it + 3 < nit) load(rb, it + 3);
    }
    if (it + 2 < nit) {
      mma(ra, sc, it + 2);
      if (it + 4 < nit) load(ra, it + 4);
    }
    if (it + 3 < nit) {
      mma(rb, sc, it + 3);
      if (it + 5 < nit) load(rb, it + 5);
    }
    sc = sn;
  }

  // K slices: summed into slice 0 in slice order
  if constexpr (KS > 1) {
    if (ks != 0) {
#pragma unroll
      for (int t = 0; t < NT; ++t) part[wid][t][lane] = acc[t];
    }
    __syncthreads();
    if (ks != 0) return;
#pragma unroll
    for (int j = 1; j < KS; ++j)
#pragma unroll
      for (int t = 0; t < NT; ++t) acc[t] += part[wid + j][t][lane];
  }
  if (!active) return;

  uint16_t* y = p.y + e * p.y_estride;
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t n = (int64_t)(tile0 + t) * 16 + c;
    if (n >= p.N) continue;
    float bg = 0.f, bu = 0.f;
    if (p.bias) {
      bg = bf2f(p.bias[n]);
      if (GLU) bu = bf2f(p.bias[n + p.N]);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 4 * g + i;
      if (m >= p.M) continue;
      float v = acc[t][i] + bg;
      if (GLU) {
        const float u = acc[T + t][i] + bu;
        v = v / (1.f + __expf(-v)) * u;
      }
      y[(int64_t)m * p.ldy + n] = f2bf(v);
    }
  }
}

// Tiles per wave and K split, from the sweep in profiles/LOG.md (MXFP4 on MFMA weight tiles): the
// most tiles per wave (shared activation loads) that still leaves 400 workgroups' worth of tile
// groups, and K split over all four waves of a workgroup (the finest grain: one tile group per
// workgroup, short waves, no tail of a few long ones) as long as a slice keeps 16 blocks.
static void pick(int64_t tiles, int KB, bool glu, int* T, int* KS) {
  int t = glu ? 2 : 4;
  while (t > 1 && tiles / t < 400) t >>= 1;
  int ks = 4;
  while (ks > 1 && KB / ks < 16) ks >>= 1;
  *T = t;
  *KS = ks;
}

template <int T, int KS, bool GLU>
static int launch_one(const Params& p, int E, hipStream_t s) {
  constexpr int G = 4 / KS;
  const int64_t groups = ((int64_t)(p.N + 15) / 16 + T - 1) / T;
  dim3 grid((unsigned)((groups + G - 1) / G), (unsigned)E), block(256);
  hipLaunchKernelGGL((mx_mfma_kernel<T, KS, GLU>), grid, block, 0, s, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <int T, bool GLU>
static int launch_ks(const Params& p, int E, int KS, hipStream_t s) {
  if (KS == 4) return launch_one<T, 4, GLU>(p, E, s);
  if (KS == 2) return launch_one<T, 2, GLU>(p, E, s);
  return launch_one<T, 1, GLU>(p, E, s);
}

}  // namespace gemv_mx_mfma

// Dense (E = 1, expert strides unused) or every expert of a stack (E experts, x shared when
// x_estride = 0).  cfg = 0 picks tiles per wave / K split by shape; cfg = 16 T + KS forces them (T in
// {1, 2, 4}, 4 only without glu; KS in {1, 2, 4}) for the benchmark tools.
int mx_mfma_launch(const void* x, int64_t ldx, int64_t x_estride, const void* w, int64_t ldw, int64_t w_estride,
                   const void* scale, int64_t lds, int64_t s_estride, const void* bias, int E, void* y, int64_t ldy,
                   int64_t y_estride, int M, int N, int K, int glu, int cfg, hipStream_t stream) {
  if (M < 1 || M > 16 || N < 1 || K < 32 || (K & 31) || E < 1 || E > 65535) return 2;
  gemv_mx_mfma::Params p{reinterpret_cast<const uint16_t*>(x), ldx, reinterpret_cast<const uint8_t*>(w), ldw,
                         reinterpret_cast<const uint8_t*>(scale), lds, reinterpret_cast<const uint16_t*>(bias),
                         reinterpret_cast<uint16_t*>(y), ldy, M, N, K, w_estride, s_estride, x_estride, y_estride};
  int T, KS;
  gemv_mx_mfma::pick((int64_t)((N + 15) / 16) * E, K >> 5, glu != 0, &T, &KS);
  if (cfg) {
    T = cfg >> 4;
    KS = cfg & 15;
    if ((T != 1 && T != 2 && T != 4) || (KS != 1 && KS != 2 && KS != 4) || (glu && T == 4)) return 2;
  }
  if (glu) {
    if (T == 2) return gemv_mx_mfma::launch_ks<2, true>(p, E, KS, stream);
    return gemv_mx_mfma::launch_ks<1, true>(p, E, KS, stream);
  }
  if (T == 4) return gemv_mx_mfma::launch_ks<4, false>(p, E, KS, stream);
  if (T == 2) return gemv_mx_mfma::launch_ks<2, false>(p, E, KS, stream);
  return gemv_mx_mfma::launch_ks<1, false>(p, E, KS, stream);
}

}  // namespace nxd
