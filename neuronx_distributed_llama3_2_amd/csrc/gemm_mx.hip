// MXFP4 weight-only projections at 17..512 activation rows, straight from the 4-bit weights:
// y[M, N] = x[M, K] @ deq(W)[Nw, K]^T with optional bias and fused SwiGLU (ops.gemv.mx_linear above
// the 16 rows of gemv_mx_mfma.hip).  The format is that of gemv_mx.hip / ops/gemv.py.
//
// Weights are read as in gemv_mx_mfma.hip: lane l works on weight row n0 + (l & 15); one 16-byte
// load is one 32-element block of that row and cvt8 of dword d of the block is the B operand of MFMA
// d of v_mfma_f32_16x16x32_bf16; lane group g = l >> 4 takes block 4 i + g of iteration i (a legal
// permutation of k, since both operands of a lane carry the same 8 k-indices).  What differs is the
// A side.  There the 16 activation rows live in registers; here a workgroup owns a row chunk of
// MC = 16 MT rows (MT = 4 or 8 row tiles) and
//   * the converted B operands of an iteration (NT weight tiles x 4 dwords) are reused by every row
//     tile of the chunk, so converts per MFMA fall as 1 / (row tiles in use) instead of staying 1:1;
//   * the chunk's activations for the iteration (rows x 128 k per K slice) are staged once per
//     workgroup in LDS and shared by its four waves, which split N (and K, below);
//   * row tiles wholly past M are skipped (a wave-uniform branch), so 17..32 rows cost two tiles;
//   * accumulators are MT x NT x 4 registers per lane (128 at MT 8, NT 4; the allocator puts them in
//     AGPRs, profiles/mxfp4_wide_kernel_resources.txt).
// M above MC runs as further chunks on blockIdx.x (the fastest grid axis, so the chunks of one weight
// tile group are dispatched together and all but the first find the weights in cache).
//
// Staging: global loads into registers, then ds_write_b128, not LDS-DMA.  A DMA load writes a wave's
// 64 dwords to consecutive LDS addresses, so it cannot apply the per-row swizzle below nor the zero
// fill of the K tail and of the rows past M; the register route does both for free, and its loads
// for stage s + 2 are issued before the MFMAs of stage s, so they are in flight under the MFMAs.
// LDS holds two stages: stage s + 1 is written while stage s is read, one barrier per stage.
// LDS layout: a row is KS x 256 bytes = 16 KS chunks of 16 bytes, chunk j of row r stored at chunk
// j ^ (r & 15).  The A fragment of MFMA d is one ds_read_b128: row 16 mt + (l & 15), chunk
// 4 (4 ks + g) + d.  Unswizzled, the 16 lanes of a lane group would read the same 4 banks of 16
// rows (a 16-way conflict at the 256-byte pitch); swizzled they read 16 different chunks = all 64
// banks: designed for 0 conflicts on the reads, and the writes (16 consecutive lanes fill the 16
// chunks of one row) are conflict-free as well.
//
// KS = 2: the two waves of a pair take the two 128-k halves of every 256-k stage (narrow outputs
// leave too few tile groups for 256 CUs); the partial sums go through LDS and are added in slice
// order: no atomics, two calls give the same bits.
// Guards: lane groups whose block is past K contribute exact zeros on both operands and do not load;
// rows past M are neither read (their LDS rows are zeros) nor stored; weight rows past N are clamped
// and their columns not stored.  GLU keeps the gate tile and the up tile of the same 16 columns as
// two accumulator sets, so the epilogue is lane-local.
#include <type_traits>

#include "common.h"

namespace nxd {
namespace gemm_mx {

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

// MT row tiles of 16 per workgroup, T output tiles of 16 columns per wave (GLU: T gate + T up weight
// tiles), KS waves per tile group splitting K
template <int MT, int T, int KS, bool GLU>
__global__ void __launch_bounds__(256) mx_wide_kernel(Params p) {
  constexpr int NT = GLU ? 2 * T : T;   // weight tiles per wave
  constexpr int G = 4 / KS;             // tile groups per workgroup
  constexpr int MC = 16 * MT;           // rows per workgroup
  constexpr int RC = 16 * KS;           // 16-byte chunks per staged row
  constexpr int STAGE = MC * RC * 16;   // bytes per stage
  constexpr int XL = MC * RC / 256;     // staging loads per thread and stage
  static_assert(2 * STAGE <= 65536 && (KS - 1) * G * MT * NT * 1024 <= 2 * STAGE, "LDS budget");
  __shared__ __attribute__((aligned(16))) uint8_t smem[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rg = wid / KS, ks = wid % KS;
  const int c = lane & 15, g = lane >> 4;
  const int m0 = (int)blockIdx.x * MC;
  const int rows = min(MC, p.M - m0);   // >= 1 by the grid
  const int tile0 = ((int)blockIdx.y * G + rg) * T;
  const bool active = (int64_t)tile0 * 16 < p.N;   // wave-uniform; an idle wave still stages and syncs

  const uint8_t* wr[NT];
  const uint8_t* sr[NT];
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t n = min((int64_t)(tile0 + t) * 16 + c, (int64_t)p.N - 1);   // rows past N are clamped (and not stored)
    wr[t] = p.w + n * p.ldw;
    sr[t] = p.scale + n * p.lds;
    if (GLU) {
      wr[T + t] = wr[t] + (int64_t)p.N * p.ldw;
      sr[T + t] = sr[t] + (int64_t)p.N * p.lds;
    }
  }

  const int KB = p.K >> 5;                         // blocks per row
  const int ns = (KB + 4 * KS - 1) / (4 * KS);     // stages of KS x 128 k, the same for every wave

  f32x4_t acc[MT][NT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt)
#pragma unroll
    for (int t = 0; t < NT; ++t) acc[mt][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // activations: thread tid moves chunk L % RC of row L / RC for L = 256 q + tid; blocks past K and
  // rows past M are zeros, not loads
  const uint16_t* xbase = p.x + (int64_t)m0 * p.ldx;
  auto gload = [&](u32x4_t (&xr)[XL], int s) {
#pragma unroll
    for (int q = 0; q < XL; ++q) {
      const int L = 256 * q + tid, r = L / RC, ch = L % RC;
      xr[q] = u32x4_t{0u, 0u, 0u, 0u};
      if (r < rows && 4 * KS * s + (ch >> 2) < KB)
        xr[q] = *reinterpret_cast<const u32x4_t*>(xbase + (int64_t)r * p.ldx + (int64_t)s * (128 * KS) + 8 * ch);
    }
  };
  auto swrite = [&](const u32x4_t (&xr)[XL], int buf) {
#pragma unroll
    for (int q = 0; q < XL; ++q) {
      const int L = 256 * q + tid, r = L / RC, ch = L % RC;
      *reinterpret_cast<u32x4_t*>(smem + buf * STAGE + r * (RC * 16) + ((ch ^ (r & 15)) << 4)) = xr[q];
    }
  };

  // Scales as in gemv_mx_mfma.hip: once per 4 stages lane (c, g) loads the 4 scale bytes of this
  // wave's blocks of stage 4 I + g as one dword (any alignment); stage 4 I + q then takes byte g of
  // the dword of lane (c, q) with one ds_bpermute.  A dword that would pass the end of the row is
  // put together from the bytes inside it.
  struct Scales {
    uint32_t v[NT];
  };
  auto load_scales = [&](Scales& sc, int I) {
    const int b = 4 * KS * (4 * I + g) + 4 * ks;
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
  struct Round {
    u32x4_t w[NT];
  };
  auto wload = [&](Round& r, int s) {
    const int kb = 4 * KS * s + 4 * ks + g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {   // idle lane group: +0 codes (its activations are zeros in LDS)
      r.w[t] = u32x4_t{0u, 0u, 0u, 0u};
      if (kb < KB) r.w[t] = *reinterpret_cast<const u32x4_t*>(wr[t] + (int64_t)kb * 16);
    }
  };
  auto mma = [&](const Round& r, const Scales& sc, int s, int buf) {
    const bool idle = 4 * KS * s + 4 * ks + g >= KB;   // scale 1 for the zero codes of an idle lane group
    const int src = c + 16 * (s & 3);
    bf16x8_t b[NT][4];   // converted once, used by every row tile
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint32_t sv = (uint32_t)__shfl((int)sc.v[t], src, 64);
      const float sf = idle ? 1.f : e8m0((uint8_t)(sv >> (8 * g)));
#pragma unroll
      for (int d = 0; d < 4; ++d) b[t][d] = cvt8(r.w[t][d], sf);
    }
    const uint8_t* arow = smem + buf * STAGE + c * (RC * 16);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      if (16 * mt < rows) {   // wave-uniform: row tiles wholly past M do no work
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const int ch = 4 * (4 * ks + g) + d;
          const bf16x8_t a = *reinterpret_cast<const bf16x8_t*>(arow + mt * (16 * RC * 16) + ((ch ^ c) << 4));
#pragma unroll
          for (int t = 0; t < NT; ++t) acc[mt][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b[t][d], acc[mt][t], 0, 0, 0);
        }
      }
    }
  };

  // Stage s: LDS buffer s & 1 holds its activations, xr those of stage s + 1 (loaded one stage ago),
  // and the weights of stages s and s + 1 are in the two Rounds.  Buffer (s + 1) & 1 was last read in
  // stage s - 1, which ended in a barrier.  (Fetching the activations three stages and the weights
  // four stages ahead was measured and lost at every shape: it costs 40-120 VGPRs, and the waves per
  // SIMD that go with them hide more latency than the deeper queue, profiles/LOG.md.)
  u32x4_t xr[XL];
  Round ra, rb;
  Scales sc, sn;
  auto step = [&](Round& r, int s, int buf) {
    if (s + 1 < ns) swrite(xr, buf ^ 1);
    if (s + 2 < ns) gload(xr, s + 2);
    if (active) {
      mma(r, sc, s, buf);
      if (s + 2 < ns) wload(r, s + 2);
    }
    __syncthreads();
  };
  gload(xr, 0);
  swrite(xr, 0);
  if (ns > 1) gload(xr, 1);
  if (active) {
    load_scales(sc, 0);
    wload(ra, 0);
    if (ns > 1) wload(rb, 1);
  }
  __syncthreads();
#pragma unroll 1
  for (int s = 0; s < ns; s += 4) {   // ns is the same for the whole workgroup, so are the barriers
    if (active && s + 4 < ns) load_scales(sn, (s >> 2) + 1);
    step(ra, s, 0);
    if (s + 1 < ns) step(rb, s + 1, 1);
    if (s + 2 < ns) step(ra, s + 2, 0);
    if (s + 3 < ns) step(rb, s + 3, 1);
    sc = sn;
  }

  // K slices: summed into slice 0 in slice order, through the staging LDS (every read of it is
  // behind the last barrier)
  if constexpr (KS > 1) {
    f32x4_t* part = reinterpret_cast<f32x4_t*>(smem);
    if (ks != 0) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < NT; ++t) part[(((rg * (KS - 1) + ks - 1) * MT + mt) * NT + t) * 64 + lane] = acc[mt][t];
    }
    __syncthreads();
    if (ks != 0) return;
#pragma unroll
    for (int j = 1; j < KS; ++j)
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[mt][t] += part[(((rg * (KS - 1) + j - 1) * MT + mt) * NT + t) * 64 + lane];
  }
  if (!active) return;

  // C: lane l holds rows 4 (l >> 4) + i of column l & 15 of each 16 x 16 tile
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
    for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 16 * mt + 4 * g + i;
        if (m >= rows) continue;
        float v = acc[mt][t][i] + bg;
        if (GLU) {
          const float u = acc[mt][T + t][i] + bu;
          v = v / (1.f + __expf(-v)) * u;
        }
        p.y[(int64_t)(m0 + m) * p.ldy + n] = f2bf(v);
      }
    }
  }
}

// The instantiation by shape, from the sweep of all six over the projection shapes of
// tools/bench_mx_gemv.py at 17, 64, 128 and 512 rows (profiles/LOG.md).  The kernel is bound by the
// loads in flight, so the count of workgroups decides before anything else:
//   * 128-row chunks (half the passes over the weights, no K split for want of LDS) only where they
//     still leave 512 workgroups, with 2 tiles per wave if that does;
//   * else 64-row chunks: 2 tiles per wave from 1024 workgroups of one tile per wave on, 1 tile from
//     400 on unless K is long (8192 or more, where two short K slices beat one long one);
//   * else K split over wave pairs, with 2 tiles per wave if 300 workgroups remain.
static void pick(int M, int64_t tiles, int KB, int* MT, int* T, int* KS) {
  const int64_t c8 = (M + 127) / 128, c4 = (M + 63) / 64;
  const int64_t w1 = c4 * ((tiles + 3) / 4);   // workgroups at 64 rows, 1 tile per wave, no K split
  *MT = 4;
  *T = 1;
  *KS = 1;
  if (M > 64 && c8 * ((tiles + 7) / 8) >= 512) {
    *MT = 8;
    *T = 2;
  } else if (M > 64 && c8 * ((tiles + 3) / 4) >= 512) {
    *MT = 8;
  } else if (w1 >= 1024) {
    *T = 2;
  } else if (w1 < 400 || KB >= 256) {
    *KS = 2;
    *T = w1 >= 300 ? 2 : 1;
  }
}

template <int MT, int T, int KS, bool GLU>
static int launch_one(const Params& p, hipStream_t s) {
  constexpr int G = 4 / KS;
  const int64_t groups = ((int64_t)(p.N + 15) / 16 + T - 1) / T;
  dim3 grid((unsigned)((p.M + 16 * MT - 1) / (16 * MT)), (unsigned)((groups + G - 1) / G)), block(256);
  if (grid.y > 65535) return 2;
  hipLaunchKernelGGL((mx_wide_kernel<MT, T, KS, GLU>), grid, block, 0, s, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <bool GLU>
static int launch_cfg(const Params& p, int MT, int T, int KS, hipStream_t s) {
  if (MT == 8) return T == 2 ? launch_one<8, 2, 1, GLU>(p, s) : launch_one<8, 1, 1, GLU>(p, s);
  if (KS == 2) return T == 2 ? launch_one<4, 2, 2, GLU>(p, s) : launch_one<4, 1, 2, GLU>(p, s);
  return T == 2 ? launch_one<4, 2, 1, GLU>(p, s) : launch_one<4, 1, 1, GLU>(p, s);
}

}  // namespace gemm_mx

// cfg = 0 picks row tiles per workgroup / output tiles per wave / K split by shape; cfg = 256 MT +
// 16 T + KS forces them (MT in {4, 8}, T in {1, 2}, KS in {1, 2}, KS = 2 only with MT = 4) for the
// tests and the benchmark tool.  Returns 2 for arguments it does not serve.
int mx_wide_launch(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* scale, int64_t lds, const void* bias,
                   void* y, int64_t ldy, int M, int N, int K, int glu, int cfg, hipStream_t stream) {
  if (M < 1 || M > 512 || N < 1 || K < 32 || (K & 31)) return 2;
  gemm_mx::Params p{reinterpret_cast<const uint16_t*>(x), ldx, reinterpret_cast<const uint8_t*>(w), ldw,
                    reinterpret_cast<const uint8_t*>(scale), lds, reinterpret_cast<const uint16_t*>(bias),
                    reinterpret_cast<uint16_t*>(y), ldy, M, N, K};
  int MT, T, KS;
  gemm_mx::pick(M, (N + 15) / 16, K >> 5, &MT, &T, &KS);
  if (cfg) {
    MT = cfg >> 8;
    T = (cfg >> 4) & 15;
    KS = cfg & 15;
    if ((MT != 4 && MT != 8) || (T != 1 && T != 2) || (KS != 1 && KS != 2) || (MT == 8 && KS == 2)) return 2;
  }
  return glu ? gemm_mx::launch_cfg<true>(p, MT, T, KS, stream) : gemm_mx::launch_cfg<false>(p, MT, T, KS, stream);
}

}  // namespace nxd
