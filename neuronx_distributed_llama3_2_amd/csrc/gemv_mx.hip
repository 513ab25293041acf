// MXFP4 weight-only decode: skinny GEMM y[M, N] = x[M, K] @ deq(W)[N, K]^T for M <= 8 reading the
// 4-bit weights directly, and the MXFP4 -> bf16 dequantisation for prefill-sized inputs.
//
// Format (OCP microscaling v1.0, see ops/gemv.py): a block is 32 consecutive elements along K;
// element = 4-bit e2m1 code s<<3 | i, i indexing {0, 0.5, 1, 1.5, 2, 3, 4, 6}; byte j of a row
// holds element 2j in its low nibble and 2j+1 in its high nibble (uint8 [N, K/2]); one E8M0 scale
// byte e per block, value 2^(e-127) (uint8 [N, K/32]).  4.25 bits per weight.
//
// One 16-byte lane load is exactly one block, so lane l of a wave owns block kb0 + l of its row and
// reads scale byte kb0 + l: the wave's scale read is one 64-byte line.  v_cvt_scalef32_pk_bf16_fp4
// turns one byte (two codes) and the block scale into two bf16 - exact, every e2m1 value has two
// significant bits - and the inner product against the bf16 activations runs on v_dot2c_f32_bf16
// with fp32 accumulation.  The weights are streamed non-temporal (each byte is read once), lanes
// are reduced with wave_sum; no atomics, so the result is deterministic.
#include <type_traits>

#include "common.h"

namespace nxd {
namespace gemv_mx {

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
static_assert(sizeof(Params) == 88 && alignof(Params) == 8, "Params layout: nine 8-byte fields, M / N / K, tail padding");

// 8 codes of one dword (element 2j = low nibble of byte j) times the block scale -> 4 bf16 pairs
struct W8 {
  bf16x2_t p[4];
};
__device__ __forceinline__ W8 cvt8(uint32_t d, float s) {
  W8 r;
  r.p[0] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0);
  r.p[1] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1);
  r.p[2] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2);
  r.p[3] = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3);
  return r;
}
__device__ __forceinline__ float dot8(const u32x4_t& x, const W8& w, float acc) {
  const bf16x8_t xv = __builtin_bit_cast(bf16x8_t, x);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(xv, xv, 0, 1), w.p[0], acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(xv, xv, 2, 3), w.p[1], acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(xv, xv, 4, 5), w.p[2], acc, false);
  acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_shufflevector(xv, xv, 6, 7), w.p[3], acc, false);
  return acc;
}

template <int MM, int ROWS, bool GLU>
__global__ void __launch_bounds__(256) mx_gemv_kernel(Params p) {
#include "gemv_mx_body.h"
}

// MoE experts: one product per blockIdx.y = pair, against expert e of a stack of E (codes w_estride
// bytes apart, scales s_estride bytes apart).  e = eidx[pair] (selective: P (token, expert-slot)
// pairs, M = 1, only the named experts' bytes are read) or e = pair (all experts, M <= 8 rows, each
// expert's bytes read once).  x rows of pair start at (pair / xdiv) * x_pair_stride elements, its y
// rows at pair * y_pair_stride.  An index outside [0, E) is clamped into the stack, never followed.
struct ExpertParams {
  Params g;              // pair 0 / expert 0 bases; bias is null
  const int32_t* eidx;   // [pairs] on the device, or null: expert = pair
  int64_t w_estride, s_estride;
  int64_t x_pair_stride, y_pair_stride;
  int E, xdiv;
};
static_assert(std::is_trivially_copyable<ExpertParams>::value && sizeof(ExpertParams) <= 4096, "kernel-argument struct");

template <int MM, int ROWS, bool GLU>
__global__ void __launch_bounds__(256) mx_expert_gemv_kernel(ExpertParams q) {
  const int pair = blockIdx.y;
  const int64_t e = q.eidx ? (int64_t)min(max(q.eidx[pair], 0), q.E - 1) : (int64_t)pair;
  Params p = q.g;
  p.w += e * q.w_estride;
  p.scale += e * q.s_estride;
  p.x += (int64_t)(pair / q.xdiv) * q.x_pair_stride;
  p.y += (int64_t)pair * q.y_pair_stride;
#include "gemv_mx_body.h"
}

// out_bf16[n, 32 kb .. 32 kb + 31] = deq(block kb of row n): one thread per 16-byte load
__global__ void __launch_bounds__(256) mx_dequant_kernel(const uint8_t* __restrict__ w, int64_t ldw,
                                                         const uint8_t* __restrict__ scale, int64_t lds,
                                                         uint16_t* __restrict__ out, int N, int K) {
  const int KB = K >> 5;
  const int64_t total = (int64_t)N * KB;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t n = i / KB;
    const int kb = (int)(i % KB);
    const u32x4_t v = *reinterpret_cast<const u32x4_t*>(w + n * ldw + (int64_t)kb * 16);
    const float s = e8m0(scale[n * lds + kb]);
    uint16_t* o = out + n * K + (int64_t)kb * 32;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      const W8 b = cvt8(v[d], s);
      u32x4_t q;
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = __builtin_bit_cast(uint32_t, b.p[j]);
      *reinterpret_cast<u32x4_t*>(o + 8 * d) = q;
    }
  }
}

// rows per wave: wide outputs take 2 (as the int8 kernel), and 4 when a row is at most one block
// per lane (K <= 2048), so that a wave still has several 16-byte loads in flight
static int rows_per_wave(int N, int K) { return N >= 8192 ? (K <= 2048 ? 4 : 2) : 1; }

template <int MM, bool GLU>
static int launch_m(const Params& p, hipStream_t s) {
  const int rows = rows_per_wave(p.N, p.K);
  const int waves = (p.N + rows - 1) / rows;
  dim3 grid((waves + 3) / 4), block(256);
  if (rows == 4)
    hipLaunchKernelGGL((mx_gemv_kernel<MM, 4, GLU>), grid, block, 0, s, p);
  else if (rows == 2)
    hipLaunchKernelGGL((mx_gemv_kernel<MM, 2, GLU>), grid, block, 0, s, p);
  else
    hipLaunchKernelGGL((mx_gemv_kernel<MM, 1, GLU>), grid, block, 0, s, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <bool GLU>
static int launch_t(const Params& p, hipStream_t s) {
  if (p.M <= 1) return launch_m<1, GLU>(p, s);
  if (p.M <= 2) return launch_m<2, GLU>(p, s);
  if (p.M <= 4) return launch_m<4, GLU>(p, s);
  if (p.M <= 8) return launch_m<8, GLU>(p, s);
  return 2;
}

template <int MM, bool GLU>
static int launch_expert_m(const ExpertParams& q, int pairs, hipStream_t s) {
  const int rows = rows_per_wave(q.g.N, q.g.K);
  const int waves = (q.g.N + rows - 1) / rows;
  dim3 grid((waves + 3) / 4, pairs), block(256);
  if (rows == 4)
    hipLaunchKernelGGL((mx_expert_gemv_kernel<MM, 4, GLU>), grid, block, 0, s, q);
  else if (rows == 2)
    hipLaunchKernelGGL((mx_expert_gemv_kernel<MM, 2, GLU>), grid, block, 0, s, q);
  else
    hipLaunchKernelGGL((mx_expert_gemv_kernel<MM, 1, GLU>), grid, block, 0, s, q);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <bool GLU>
static int launch_expert_t(const ExpertParams& q, int pairs, hipStream_t s) {
  if (q.g.M <= 1) return launch_expert_m<1, GLU>(q, pairs, s);
  if (q.g.M <= 2) return launch_expert_m<2, GLU>(q, pairs, s);
  if (q.g.M <= 4) return launch_expert_m<4, GLU>(q, pairs, s);
  if (q.g.M <= 8) return launch_expert_m<8, GLU>(q, pairs, s);
  return 2;
}

}  // namespace gemv_mx

int mx_gemv_rows_per_wave(int N, int K) { return gemv_mx::rows_per_wave(N, K); }

int mx_gemv_launch(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* scale, int64_t lds, const void* bias,
                   void* y, int64_t ldy, int M, int N, int K, int glu, hipStream_t stream) {
  if (M < 1 || N < 1 || K < 32 || (K & 31)) return 2;
  gemv_mx::Params p{reinterpret_cast<const uint16_t*>(x), ldx, reinterpret_cast<const uint8_t*>(w), ldw,
                    reinterpret_cast<const uint8_t*>(scale), lds, reinterpret_cast<const uint16_t*>(bias),
                    reinterpret_cast<uint16_t*>(y), ldy, M, N, K};
  return glu ? gemv_mx::launch_t<true>(p, stream) : gemv_mx::launch_t<false>(p, stream);
}

// MoE forms (see ExpertParams).  Selective: eidx [pairs] int32 on the device, M = 1.  All experts:
// eidx null, pairs = E, M <= 8 rows per expert, x shared (x_pair_stride 0) or per expert.
int mx_expert_gemv_launch(const void* x, int64_t ldx, int64_t x_pair_stride, const void* w, int64_t ldw, int64_t w_estride,
                          const void* scale, int64_t lds, int64_t s_estride, const int32_t* eidx, int E, int pairs, int xdiv,
                          void* y, int64_t ldy, int64_t y_pair_stride, int M, int N, int K, int glu, hipStream_t stream) {
  if (M < 1 || N < 1 || K < 32 || (K & 31) || E < 1 || pairs < 1 || pairs > 65535 || xdiv < 1) return 2;
  if (!eidx && pairs > E) return 2;
  gemv_mx::ExpertParams q{{reinterpret_cast<const uint16_t*>(x), ldx, reinterpret_cast<const uint8_t*>(w), ldw,
                           reinterpret_cast<const uint8_t*>(scale), lds, nullptr, reinterpret_cast<uint16_t*>(y), ldy, M, N, K},
                          eidx, w_estride, s_estride, x_pair_stride, y_pair_stride, E, xdiv};
  return glu ? gemv_mx::launch_expert_t<true>(q, pairs, stream) : gemv_mx::launch_expert_t<false>(q, pairs, stream);
}

int mx_dequant_launch(const void* w, int64_t ldw, const void* scale, int64_t lds, void* out, int N, int K,
                      hipStream_t stream) {
  if (N < 1 || K < 32 || (K & 31)) return 2;
  const int64_t total = (int64_t)N * (K / 32);
  const int64_t g = (total + 255) / 256;
  const int grid = (int)(g < 8192 ? g : 8192);
  hipLaunchKernelGGL(gemv_mx::mx_dequant_kernel, dim3(grid), dim3(256), 0, stream, reinterpret_cast<const uint8_t*>(w),
                     ldw, reinterpret_cast<const uint8_t*>(scale), lds, reinterpret_cast<uint16_t*>(out), N, K);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

}  // namespace nxd
