// MXFP8 KV cache (format: ops/decode.py): the quantizing cache write and the codes -> bf16
// dequantisation the decode-attention fallbacks use.
//
// Codes are OCP FP8 E4M3 bytes in the bf16 cache's shape [Bc, Hkv, Lmax, D]; one E8M0 scale byte e
// (value 2^(e-127)) per 32 consecutive elements of a head vector, [Bc, Hkv, Lmax, D/32].
//
// kv_write_mx8: one thread per (k | v, batch, token, kv head, 32-element block).  It loads the
// block's 64 bytes with four 16-byte loads from the strided [B, T, Hkv, D] view (a slice of the
// fused QKV buffer), takes amax on the magnitude bits (monotonic for finite bf16), derives the block
// exponent from amax's exponent field -- floor(log2(amax)) - 8 is field - 135, so the scale byte is
// field - 8 clamped to [1, 254], 127 for an all-zero block -- and converts pairs with
// v_cvt_scalef32_pk_fp8_bf16, which DIVIDES the source by the scale operand (the float whose
// exponent field is e), rounds to nearest even and saturates.  The saturation does not rest on
// the instruction: every magnitude is first clamped, on its bits, to 448 * 2^(e-127) (exactly
// representable in bf16: exponent field e + 8, mantissa 1.75), which also turns a non-finite input
// into a finite one, so no NaN code is ever written.  32 code bytes leave as two 16-byte stores,
// then the scale byte.
//
// mx8_dequant: code * 2^(e-127) by v_cvt_scalef32_pk_bf16_fp8 (multiplies by the scale operand);
// exact, every product has at most four significant bits.
#include "common.h"

namespace nxd {
namespace kvmx {

typedef short short2_t __attribute__((ext_vector_type(2)));

// 4 codes (one dword) from 4 bf16 (two dwords of pairs), divided by `scale`
__device__ __forceinline__ uint32_t cvt4_fp8(uint32_t p01, uint32_t p23, float scale) {
  short2_t r = {0, 0};
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(r, __builtin_bit_cast(bf16x2_t, p01), scale, false);
  r = __builtin_amdgcn_cvt_scalef32_pk_fp8_bf16(r, __builtin_bit_cast(bf16x2_t, p23), scale, true);
  return __builtin_bit_cast(uint32_t, r);
}

// both halves of a bf16 pair clamped in magnitude to `lim` (bf16 bits, sign clear)
__device__ __forceinline__ uint32_t clamp_pair(uint32_t p, uint32_t lim) {
  const uint32_t lo = min(p & 0x7fffu, lim) | (p & 0x8000u);
  const uint32_t hi = min((p >> 16) & 0x7fffu, lim) | ((p >> 16) & 0x8000u);
  return lo | (hi << 16);
}

__global__ void __launch_bounds__(256) kv_write_mx8_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v,
                                                           int64_t n_sb, int64_t n_st, int64_t n_sh,
                                                           uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                           uint8_t* __restrict__ ks, uint8_t* __restrict__ vs,
                                                           const int* __restrict__ cache_idx, const int* __restrict__ pos,
                                                           int B, int Bc, int T, int H, int D, int Lmax) {
  const int nb = D / 32;
  const int64_t half = (int64_t)B * T * H * nb, total = 2 * half;
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + threadIdx.x; i0 < total; i0 += (int64_t)gridDim.x * 256) {
    const bool is_v = i0 >= half;
    const int64_t i = is_v ? i0 - half : i0;
    const int j = i % nb;
    const int h = (i / nb) % H;
    const int t = (i / ((int64_t)nb * H)) % T;
    const int b = i / ((int64_t)nb * H * T);
    const int cb = cache_idx ? cache_idx[b] : b;
    const int ps = pos[b] + t;
    if (ps < 0 || ps >= Lmax || cb < 0 || cb >= Bc) continue;   // dropped, never out of bounds
    const uint16_t* src = (is_v ? v : k) + (int64_t)b * n_sb + (int64_t)t * n_st + (int64_t)h * n_sh + 32 * j;
    u32x4_t x[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) x[q] = *reinterpret_cast<const u32x4_t*>(src + 8 * q);
    uint32_t amax = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
      for (int d = 0; d < 4; ++d) amax = max(amax, max(x[q][d] & 0x7fffu, (x[q][d] >> 16) & 0x7fffu));
    int e = (int)(amax >> 7) - 8;
    e = amax == 0 ? 127 : (e < 1 ? 1 : (e > 254 ? 254 : e));
    const uint32_t lim = ((uint32_t)min(e + 8, 254) << 7) | 0x60u;   // 448 * 2^(e-127)
    const float scale = e8m0((uint8_t)e);
    u32x4_t c[2];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      c[q >> 1][2 * (q & 1)] = cvt4_fp8(clamp_pair(x[q][0], lim), clamp_pair(x[q][1], lim), scale);
      c[q >> 1][2 * (q & 1) + 1] = cvt4_fp8(clamp_pair(x[q][2], lim), clamp_pair(x[q][3], lim), scale);
    }
    const int64_t row = ((int64_t)cb * H + h) * Lmax + ps;   // caches are contiguous
    uint8_t* dst = (is_v ? vc : kc) + row * D + 32 * j;
    *reinterpret_cast<u32x4_t*>(dst) = c[0];
    *reinterpret_cast<u32x4_t*>(dst + 16) = c[1];
    (is_v ? vs : ks)[row * nb + j] = (uint8_t)e;
  }
}

// 8 codes per thread: codes [R0, R1, R2, D] with strides (c_s0, c_s1, c_s2, 1), scales likewise with
// D / 32 columns, out contiguous bf16.  ALIGNED: every 8-code group is 8-byte aligned (one load).
template <bool ALIGNED>
__global__ void __launch_bounds__(256) mx8_dequant_kernel(const uint8_t* __restrict__ codes, int64_t c_s0, int64_t c_s1,
                                                          int64_t c_s2, const uint8_t* __restrict__ scale, int64_t s_s0,
                                                          int64_t s_s1, int64_t s_s2, uint16_t* __restrict__ out, int64_t R0,
                                                          int64_t R1, int64_t R2, int D) {
  const int ng = D / 8;
  const int64_t total = R0 * R1 * R2 * ng;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int c = i % ng;
    const int64_t r2 = (i / ng) % R2, r1 = (i / ((int64_t)ng * R2)) % R1, r0 = i / ((int64_t)ng * R2 * R1);
    const uint8_t* src = codes + r0 * c_s0 + r1 * c_s1 + r2 * c_s2 + 8 * c;
    uint32_t d0, d1;
    if (ALIGNED) {
      const u32x2_t w = *reinterpret_cast<const u32x2_t*>(src);
      d0 = w[0];
      d1 = w[1];
    } else {
      d0 = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | ((uint32_t)src[3] << 24);
      d1 = (uint32_t)src[4] | ((uint32_t)src[5] << 8) | ((uint32_t)src[6] << 16) | ((uint32_t)src[7] << 24);
    }
    const float s = e8m0(scale[r0 * s_s0 + r1 * s_s1 + r2 * s_s2 + c / 4]);
    u32x4_t o;
    o[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, s, false));
    o[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d0, s, true));
    o[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, s, false));
    o[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d1, s, true));
    *reinterpret_cast<u32x4_t*>(out + i * 8) = o;
  }
}

}  // namespace kvmx

// k, v: bf16 [B, T, H, D] views with strides ns (elements; 16-byte aligned rows); caches uint8
// contiguous [Bc, H, Lmax, D] with scales [Bc, H, Lmax, D / 32]; D % 32 == 0.
int kv_write_mx8_launch(const void* k, const void* v, const int64_t* ns, void* kc, void* vc, void* ks, void* vs,
                        const int* cache_idx, const int* pos, int B, int Bc, int T, int H, int D, int Lmax, hipStream_t stream) {
  if (D <= 0 || D % 32) return -1;
  const int64_t total = (int64_t)2 * B * T * H * (D / 32);
  if (total == 0) return 0;
  int64_t g = (total + 255) / 256;
  if (g > 4096) g = 4096;
  hipLaunchKernelGGL(kvmx::kv_write_mx8_kernel, dim3((unsigned)g), dim3(256), 0, stream, (const uint16_t*)k, (const uint16_t*)v,
                     ns[0], ns[1], ns[2], (uint8_t*)kc, (uint8_t*)vc, (uint8_t*)ks, (uint8_t*)vs, cache_idx, pos, B, Bc, T, H,
                     D, Lmax);
  return (int)hipGetLastError();
}

// codes / scale: uint8 [R0, R1, R2, D] / [R0, R1, R2, D / 32] with strides cs / ss (bytes, unit inner
// stride); out: contiguous bf16 [R0, R1, R2, D], 16-byte aligned.
int mx8_dequant_launch(const void* codes, const int64_t* cs, const void* scale, const int64_t* ss, void* out, int64_t R0,
                       int64_t R1, int64_t R2, int D, hipStream_t stream) {
  if (D <= 0 || D % 32) return -1;
  const int64_t total = R0 * R1 * R2 * (D / 8);
  if (total == 0) return 0;
  int64_t g = (total + 255) / 256;
  if (g > 65536) g = 65536;
  const bool aligned = reinterpret_cast<uintptr_t>(codes) % 8 == 0 && cs[0] % 8 == 0 && cs[1] % 8 == 0 && cs[2] % 8 == 0;
  if (aligned)
    hipLaunchKernelGGL(kvmx::mx8_dequant_kernel<true>, dim3((unsigned)g), dim3(256), 0, stream, (const uint8_t*)codes, cs[0],
                       cs[1], cs[2], (const uint8_t*)scale, ss[0], ss[1], ss[2], (uint16_t*)out, R0, R1, R2, D);
  else
    hipLaunchKernelGGL(kvmx::mx8_dequant_kernel<false>, dim3((unsigned)g), dim3(256), 0, stream, (const uint8_t*)codes, cs[0],
                       cs[1], cs[2], (const uint8_t*)scale, ss[0], ss[1], ss[2], (uint16_t*)out, R0, R1, R2, D);
  return (int)hipGetLastError();
}

}  // namespace nxd
