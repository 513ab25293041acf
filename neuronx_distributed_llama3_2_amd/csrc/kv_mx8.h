// Device pieces of the MXFP8 KV-cache quantizer (format: ops/decode.py), shared by the quantizing cache
// write (kv_cache_mx.hip) and the append form of the decode-attention kernel (decode_attn.hip), so both
// give the same bytes for the same bf16 block.
#pragma once

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

// largest magnitude (bf16 bits, sign clear) among the 8 bf16 of a 16-byte load
__device__ __forceinline__ uint32_t amax8(const u32x4_t& x) {
  uint32_t a = 0;
#pragma unroll
  for (int d = 0; d < 4; ++d) a = max(a, max(x[d] & 0x7fffu, (x[d] >> 16) & 0x7fffu));
  return a;
}

// E8M0 scale byte of a block whose largest magnitude is `amax` (bf16 bits): exponent field - 8 clamped
// to [1, 254], 127 for an all-zero block
__device__ __forceinline__ int block_exp(uint32_t amax) {
  const int e = (int)(amax >> 7) - 8;
  return amax == 0 ? 127 : (e < 1 ? 1 : (e > 254 ? 254 : e));
}

// 8 bf16 (one 16-byte load) of a block with scale byte e -> 8 codes: clamped to 448 * 2^(e-127), divided
// by the scale, rounded to nearest even
__device__ __forceinline__ u32x2_t quant8(const u32x4_t& x, int e) {
  const uint32_t lim = ((uint32_t)min(e + 8, 254) << 7) | 0x60u;   // 448 * 2^(e-127)
  const float scale = e8m0((uint8_t)e);
  return u32x2_t{cvt4_fp8(clamp_pair(x[0], lim), clamp_pair(x[1], lim), scale),
                 cvt4_fp8(clamp_pair(x[2], lim), clamp_pair(x[3], lim), scale)};
}

}  // namespace kvmx
}  // namespace nxd
