// LDS / LDS-DMA plumbing shared by the hand-written GEMM kernels (dense_gemm, wgrad_gemm,
// grouped_rowgemm, grouped_gemm) and, for the address helpers, the flash-attention kernels.
// Device-only.  Each kernel keeps its own tile constants, Params, source addressing and epilogue.
#pragma once
#include "common.h"

namespace nxd {

typedef __attribute__((address_space(3))) char lds_char_t;
typedef __attribute__((address_space(3))) short4_t lds_short4_t;

// 32-bit LDS byte address of a pointer into __shared__ memory
__device__ __forceinline__ uint32_t lds_addr(const char* q) { return (uint32_t)(uintptr_t)(const lds_char_t*)q; }

// One 1 KiB LDS-DMA piece (global_load_lds_dwordx4, 16 B per lane, written lane-linearly) at the
// wave-uniform LDS address `lds_dst`; M0 carries the destination and is restored.  Inline asm so
// the compiler does not wait for it (vmcnt(0)) before every later LDS read: completion is the
// caller's counted s_waitcnt vmcnt.  An LDS swizzle is applied to each lane's SOURCE address.
__device__ __forceinline__ void dma16(const void* src, uint32_t lds_dst) {
  uint32_t sv;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(sv) : "v"(src), "s"(lds_dst) : "memory");
}

// s_barrier the scheduler moves nothing across
__device__ __forceinline__ void barrier() {
  __builtin_amdgcn_sched_barrier(0);
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_sched_barrier(0);
}

// L2-aware raster: walk the (row tile, column tile) grid in bands of `band` row tiles, column-major
// inside a band, so the workgroups resident on one XCD at a time (consecutive ids after
// xcd_remap) share both A row tiles and B column tiles in that XCD's 4 MiB L2.  Row-major order
// re-streams the whole B operand from HBM once per row tile.
__device__ __forceinline__ void band_raster(int id, int rows, int cols, int band, int& r, int& c) {
  const int bnd = id / (band * cols), within = id - bnd * band * cols;
  const int h = min(band, rows - bnd * band);
  r = bnd * band + within % h;
  c = within / h;
}

// Token-major image [tokens][features], PITCH-byte rows: 16-B chunk c of token row t is stored at
// c ^ tok_swz(t).  The two 16-lane groups of a transposed read (4 token rows x 16 features each,
// rows t and t + 8) land on 16 distinct bank quads -- conflict-free.
__device__ __forceinline__ int tok_swz(int t) { return 2 * ((t & 3) | (((t >> 3) & 1) << 2)); }

// 16x16x32 operand fragment of features [c0, c0 + 16), tokens [t0, t0 + 32) of such an image: lane l
// holds feature c0 + (l & 15) at tokens t0 + 8 (l >> 4) + j, j = 0..7 -- two ds_read_b64_tr_b16,
// each a block of 4 token rows x 16 features per 16-lane group (lane 4q + p supplies row q,
// features 4p .. 4p + 3).
template <int PITCH>
__device__ __forceinline__ bf16x8_t frag_tr16(const char* img, int c0, int t0) {
  const int l = threadIdx.x & 63, g = l >> 4, i = l & 15, q = i >> 2, p = i & 3;
  const int col = c0 + 4 * p, t = t0 + 8 * g + q;
  const char* b0 = img + t * PITCH + 16 * ((col >> 3) ^ tok_swz(t)) + 8 * (p & 1);
  const char* b1 = img + (t + 4) * PITCH + 16 * ((col >> 3) ^ tok_swz(t + 4)) + 8 * (p & 1);
  const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_t*)b0);
  const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4_t*)b1);
  const short __attribute__((ext_vector_type(8))) a8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, a8);
}

}  // namespace nxd
