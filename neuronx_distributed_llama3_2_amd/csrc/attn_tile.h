// The swizzled [rows][D] bf16 LDS image shared by the flash-attention forward and backward kernels
// (K / V / Q / dO tiles): D/8 16-byte chunks per row, serving both row reads (ds_read_b128) and
// transposed reads (ds_read_b64_tr_b16) without bank conflicts.  Device-only.
#pragma once
#include "gemm_tile.h"

namespace nxd {

// 16-byte chunk swizzle of a [rows][D] bf16 LDS image (D/8 chunks per row).
template <int D>
__device__ __forceinline__ int swz(int row, int ch) {
  if constexpr (D == 128) {
    return ch ^ (((row & 3) << 2) | ((row >> 2) & 3));
  } else {
    return ch ^ ((((row >> 1) & 1) << 2) | ((row >> 2) & 3));
  }
}

template <int D>
__device__ __forceinline__ int lds_off(int row, int ch) {  // byte offset of a 16-B chunk
  return row * (D * 2) + swz<D>(row, ch) * 16;
}

}  // namespace nxd
