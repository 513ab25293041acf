// Launchers of the fused decode GEMVs over MXFP4 weights (decode_fused_mx.hip: 1-3 rows, decode_fused_mx_mfma.hip:
// 4-16 rows) and the operands of their QKV form (epi = 3: RoPE + KV-cache write).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace nxd {

struct DgemvMxRope {
  int nq, nkv, D;           // y rows hold [nq | nkv | nkv] heads of D
  const float* cos_t;       // fp32 [max_pos, D/2]
  const float* sin_t;
  const int64_t* pos;       // [M] absolute position of each row
  int T;                    // rows per sequence (cache row = cache_idx[m / T] or m / T)
  void* kc;                 // bf16 caches [B, nkv, Lmax, D] with the strides below (elements), unit inner stride
  void* vc;
  int64_t c_sb, c_sh, c_sl;
  const int* cache_idx;     // [M / T], nullable
  int Lmax, max_pos;
  const int64_t* xidx;      // nullable; else x is the embedding table [xrows, K] and row m is x[xidx[m]]
  int64_t xrows;
  void* xcopy;              // nullable; bf16 [M, K] contiguous, receives the gathered rows
};

int dgemv_mx_launch(int epi, const void* x, int64_t ldx, const void* norm_w, float eps, const void* w, int64_t ldw,
                    const void* scale, int64_t lds, void* y, int64_t ldy, int M, int N, int K, int cfg, hipStream_t stream,
                    const DgemvMxRope* rope = nullptr);
int dgemv_mx_mfma_launch(int epi, const void* x, int64_t ldx, const void* norm_w, float eps, const void* w, int64_t ldw,
                         const void* scale, int64_t lds, void* y, int64_t ldy, int M, int N, int K, int cfg,
                         hipStream_t stream, const DgemvMxRope* rope = nullptr);

}  // namespace nxd
