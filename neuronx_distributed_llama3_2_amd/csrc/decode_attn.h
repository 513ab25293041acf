// The one description of a decode-attention call, and the only prototypes of its launchers
// (decode_attn.hip, inference.hip) and their switches.  Included by both and by bindings.cpp, so the
// compiler checks every definition and every call against the same declaration.  HIP runtime header
// only: the kernel translation units stay free of torch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nxd {

// Callers value-initialise (`DecodeAttnArgs a{};`) and set what the call has: an unset field is
// zero / null, which every launcher reads as "absent".
struct DecodeAttnArgs {
  const void* q;                 // bf16 [B, T, Hq, D], unit stride on D
  int64_t q_sb, q_st, q_sh;      // element strides of batch, token, head
  const void* kc;                // caches [Bc, Hkv, Lmax, D]: bf16, or the E4M3 code bytes of an MXFP8 cache
  const void* vc;
  int64_t c_sb, c_sh, c_sl;      // element strides of cache row, kv head, key (bytes for codes)
  const void* ksc;               // MXFP8 cache: E8M0 scale bytes [Bc, Hkv, Lmax, D / 32]; null for bf16
  const void* vsc;
  int64_t s_sb, s_sh, s_sl;
  const int* cache_idx;          // [B] cache row of each batch entry; null: the identity
  const int* seq_len;            // [B] keys visible to the last new token
  void* out;                     // bf16 [B, T, Hq, D]; null where the attention rows stay in the partials
  int64_t o_sb, o_st, o_sh;
  float* po;                     // split partials [B * Hkv, splits, M, D], M = (Hq / Hkv) * T,
  float* pm;                     // their natural-log row maxima [B * Hkv, splits, M]
  float* pl;                     // and row sums; sized for Lmax / 128 splits
  int B, T, Hq, Hkv, D;
  int Lmax;                      // cache capacity in keys
  float scale;                   // softmax scale
  int window;                    // sliding window in keys; 0: none
  hipStream_t stream;
};

// What the fused attention + o_proj launch needs beside it
struct DecodeOprojArgs {
  const void* wo;                // bf16 [Hout, Hq * D], row stride ldwo
  int64_t ldwo;
  int Hout;
  float* oacc;                   // fp32 [B * T, Hout], zero on entry: += o_proj(attention)
  float* mo;                     // SYNC form: [B * Hkv, M, D] merged attention rows; null: never SYNC
};

// Return codes of the three launchers: 0 launched; -1 shape not covered (nothing launched); -4 (MXFP8
// cache) dequantise and come back with a bf16 cache; -2 / -3 head dim / LDS size outside the chunk
// kernel; 3 the fused launcher's two launches disagree on the split count; otherwise the HIP error.

// 128-key-chunk kernel with its merge, or the MFMA kernel below where it covers the call
// (inference.hip).  The partials hold nsplit splits and nsplit * 128 keys stand for a.Lmax;
// counters: zeroed [B * Hkv] ints of the chunk kernel's fused merge (null with an MXFP8 cache).
int decode_attn_launch(DecodeAttnArgs a, int nsplit, int* counters);
// MFMA flash-decoding kernel (decode_attn.hip); *nsplit_out > 1: the caller merges the partials.
// Consumes the ranges armed by decode_attn_set_prefetch.
int decode_attn2_launch(DecodeAttnArgs a, int* nsplit_out);
// Fused attention + o_proj (decode_attn.hip): a.out unused, bf16 cache only.
int decode_attn_oproj_launch(DecodeAttnArgs a, const DecodeOprojArgs& o);

void decode_attn_set_prefetch(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes, int wgs);
void decode_attn_set_trace(uint64_t* trace);
void decode_attn_set_v2(int v);
void decode_attn_set_sync(int v);
int decode_attn_sync_error(bool reset);
void decode_attn_set_oproj_maxl(int v);
int decode_attn_oproj_maxl();

}  // namespace nxd
