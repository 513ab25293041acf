// The description of a tree-verification attention call (Medusa: cached prefix + tree mask) and the
// prototypes of its launcher (tree_attn.hip).  Included by the kernel and by bindings.cpp.  HIP runtime
// header only: the kernel translation unit stays free of torch.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace nxd {

// Callers value-initialise (`TreeAttnArgs a{};`) and set every field the call has.
struct TreeAttnArgs {
  const void* q;                 // bf16 [B, N, Hq, D], unit stride on D, 16-byte aligned rows
  int64_t q_sb, q_sn, q_sh;      // element strides of batch, node, head
  const void* k_tree;            // the tree nodes' bf16 K / V rows [B, N, Hkv, D] (views of the QKV buffer:
  const void* v_tree;            // unit stride on D, 16-byte aligned rows, one set of strides for both)
  int64_t t_sb, t_sn, t_sh;
  const uint64_t* mask_words;    // [N]: bit j of word n set iff node n sees tree key j (shared by the batch)
  const void* kc;                // bf16 caches [Bc, Hkv, Lmax, D], unit stride on D, 16-byte aligned rows
  const void* vc;
  int64_t c_sb, c_sh, c_sl;      // element strides of cache row, kv head, key
  const int* cache_idx;          // [B] cache row of each batch entry; null: the identity
  const int* prefix_len;         // [B] cached keys [0, prefix_len[b]) are visible to every row
  void* out;                     // bf16 [B, N, Hq, D]
  int64_t o_sb, o_sn, o_sh;
  float* po;                     // split partials [B * Hkv, nsplit, M, D], M = (Hq / Hkv) * N,
  float* pm;                     // their log2-domain row maxima [B * Hkv, nsplit, M]
  float* pl;                     // and row sums; unused (may be null) with one split
  int B, N, Hq, Hkv, D;
  int Bc, Lmax;                  // cache rows and capacity in keys
  float scale;                   // softmax scale
  hipStream_t stream;
};

// Key splits of a covered call, sized from Lmax (never from the device prefix_len) so that the grid
// fills the chip; -1: the shape is not covered (bf16, D 64 / 128, 1 <= N <= 64, (Hq / Hkv) * N <= 512).
int tree_attn_splits(int B, int N, int Hq, int Hkv, int D, int Lmax);
// 0 launched; -1 not covered or nsplit is not what tree_attn_splits gives (nothing launched);
// otherwise the HIP error.
int tree_attn_launch(const TreeAttnArgs& a, int nsplit);

}  // namespace nxd
