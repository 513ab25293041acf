// Fused decode-step projections over MXFP4 weights on MFMA weight tiles, 4-16 activation rows: the four
// forms of decode_fused_mx.hip (same rounding points, tests/decode_refs.py with w the dequantized weight)
//
//   PLAIN (+ norm) : y = bf16(acc)                                  final norm + lm_head
//   RESID          : y <- bf16(y + bf16(acc)), in place             o_proj, down
//   GLU   (+ norm) : y = bf16(silu(g) u), g = acc[:, n], u = acc[:, N + n]   gate_up ([gate; up] rows)
//   ROPE_KV (+ norm): QKV with RoPE and the KV-cache write (rounding points: decode_fused_mx.hip)
//   norm prologue  : a = bf16(x rstd w_norm), rstd = rsqrt(mean(x^2) + eps) in fp32
//
// on the weight side of gemv_mx_mfma.hip and an activation side of its own.  _C.dgemv_mx launches this
// kernel for 4 <= M <= 16 and dgemv_mx_kernel (VALU, decode_fused_mx.hip) for M <= 3.
//
// Weight side (mx_mfma_kernel's, see the reasons there).  A workgroup is 4 waves = (4 / KS) tile groups x
// KS k-slices on 4-block boundaries; a wave owns T tiles of 16 weight rows (GLU: T gate tiles and the up
// tiles of the same columns, so the epilogue is lane-local).  Lane l takes weight row l & 15 and in
// iteration i block 4 i + (l >> 4) of it: one plain 16-byte load is the block, cvt8 of its dword d is the B
// operand of MFMA d.  Scale bytes come as one dword per lane for four iterations and are handed out with
// ds_bpermute; two load rounds are in flight; lane groups past the slice contribute exact zeros and do not
// load; weight rows past N are clamped and never stored; the k-slices are summed through LDS in slice
// order (no atomics: two launches give the same bits).
// ROPE_KV takes tile pairs the way GLU takes gate and up tiles: in the q / k region a wave owns T units =
// the 16 weight rows d0 .. d0 + 15 of a head and the 16 rows at + D/2, as two accumulators, so lane l holds
// both halves of the rotary pair (d0 + (l & 15), + D/2) for activation rows 4 (l >> 4) + i and the rotation
// is lane-local; in the v region it owns 2 T plain tiles.  This needs (D / 2) % 16 == 0.  q, k, v and the
// cache elements are 2-byte scattered stores from the accumulator layout (16 lanes cover 32 contiguous
// bytes), as in dmm_kernel of decode_fused.hip.  The tile loader, cvt8 and the scale hand-out are
// copies of mx_mfma_kernel's, not a shared header: that kernel's register allocation is recorded
// (profiles/mxfp4_mfma_kernel_resources.txt) and stays untouched this way.
//
// Activation side.  The A operands come from LDS, written once per workgroup, not from per-wave global
// loads and v_permlane swaps.  The image is fragment-ordered: chunk d (8 elements) of block 4 i + g of row
// c, for iteration i of k-slice s, is the 16 bytes at
//
//     ((slot * 4 + d) * 64 + 16 g + c) * 16,      slot = s * SI + (i mod SI),
//
// so the ds_read_b128 of a wave for (i, d) is unit-stride over its 64 lanes (1 KB contiguous), and so is
// the ds_write_b128 of the wave that stages (slot, d): no bank conflicts either way.  K is staged in slabs
// of SLAB = 4 slots (16 KB: SI = 4 / KS iterations of every k-slice), wave w staging slot w with four
// 16-byte global loads per lane (its 16 lanes of a lane group read 16 rows, the four loads 64 contiguous
// bytes of each), through a ring of two slabs with one barrier per slab: the loads of slab s + 1 are
// issued before the MFMAs of slab s and written after them.  The LDS footprint (32 KB + the slice
// partials) does not depend on K or M, so RESID serves K = 8192 / 14336 and the norm forms carry no
// M * K limit.  Only this form is built: normalised rows staged whole (M K 2 bytes) would leave two
// workgroups per CU at 16 x 2048 and none at 16 x 4096, and were not measured.
// Only rows < M are staged; lanes with c >= M read row M - 1 (an A row feeds only its own C row, which is
// not stored).  Blocks past a slice are staged as zeros (their B operands are zeros as well).
// Slab depth: 4 slots.  8 slots (64 KB ring) leave two workgroups per CU where the registers allow three
// to five; it was ruled out on that count, not timed (profiles/LOG.md).
//
// Norm forms.  A statistics pass first: the M rows are dealt over the four waves, a wave sums the squares
// of a whole row in fp32 (wave_sum) and leaves rstd in LDS; the staging then normalises and rounds to
// bf16 on the way into the image.  Issue order (vmcnt retires in order): the staging loads of slab 0, the
// first chunk of every statistics row and RESID's old y elements go out ahead of the first weight round;
// so do ROPE_KV's positions (first of all) and, behind the staging loads, the cos / sin of the lane's
// rotary pairs: they wait for the positions only.
// XI (ROPE_KV): x is the embedding table and row m is x[xidx[m]] (zeros for an id outside it); workgroup 0,
// which stages every block of every row exactly once, also stores the gathered rows to xcopy.
#include <type_traits>

#include "common.h"
#include "decode_fused_mx.h"

namespace nxd {
namespace dfused_mx_mfma {

enum Epi { PLAIN = 0, RESID = 1, GLU = 2, ROPE_KV = 3 };

struct Params {
  const uint16_t* x;       // [M, K] bf16 activations, rows ldx elements apart
  int64_t ldx;
  const uint16_t* norm_w;  // [K] RMSNorm weight (PLAIN, GLU)
  const uint8_t* w;        // [Nw, K/2] packed codes, rows ldw bytes apart
  int64_t ldw;
  const uint8_t* scale;    // [Nw, K/32] E8M0, rows lds bytes apart
  int64_t lds;
  uint16_t* y;             // [M, N] (RESID: the residual stream, updated in place)
  int64_t ldy;
  float eps;
  int M, N, K;             // N = output columns (GLU: the up rows start at weight row N)
  // ROPE_KV: y rows hold [nq | nkv | nkv] heads of D; k / v also go to the caches
  int nq, nkv, D;
  const float* cos_t;      // [max_pos, D/2]
  const float* sin_t;
  const int64_t* pos;      // [M] absolute position of each row
  int T;                   // rows per sequence (cache row = cache_idx[m / T])
  uint16_t* kc;
  uint16_t* vc;
  int64_t c_sb, c_sh, c_sl;
  const int* cache_idx;    // [M / T] (nullable: identity)
  int Lmax, max_pos;
  // XI: x is the embedding table [xrows, K]
  const int64_t* xidx;
  int64_t xrows;
  uint16_t* xcopy;         // [M, K] contiguous (nullable)
};
static_assert(std::is_trivially_copyable<Params>::value && sizeof(Params) <= 4096, "kernel-argument struct");

constexpr int SLAB = 4;                   // slots (iterations over all k-slices) per slab = waves per workgroup
constexpr int SLAB_CHUNKS = SLAB * 256;   // 16-byte chunks per slab

// 8 codes of one dword (element 2j = low nibble of byte j) times the block scale -> 8 bf16, in k order
__device__ __forceinline__ bf16x8_t cvt8(uint32_t d, float s) {
  u32x4_t q;
  q[0] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 0));
  q[1] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 1));
  q[2] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 2));
  q[3] = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(d, s, 3));
  return __builtin_bit_cast(bf16x8_t, q);
}

// T output tiles of 16 columns per wave (GLU: T gate + T up weight tiles; ROPE_KV: T rotary tile pairs or 2 T
// v tiles), KS k-slices per tile group.  PLAIN, GLU and ROPE_KV carry the norm prologue, RESID does not.
// XI: ROPE_KV with the embedding gather.
template <int T, int KS, int EPI, bool XI = false>
__global__ void __launch_bounds__(256) dmx_mfma_kernel(Params p) {
  constexpr bool NORM = EPI != RESID;
  constexpr int NT = (EPI == GLU || EPI == ROPE_KV) ? 2 * T : T;   // weight tiles (accumulators) per wave
  constexpr int G = 4 / KS;                    // tile groups per workgroup
  constexpr int SI = SLAB / KS;                // iterations of one k-slice per slab
  __shared__ u32x4_t ring[2][SLAB_CHUNKS];
  __shared__ f32x4_t part[KS > 1 ? 4 : 1][NT][64];
  __shared__ float rs[16];
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int rg = wid / KS, ks = wid % KS;
  const int c = lane & 15, g = lane >> 4;
  const int cm = min(c, p.M - 1);
  const int tile0 = ((int)blockIdx.x * G + rg) * T;
  bool active = (int64_t)tile0 * 16 < p.N;   // wave-uniform

  // ROPE_KV: tile0 counts units; unit u of the q / k region is rows h D + d0 .. + 15 | + D/2 with
  // h = u / upd, d0 = 16 (u % upd), upd = D / 32 units per head; tile groups past the units take v tiles
  const int half = EPI == ROPE_KV ? p.D >> 1 : 0;
  const int upd = half >> 4;
  const int units = EPI == ROPE_KV ? (p.nq + p.nkv) * upd : 0;
  const int qk_rows = units * 32;
  const bool is_qk = tile0 < units;   // wave-uniform
  const int64_t v0 = EPI == ROPE_KV ? qk_rows + (int64_t)(tile0 / T - (units + T - 1) / T) * NT * 16 : 0;   // first v row

  const uint8_t* wr[NT];
  const uint8_t* sr[NT];
  if constexpr (EPI == ROPE_KV) {
    active = is_qk || v0 < p.N;
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      int64_t n;
      if (is_qk) {
        const int u = min(tile0 + t % T, units - 1);   // units past the last are clamped (and not stored)
        n = (int64_t)(u / upd) * p.D + 16 * (u % upd) + c + (t / T) * half;
      } else {
        n = min(v0 + 16 * t + c, (int64_t)p.N - 1);
      }
      wr[t] = p.w + n * p.ldw;
      sr[t] = p.scale + n * p.lds;
    }
  } else {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int64_t n = min((int64_t)(tile0 + t) * 16 + c, (int64_t)p.N - 1);   // rows past N are clamped (and not stored)
      wr[t] = p.w + n * p.ldw;
      sr[t] = p.scale + n * p.lds;
      if (EPI == GLU) {
        wr[T + t] = wr[t] + (int64_t)p.N * p.ldw;
        sr[T + t] = sr[t] + (int64_t)p.N * p.lds;
      }
    }
  }

  // k-slices in blocks; they start at multiples of 4 blocks.  Slice 0 is the longest: its iteration count
  // is the workgroup's (every wave stages and meets every barrier, whatever its own slice holds).
  const int KB = p.K >> 5;
  const int per = ((KB + KS - 1) / KS + 3) & ~3;
  const int kb0 = min(ks * per, KB), kb1 = min(KB, kb0 + per);
  const int nit = active ? (kb1 - kb0 + 3) >> 2 : 0;
  const int nit_wg = (min(per, KB) + 3) >> 2;
  // staging: this wave fills slot wid of every slab = iteration (slab * SI + wid % SI) of slice wid / SI
  const int skb0 = min((wid / SI) * per, KB), skb1 = min(KB, skb0 + per);
  // XI: input row m is the embedding-table row of token id xidx[m]; an id outside [0, xrows) reads an
  // in-bounds row whose value is replaced by zeros at its use (ops.vocab_parallel_embedding's zero row)
  auto xbase = [&](int m) -> const uint16_t* {
    if constexpr (XI) {
      const int64_t t = p.xidx[m];
      return p.x + (t < 0 ? 0 : (t >= p.xrows ? p.xrows - 1 : t)) * p.ldx;
    } else {
      return p.x + (int64_t)m * p.ldx;
    }
  };
  auto xok = [&](int m) -> bool {
    if constexpr (XI) {
      const int64_t t = p.xidx[m];
      return t >= 0 && t < p.xrows;
    } else {
      return true;
    }
  };
  // ROPE_KV: position and cache row of this lane's C rows 4 g + i (clamped rows are not stored); pc is the
  // position as the caches take it, -1 outside [0, Lmax)
  int64_t ps[EPI == ROPE_KV ? 4 : 1];
  int cb[EPI == ROPE_KV ? 4 : 1], pc[EPI == ROPE_KV ? 4 : 1];
  if constexpr (EPI == ROPE_KV) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = min(4 * g + i, p.M - 1);
      ps[i] = p.pos[m];
      cb[i] = p.cache_idx ? p.cache_idx[m / p.T] : m / p.T;
    }
  }
  const uint16_t* xrow = xbase(cm);
  const bool xrow_ok = xok(cm);

  struct Stage {
    u32x4_t x[4];
    u32x4_t nw[NORM ? 4 : 1];
    bool ok;
    int kb;
  };
  auto stage_load = [&](Stage& st, int slab) {
    const int kb = skb0 + 4 * (slab * SI + wid % SI) + g;
    st.kb = kb;
    st.ok = kb < skb1 && c < p.M;
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      st.x[d] = u32x4_t{0u, 0u, 0u, 0u};
      if (NORM) st.nw[d] = u32x4_t{0u, 0u, 0u, 0u};
      if (st.ok) {
        st.x[d] = *reinterpret_cast<const u32x4_t*>(xrow + (int64_t)kb * 32 + 8 * d);
        if (NORM) st.nw[d] = *reinterpret_cast<const u32x4_t*>(p.norm_w + (int64_t)kb * 32 + 8 * d);
      }
    }
  };
  float rstd = 0.f;   // NORM: of row cm, after the statistics pass
  auto stage_store = [&](const Stage& st, int buf) {
    if (c >= p.M) return;   // only rows < M are staged
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      u32x4_t v = st.x[d];
      if constexpr (XI) {
        if (!xrow_ok) v = u32x4_t{0u, 0u, 0u, 0u};
        if (blockIdx.x == 0 && p.xcopy && st.ok) *reinterpret_cast<u32x4_t*>(p.xcopy + (int64_t)c * p.K + (int64_t)st.kb * 32 + 8 * d) = v;
      }
      if constexpr (NORM) {
        float f[8], gw[8];
        unpack8(v, f);
        unpack8(st.nw[d], gw);
#pragma unroll
        for (int j = 0; j < 8; ++j) f[j] = f[j] * rstd * gw[j];
        v = pack8(f);
        if (!st.ok) v = u32x4_t{0u, 0u, 0u, 0u};   // past the slice: zeros whatever rstd is
      }
      ring[buf][(wid * 4 + d) * 64 + 16 * g + c] = v;
    }
  };

  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  struct Round {
    u32x4_t w[NT];
  };
  // Scales: once per 4 iterations lane (c, g) loads the 4 scale bytes of iteration 4 I + g of its row as
  // one dword (any alignment); iteration 4 I + q then takes byte g of the dword of lane (c, q) with one
  // ds_bpermute.  A dword that would pass the end of the row is put together from the bytes inside it.
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
    const int kb = kb0 + 4 * it + g;
#pragma unroll
    for (int t = 0; t < NT; ++t) {   // idle lane group: +0 codes (its activations are staged as zeros)
      r.w[t] = u32x4_t{0u, 0u, 0u, 0u};
      if (kb < kb1) r.w[t] = *reinterpret_cast<const u32x4_t*>(wr[t] + (int64_t)kb * 16);
    }
  };
  // iteration `it` of this wave's slice, its A fragments in slab buffer `buf`
  auto mma = [&](const Round& r, const Scales& sc, int it, int buf) {
    const bool idle = kb0 + 4 * it + g >= kb1;   // scale 1 for the zero codes of an idle lane group
    const int src = c + 16 * (it & 3);
    const u32x4_t* a = &ring[buf][((ks * SI + it % SI) * 4) * 64 + 16 * g + cm];
    u32x4_t x[4];
#pragma unroll
    for (int d = 0; d < 4; ++d) x[d] = a[d * 64];
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const uint32_t sv = (uint32_t)__shfl((int)sc.v[t], src, 64);
      const float s = idle ? 1.f : e8m0((uint8_t)(sv >> (8 * g)));
#pragma unroll
      for (int d = 0; d < 4; ++d)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, x[d]), cvt8(r.w[t][d], s), acc[t], 0, 0, 0);
    }
  };

  // ---- loads that go out ahead of the weights, raw until used
  Stage st;
  stage_load(st, 0);
  const int nch = p.K >> 3;   // 16-byte chunks per activation row
  u32x4_t x0[NORM ? 4 : 1];
  if constexpr (NORM) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {   // statistics: this wave's rows wid, wid + 4, ..., first chunk of each
      const int r = wid + 4 * i;
      x0[i] = u32x4_t{0u, 0u, 0u, 0u};
      if (r < p.M && lane < nch) x0[i] = *reinterpret_cast<const u32x4_t*>(xbase(r) + 8 * lane);
    }
  }
  // ROPE_KV: cos / sin of this lane's rotary pairs (unit t: d = d0 + c) at the positions of its C rows
  float cosv[EPI == ROPE_KV ? T : 1][4], sinv[EPI == ROPE_KV ? T : 1][4];
  if constexpr (EPI == ROPE_KV) {
#pragma unroll
    for (int t = 0; t < T; ++t)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        cosv[t][i] = sinv[t][i] = 0.f;
        if (is_qk && ks == 0) {
          const int64_t pt = ps[i] < 0 ? 0 : (ps[i] >= p.max_pos ? p.max_pos - 1 : ps[i]);
          const int d = 16 * (min(tile0 + t, units - 1) % upd) + c;
          cosv[t][i] = p.cos_t[pt * half + d];
          sinv[t][i] = p.sin_t[pt * half + d];
        }
      }
#pragma unroll
    for (int i = 0; i < 4; ++i) pc[i] = ps[i] >= 0 && ps[i] < p.Lmax ? (int)ps[i] : -1;
  }
  uint16_t y_raw[EPI == RESID ? T : 1][4];   // RESID: the old y elements of this lane's C fragment
  if (EPI == RESID && ks == 0 && active) {
#pragma unroll
    for (int t = 0; t < T; ++t) {
      const int64_t n = (int64_t)(tile0 + t) * 16 + c;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int m = 4 * g + i;
        y_raw[t][i] = 0;
        if (n < p.N && m < p.M) y_raw[t][i] = p.y[(int64_t)m * p.ldy + n];
      }
    }
  }
  // two weight rounds in flight: rounds 0 and 1 go out first; after the MFMAs of round i its buffer takes
  // round i + 2
  Round ra, rb;
  Scales sc, sn;
  if (nit > 0) {
    load_scales(sc, 0);
    load(ra, 0);
  }
  if (nit > 1) load(rb, 1);

  // ---- statistics pass of the norm forms
  if constexpr (NORM) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = wid + 4 * i;   // wave-uniform
      if (r >= p.M) continue;
      float ss = 0.f;
      for (int ci = lane; ci < nch; ci += 64) {
        u32x4_t v = ci == lane ? x0[i] : *reinterpret_cast<const u32x4_t*>(xbase(r) + 8 * ci);
        if (XI && !xok(r)) v = u32x4_t{0u, 0u, 0u, 0u};
        float f[8];
        unpack8(v, f);
#pragma unroll
        for (int j = 0; j < 8; ++j) ss += f[j] * f[j];
      }
      ss = wave_sum(ss);
      if (lane == 0) rs[r] = rsqrtf(ss / (float)p.K + p.eps);
    }
    __syncthreads();
    rstd = rs[cm];
  }
  stage_store(st, 0);
  __syncthreads();

  // ---- main loop: four iterations = 4 / SI slabs per trip.  Per slab: issue the staging loads of the next
  // one, run this wave's SI iterations from the current buffer, write the next slab to the other buffer,
  // one barrier.  Every wave takes every trip (nit_wg), whatever its own slice holds.
  int slab = 0;
#pragma unroll 1
  for (int it = 0; it < nit_wg; it += 4) {
    if (it + 4 < nit) load_scales(sn, (it >> 2) + 1);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (q % SI == 0) stage_load(st, slab + 1);
      if (it + q < nit) {
        mma(q & 1 ? rb : ra, sc, it + q, slab & 1);
        if (it + q + 2 < nit) load(q & 1 ? rb : ra, it + q + 2);
      }
      if (q % SI == SI - 1) {
        stage_store(st, (slab + 1) & 1);
        __syncthreads();
        ++slab;
      }
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

  // ---- epilogue: lane (c, g) holds rows 4 g .. 4 g + 3 of column c of each of its tiles
  if constexpr (EPI == ROPE_KV) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      if (is_qk) {   // unit t: accumulators t (rows d) and T + t (rows d + D/2)
        if (t >= T || tile0 + t >= units) continue;
        const int h = (tile0 + t) / upd, d = 16 * ((tile0 + t) % upd) + c;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = 4 * g + i;
          if (m >= p.M) continue;
          const float x1 = bf2f(f2bf(acc[t % T][i])), x2 = bf2f(f2bf(acc[T + t % T][i]));   // bf16 projection output
          const float cc = cosv[t % T][i], ss = sinv[t % T][i];
          const uint16_t o1 = f2bf(x1 * cc - x2 * ss), o2 = f2bf(x2 * cc + x1 * ss);
          uint16_t* yp = p.y + (int64_t)m * p.ldy + h * p.D + d;
          yp[0] = o1;
          yp[half] = o2;
          if (h >= p.nq && pc[i] >= 0) {
            uint16_t* kp = p.kc + (int64_t)cb[i] * p.c_sb + (int64_t)(h - p.nq) * p.c_sh + (int64_t)pc[i] * p.c_sl + d;
            kp[0] = o1;
            kp[half] = o2;
          }
        }
      } else {
        const int64_t n = v0 + 16 * t + c;
        if (n >= p.N) continue;
        const int vr = (int)(n - qk_rows);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int m = 4 * g + i;
          if (m >= p.M) continue;
          const uint16_t o = f2bf(acc[t][i]);
          p.y[(int64_t)m * p.ldy + n] = o;
          if (pc[i] >= 0)
            p.vc[(int64_t)cb[i] * p.c_sb + (int64_t)(vr / p.D) * p.c_sh + (int64_t)pc[i] * p.c_sl + vr % p.D] = o;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int t = 0; t < T; ++t) {
    const int64_t n = (int64_t)(tile0 + t) * 16 + c;
    if (n >= p.N) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = 4 * g + i;
      if (m >= p.M) continue;
      uint16_t* yp = p.y + (int64_t)m * p.ldy + n;
      if (EPI == GLU) {
        const float gt = acc[t][i], u = acc[EPI == GLU ? T + t : t][i];
        *yp = f2bf(gt / (1.f + __expf(-gt)) * u);
      } else if (EPI == RESID) {
        *yp = f2bf(bf2f(y_raw[EPI == RESID ? t : 0][i]) + bf2f(f2bf(acc[t][i])));
      } else {
        *yp = f2bf(acc[t][i]);
      }
    }
  }
}

// Tiles per wave and K split as mx_mfma_launch picks them (gemv_mx_mfma.hip): the most tiles per wave that
// still leaves 400 workgroups' worth of tile groups, K split over the four waves while a slice keeps 16
// blocks.  The norm forms then take the smallest K split that still gives 400 workgroups: every workgroup
// repeats the statistics pass and stages all of x, so four tile groups sharing one image win where the
// tiles are plentiful (8 rows, lm_head of Llama-3.2-1B: T 4 / KS 1 40.1 us, KS 4 56.0; gate_up stays at
// KS 4; sweep in profiles/LOG.md).
static void pick(int64_t tiles, int KB, int epi, int* T, int* KS) {
  int t = epi == GLU || epi == ROPE_KV ? 2 : 4;
  while (t > 1 && tiles / t < 400) t >>= 1;
  int ks = 4;
  while (ks > 1 && KB / ks < 16) ks >>= 1;
  if (epi != RESID) {
    const int64_t groups = (tiles + t - 1) / t;
    int k = 1;
    while (k < ks && groups * k / 4 < 400) k <<= 1;
    ks = k;
  }
  *T = t;
  *KS = ks;
}

template <int T, int KS, int EPI, bool XI = false>
static int launch_one(const Params& p, hipStream_t s) {
  constexpr int G = 4 / KS;
  int64_t groups = ((int64_t)(p.N + 15) / 16 + T - 1) / T;
  if (EPI == ROPE_KV) {   // tile groups of T rotary tile pairs, then of 2 T v tiles
    const int units = (p.nq + p.nkv) * (p.D / 32);
    groups = (units + T - 1) / T + (p.nkv * p.D / 16 + 2 * T - 1) / (2 * T);
  }
  dim3 grid((unsigned)((groups + G - 1) / G)), block(256);
  hipLaunchKernelGGL((dmx_mfma_kernel<T, KS, EPI, XI>), grid, block, 0, s, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <int T, int EPI, bool XI = false>
static int launch_ks(const Params& p, int KS, hipStream_t s) {
  if (KS == 4) return launch_one<T, 4, EPI, XI>(p, s);
  if (KS == 2) return launch_one<T, 2, EPI, XI>(p, s);
  return launch_one<T, 1, EPI, XI>(p, s);
}

template <int EPI>
static int launch_t(const Params& p, int T, int KS, hipStream_t s) {
  if constexpr (EPI == ROPE_KV) {
    if (p.xidx) return T == 2 ? launch_ks<2, EPI, true>(p, KS, s) : launch_ks<1, EPI, true>(p, KS, s);
  } else if constexpr (EPI != GLU) {
    if (T == 4) return launch_ks<4, EPI>(p, KS, s);
  }
  if (T == 2) return launch_ks<2, EPI>(p, KS, s);
  return launch_ks<1, EPI>(p, KS, s);
}

}  // namespace dfused_mx_mfma

// The 4-16 row form of dgemv_mx.  cfg = 0: tiles per wave T and k-slices KS from the shape; cfg = 16 T + KS
// forces them (T in {1, 2, 4}, 4 not with GLU or ROPE_KV; KS in {1, 2, 4}) for the tests and tools/bench_mx_decode.py.
// rope (epi = 3 only, else null): the ROPE_KV operands; a head dim with (D / 2) % 16 != 0 returns -5.
int dgemv_mx_mfma_launch(int epi, const void* x, int64_t ldx, const void* norm_w, float eps, const void* w, int64_t ldw,
                         const void* scale, int64_t lds, void* y, int64_t ldy, int M, int N, int K, int cfg,
                         hipStream_t stream, const DgemvMxRope* rope) {
  using namespace dfused_mx_mfma;
  if (epi < PLAIN || epi > ROPE_KV || (epi == ROPE_KV) != (rope != nullptr)) return -1;
  if (M < 4 || M > 16 || N < 1 || K < 32 || (K & 31)) return -1;
  if ((epi == RESID) != (norm_w == nullptr)) return -3;   // PLAIN / GLU carry the norm prologue, RESID does not
  if ((ldw & 15) || (reinterpret_cast<uintptr_t>(w) & 15) || (ldx & 7) || (reinterpret_cast<uintptr_t>(x) & 15) ||
      (reinterpret_cast<uintptr_t>(norm_w) & 15))
    return -4;
  int T, KS;
  pick((N + 15) / 16, K >> 5, epi, &T, &KS);
  if (cfg) {
    T = cfg >> 4;
    KS = cfg & 15;
    if ((T != 1 && T != 2 && T != 4) || (KS != 1 && KS != 2 && KS != 4) || ((epi == GLU || epi == ROPE_KV) && T == 4))
      return -6;
  }
  Params p{static_cast<const uint16_t*>(x), ldx, static_cast<const uint16_t*>(norm_w), static_cast<const uint8_t*>(w), ldw,
           static_cast<const uint8_t*>(scale), lds, static_cast<uint16_t*>(y), ldy, eps, M, N, K};
  if (epi == ROPE_KV) {
    const DgemvMxRope& q = *rope;
    if (q.nq < 1 || q.nkv < 1 || q.D < 2 || (q.D & 1) || (int64_t)(q.nq + 2 * q.nkv) * q.D != N || q.T < 1 || M % q.T ||
        q.max_pos < 1)
      return -1;
    if ((q.D / 2) % 16) return -5;   // the rotary tile pairs
    if (q.xidx && q.xrows < 1) return -4;
    p.nq = q.nq, p.nkv = q.nkv, p.D = q.D;
    p.cos_t = q.cos_t, p.sin_t = q.sin_t, p.pos = q.pos, p.T = q.T;
    p.kc = static_cast<uint16_t*>(q.kc), p.vc = static_cast<uint16_t*>(q.vc);
    p.c_sb = q.c_sb, p.c_sh = q.c_sh, p.c_sl = q.c_sl;
    p.cache_idx = q.cache_idx, p.Lmax = q.Lmax, p.max_pos = q.max_pos;
    p.xidx = q.xidx, p.xrows = q.xrows, p.xcopy = static_cast<uint16_t*>(q.xcopy);
    return launch_t<ROPE_KV>(p, T, KS, stream);
  }
  if (epi == PLAIN) return launch_t<PLAIN>(p, T, KS, stream);
  if (epi == RESID) return launch_t<RESID>(p, T, KS, stream);
  return launch_t<GLU>(p, T, KS, stream);
}

}  // namespace nxd
