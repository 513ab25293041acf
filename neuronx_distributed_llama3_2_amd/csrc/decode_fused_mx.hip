// Fused decode-step GEMVs over MXFP4 weights (1-3 activation rows): the launches of decode_fused.hip
// that a weight-quantized Llama can take -- o_proj / down with the residual add as epilogue, gate_up
// with the RMSNorm prologue and SwiGLU, the final norm + lm_head, the fused QKV projection with RoPE
// and the KV-cache write -- reading the 4-bit codes directly
// (format: ops/gemv.py; one 16-byte lane load is one 32-element block, converted by
// v_cvt_scalef32_pk_bf16_fp4 and multiplied on v_dot2c_f32_bf16 as in gemv_mx.hip).  The rounding
// points are those of dgemv (tests/decode_refs.py) with w read as the dequantized weight:
//
//   PLAIN (+ norm) : y = bf16(acc)                                  final norm + lm_head
//   RESID          : y <- bf16(y + bf16(acc)), in place             o_proj, down
//   GLU   (+ norm) : y = bf16(silu(g) u), g = acc[:, n], u = acc[:, N + n]   gate_up ([gate; up] rows)
//   ROPE_KV (+ norm): p = bf16(acc); q / k heads rotate the pair (d, d + D/2) in fp32,
//                    o1 = bf16(p1 c - p2 s), o2 = bf16(p2 c + p1 s), c / s from the fp32 tables at
//                    clamp(pos[m], 0, max_pos - 1); q, k, v -> y, k and v also into the bf16 caches
//                    at (cache_idx[m / T] or m / T, head, pos[m]) when 0 <= pos[m] < Lmax        QKV
//   norm prologue  : a = bf16(x rstd w_norm), rstd = rsqrt(mean(x^2) + eps) in fp32
//   XI (ROPE_KV)   : x is the embedding table, row m is x[xidx[m]] (zeros for an id outside the
//                    table); workgroup 0 also stores the gathered rows to xcopy (first layer's QKV)
//
// Work split.  A 4-bit row is short: 2048 elements are 64 blocks, ONE 16-byte load per lane, so a wave
// that owned one row would keep 1 KB in flight.  A wave therefore owns NW weight rows (R rows, or R
// (gate, up) pairs) and U 64-block k-steps per round with NW * U = 4: every lane has four code loads
// (and, issued right next to each, that row's scale byte) outstanding before the first convert.  R
// follows from the k-steps a wave's slice has (launcher: rows_for).  A workgroup is 4 waves =
// (4 / KS) row groups x KS k-slices; a slice is a whole number of blocks, partial sums meet in LDS
// and are added in slice order (no atomics: two launches give the same bits); an empty slice adds
// exact zeros.  The wave index goes through readfirstlane, so row pointers and the k range live in
// SGPRs.  Rows past N are clamped and never stored.
// ROPE_KV owns rows the way GLU owns (n, n + N) pairs: in the q / k region a wave has R rotary pairs
// (rows h D + d and h D + d + D/2, pairs numbered through the heads), so after wave_sum the rotation
// is lane-local; in the v region it has NW = 2 R consecutive rows.  The q / k row groups come first in
// the grid, the v row groups after them.
//
// Issue order.  vmcnt retires in order, so a load issued after the weight round can only be waited for
// together with all of it (decode_fused.hip measured 2-4 us per launch for getting this wrong).  Ahead
// of the first weight round, and kept raw until their use, go: the prologue's first chunk of every x
// row and of the norm weight; at one row without a prologue the first round's activation chunks; the
// RESID epilogue's old y elements; ROPE_KV's positions (scalar loads, issued first of all), then the
// cos / sin of the lane's pair and the cache row.
//
// Normalised rows in LDS.  A lane needs the 32 activations of its block = four ds_read_b128 per row.
// Row-major, lane l would read at 64 l + 16 d bytes (a 4-way bank conflict); the image is chunk-major
// instead: 16-byte chunk d of block b of row m at ((m * 4 + d) * (K / 32) + b) * 16, so each of the
// four reads is unit-stride across the wave.  The prologue writes it once per workgroup, 16 lanes per
// chunk index d (lane = 16 d + block), which keeps both the global reads (a wave covers 1 KB
// contiguous) and the LDS writes (256 contiguous bytes per 16 lanes) conflict-free.
#include <cstdlib>
#include <type_traits>

#include "common.h"
#include "decode_fused_mx.h"

namespace nxd {
namespace dfused_mx {

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

// MM: activation rows compiled in (rows >= p.M are neither read nor stored); R: output rows (GLU:
// gate/up pairs, ROPE_KV: rotary pairs or 2 R v rows) per wave; KS: k-slices per row group.  PLAIN, GLU
// and ROPE_KV carry the norm prologue, RESID does not.  XI: ROPE_KV with the embedding gather.
template <int MM, int R, int EPI, int KS, bool XI = false>
__global__ void __launch_bounds__(256) dgemv_mx_kernel(Params p) {
  constexpr bool NORM = EPI != RESID;
  constexpr int NW = (EPI == GLU || EPI == ROPE_KV) ? 2 * R : R;   // weight rows per wave
  constexpr int U = 4 / NW;                    // 64-block k-steps per load round
  static_assert(NW == 1 || NW == 2 || NW == 4, "NW * U = 4 code loads per lane and round");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  u32x4_t* xs = reinterpret_cast<u32x4_t*>(smem);   // NORM: chunk-major normalised rows (see the header)
  __shared__ float red[4][MM];
  __shared__ float part[4][MM][NW];
  const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rg = wid / KS, ks = wid % KS;
  const int n0 = (blockIdx.x * (4 / KS) + rg) * R;   // first output column of this row group
  bool active = n0 < p.N;                            // inactive groups compute on clamped rows, never store
  const int KB = p.K >> 5;                           // blocks per row

  // ROPE_KV: pair n0 + r of the q / k heads is rows h D + d | + D/2 with h = pair / (D/2), d = pair % (D/2);
  // row groups past the pairs take v rows v0 + i
  const int half = EPI == ROPE_KV ? p.D >> 1 : 0;
  const int npair = EPI == ROPE_KV ? (p.nq + p.nkv) * half : 0;
  const int qk_rows = 2 * npair;
  const bool is_qk = n0 < npair;
  const int v0 = EPI == ROPE_KV ? qk_rows + (n0 / R - (npair + R - 1) / R) * NW : 0;

  const uint8_t* wrow[NW];
  const uint8_t* srow[NW];
  if constexpr (EPI == ROPE_KV) {
    active = is_qk || v0 < p.N;
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      int n;
      if (is_qk) {
        const int j = min(n0 + i % R, npair - 1);
        n = (j / half) * p.D + j % half + (i / R) * half;
      } else {
        n = (int)min((int64_t)v0 + i, (int64_t)p.N - 1);
      }
      wrow[i] = p.w + (int64_t)n * p.ldw;
      srow[i] = p.scale + (int64_t)n * p.lds;
    }
  } else {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int n = min(n0 + r, p.N - 1);
      wrow[r] = p.w + (int64_t)n * p.ldw;
      srow[r] = p.scale + (int64_t)n * p.lds;
      if (EPI == GLU) {
        wrow[R + r] = p.w + (int64_t)(n + p.N) * p.ldw;
        srow[R + r] = p.scale + (int64_t)(n + p.N) * p.lds;
      }
    }
  }
  // this wave's k-slice in blocks; an empty one (kbeg == kend) loads block klast and multiplies nothing
  const int kbc = (KB + KS - 1) / KS;
  const int kbeg = min(ks * kbc, KB), kend = min(KB, kbeg + kbc);
  const int klast = max(kend, 1) - 1;

  // Codes non-temporal (every byte is read once per token), unpredicated: a lane past kend re-reads
  // the slice's last block (in bounds) and the FMA loop skips it.  The scale byte is issued next to
  // its row's codes and kept raw.
  u32x4_t wv[NW][U];
  uint8_t sc[NW][U];
  auto load_round = [&](int base) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kb = min(base + u * 64 + lane, klast);
#pragma unroll
      for (int r = 0; r < NW; ++r) {
        wv[r][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(wrow[r] + (int64_t)kb * 16));
        sc[r][u] = srow[r][kb];
      }
    }
  };

  // ---- loads that go out ahead of the weights (see "Issue order"), raw until used
  // prologue: thread (wid, lane) owns chunk pd of block pb0 + 64 trip
  const int pd = lane >> 4, pb0 = wid * 16 + (lane & 15);
  // XI: input row m is the embedding-table row of token id xidx[m] (a scalar load); an id outside
  // [0, xrows) reads an in-bounds row whose value is replaced by zeros at its use, as
  // ops.vocab_parallel_embedding returns a zero row for such ids
  auto xrow = [&](int m) -> const uint16_t* {
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
  // ROPE_KV: positions of the rows (scalar; the cos / sin loads below wait for them, the prologue's
  // loads in between do not)
  int64_t ps[EPI == ROPE_KV ? MM : 1];
  if constexpr (EPI == ROPE_KV) {
#pragma unroll
    for (int m = 0; m < MM; ++m) ps[m] = p.pos[min(m, p.M - 1)];
  }
  u32x4_t x0[MM], gw0 = {0, 0, 0, 0};
  if (NORM && pb0 < KB) {
#pragma unroll
    for (int m = 0; m < MM; ++m)   // rows past M re-read the last row (never used)
      x0[m] = *reinterpret_cast<const u32x4_t*>(xrow(min(m, p.M - 1)) + pb0 * 32 + pd * 8);
    gw0 = *reinterpret_cast<const u32x4_t*>(p.norm_w + pb0 * 32 + pd * 8);
  }
  // ROPE_KV: lane r < R holds cos / sin of pair n0 + r at every row's position, every lane the cache rows
  float cs[EPI == ROPE_KV ? MM : 1], sn[EPI == ROPE_KV ? MM : 1];
  int cb[EPI == ROPE_KV ? MM : 1];
  if constexpr (EPI == ROPE_KV) {
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      const int b = min(m, p.M - 1) / p.T;
      cb[m] = p.cache_idx ? p.cache_idx[b] : b;
      cs[m] = sn[m] = 0.f;
      if (is_qk && lane < R && ks == 0) {
        const int64_t pt = ps[m] < 0 ? 0 : (ps[m] >= p.max_pos ? p.max_pos - 1 : ps[m]);
        const int d = min(n0 + lane, npair - 1) % half;
        cs[m] = p.cos_t[pt * half + d];
        sn[m] = p.sin_t[pt * half + d];
      }
    }
  }
  constexpr bool PREX = !NORM && MM == 1;   // one row, no prologue: the first round's activation chunks
  u32x4_t xv0[PREX ? U : 1][4];
  if constexpr (PREX) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kb = min(kbeg + u * 64 + lane, klast);
#pragma unroll
      for (int d = 0; d < 4; ++d) xv0[u][d] = *reinterpret_cast<const u32x4_t*>(p.x + kb * 32 + d * 8);
    }
  }
  uint16_t y_raw[MM];   // RESID: lane r < R holds the old y[m, n0 + r]
  if (EPI == RESID && lane < R && ks == 0) {
    const int n = min(n0 + lane, p.N - 1);
#pragma unroll
    for (int m = 0; m < MM; ++m) y_raw[m] = p.y[(int64_t)min(m, p.M - 1) * p.ldy + n];
  }
  load_round(kbeg);

  // ---- RMSNorm prologue: raw rows -> LDS and sum of squares, then normalised in place
  if constexpr (NORM) {
    float ss[MM];
#pragma unroll
    for (int m = 0; m < MM; ++m) ss[m] = 0.f;
    for (int b = pb0; b < KB; b += 64) {
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        if (m < p.M) {
          u32x4_t v = b == pb0 ? x0[m] : *reinterpret_cast<const u32x4_t*>(xrow(m) + b * 32 + pd * 8);
          if (XI && !xok(m)) v = u32x4_t{0u, 0u, 0u, 0u};
          float f[8];
          unpack8(v, f);
#pragma unroll
          for (int j = 0; j < 8; ++j) ss[m] += f[j] * f[j];
          xs[(m * 4 + pd) * KB + b] = v;
          if (XI && blockIdx.x == 0 && p.xcopy) *reinterpret_cast<u32x4_t*>(p.xcopy + (int64_t)m * p.K + b * 32 + pd * 8) = v;
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      const float sm = wave_sum(ss[m]);
      if (lane == 0) red[wid][m] = sm;
    }
    __syncthreads();
    float rstd[MM];
#pragma unroll
    for (int m = 0; m < MM; ++m) rstd[m] = rsqrtf((red[0][m] + red[1][m] + red[2][m] + red[3][m]) / (float)p.K + p.eps);
    for (int b = pb0; b < KB; b += 64) {
      float g[8];
      unpack8(b == pb0 ? gw0 : *reinterpret_cast<const u32x4_t*>(p.norm_w + b * 32 + pd * 8), g);
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        if (m < p.M) {
          float f[8];
          unpack8(xs[(m * 4 + pd) * KB + b], f);
#pragma unroll
          for (int j = 0; j < 8; ++j) f[j] = f[j] * rstd[m] * g[j];
          xs[(m * 4 + pd) * KB + b] = pack8(f);
        }
      }
    }
    __syncthreads();
  }

  float acc[MM][NW];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < NW; ++r) acc[m][r] = 0.f;

  auto fma_round = [&](int base, bool first) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int kb = base + u * 64 + lane;
      if (kb < kend) {
        float s[NW];
#pragma unroll
        for (int r = 0; r < NW; ++r) s[r] = e8m0(sc[r][u]);
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          W8 wb[NW];
#pragma unroll
          for (int r = 0; r < NW; ++r) wb[r] = cvt8(wv[r][u][d], s[r]);
#pragma unroll
          for (int m = 0; m < MM; ++m) {
            if (m < p.M) {
              u32x4_t xv;
              if constexpr (NORM) {
                xv = xs[(m * 4 + d) * KB + kb];
              } else {
                xv = (PREX && first) ? xv0[PREX ? u : 0][d]
                                     : *reinterpret_cast<const u32x4_t*>(p.x + (int64_t)m * p.ldx + kb * 32 + d * 8);
              }
#pragma unroll
              for (int r = 0; r < NW; ++r) acc[m][r] = dot8(xv, wb[r], acc[m][r]);
            }
          }
        }
      }
    }
  };
  fma_round(kbeg, true);
  for (int base = kbeg + 64 * U; base < kend; base += 64 * U) {
    load_round(base);
    fma_round(base, false);
  }

#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < NW; ++r) acc[m][r] = wave_sum(acc[m][r]);
  if (KS > 1) {
    if (lane == 0) {
#pragma unroll
      for (int m = 0; m < MM; ++m)
#pragma unroll
        for (int r = 0; r < NW; ++r) part[wid][m][r] = acc[m][r];
    }
    __syncthreads();
    if (ks != 0) return;
#pragma unroll
    for (int m = 0; m < MM; ++m)
#pragma unroll
      for (int r = 0; r < NW; ++r) {
        float t = 0.f;
#pragma unroll
        for (int j = 0; j < KS; ++j) t += part[wid + j][m][r];   // slice order
        acc[m][r] = t;
      }
  }
  if (!active) return;

  // ---- epilogue: every lane holds every sum; lane r stores output column n0 + r of all rows
  if constexpr (EPI == ROPE_KV) {   // lane r: rotary pair n0 + r; in the v region lane i: row v0 + i
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      if (lane != i) continue;
      if (is_qk) {
        if (i >= R || n0 + i >= npair) continue;
        const int h = (n0 + i) / half, d = (n0 + i) % half;
#pragma unroll
        for (int m = 0; m < MM; ++m) {
          if (m >= p.M) continue;
          const float x1 = bf2f(f2bf(acc[m][i % R])), x2 = bf2f(f2bf(acc[m][R + i % R]));   // bf16 projection output
          const uint16_t o1 = f2bf(x1 * cs[m] - x2 * sn[m]), o2 = f2bf(x2 * cs[m] + x1 * sn[m]);
          uint16_t* yp = p.y + (int64_t)m * p.ldy + h * p.D + d;
          yp[0] = o1;
          yp[half] = o2;
          if (h >= p.nq && ps[m] >= 0 && ps[m] < p.Lmax) {
            uint16_t* kp = p.kc + (int64_t)cb[m] * p.c_sb + (int64_t)(h - p.nq) * p.c_sh + ps[m] * p.c_sl + d;
            kp[0] = o1;
            kp[half] = o2;
          }
        }
      } else {
        if ((int64_t)v0 + i >= p.N) continue;
        const int vr = v0 + i - qk_rows;
#pragma unroll
        for (int m = 0; m < MM; ++m) {
          if (m >= p.M) continue;
          const uint16_t o = f2bf(acc[m][i]);
          p.y[(int64_t)m * p.ldy + v0 + i] = o;
          if (ps[m] >= 0 && ps[m] < p.Lmax)
            p.vc[(int64_t)cb[m] * p.c_sb + (int64_t)(vr / p.D) * p.c_sh + ps[m] * p.c_sl + vr % p.D] = o;
        }
      }
    }
    return;
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (lane != r || n0 + r >= p.N) continue;
#pragma unroll
    for (int m = 0; m < MM; ++m) {
      if (m >= p.M) continue;
      uint16_t* yp = p.y + (int64_t)m * p.ldy + n0 + r;
      if (EPI == GLU) {
        const float g = acc[m][r], u = acc[m][R + r];
        *yp = f2bf(g / (1.f + __expf(-g)) * u);
      } else if (EPI == RESID) {
        *yp = f2bf(bf2f(y_raw[m]) + bf2f(f2bf(acc[m][r])));
      } else {
        *yp = f2bf(acc[m][r]);
      }
    }
  }
}

// Rows (GLU: pairs) per wave from the 64-block k-steps of a wave's slice: NW * U = 4 with U no more than
// the steps there are (K = 2048, one slice: one step, so four rows / two pairs)
static int rows_for(int KB, int ks, int epi) {
  const int kbc = (KB + ks - 1) / ks;
  const int steps = (kbc + 63) / 64;
  const int nw = steps >= 4 ? 1 : (steps >= 2 ? 2 : 4);
  return epi == GLU || epi == ROPE_KV ? (nw >= 4 ? 2 : 1) : nw;
}

// k-slices per row group, as pick_ks of decode_fused.hip in units of blocks: split K while the grid
// stays <= 8192 waves and a slice keeps a full 64-block step (Llama-3.2-1B: o_proj 1, down 4,
// gate_up / lm_head 1)
static int pick_ks(int N, int KB, int epi) {
  int ks = 1;
  while (ks < 4 && KB / (ks * 2) >= 64) {
    const int r = rows_for(KB, ks * 2, epi);
    if ((int64_t)((N + r - 1) / r) * ks * 2 > 8192) break;
    ks *= 2;
  }
  return ks;
}

template <int MM, int R, int EPI, bool XI = false>
static int launch_ks(const Params& p, int ks, hipStream_t s) {
  const size_t lds = EPI != RESID ? (size_t)p.M * p.K * 2 : 0;
  int groups = (p.N + R - 1) / R;
  if (EPI == ROPE_KV) {   // row groups of R rotary pairs, then of 2 R v rows
    const int npair = (p.nq + p.nkv) * (p.D / 2);
    groups = (npair + R - 1) / R + (p.nkv * p.D + 2 * R - 1) / (2 * R);
  }
  const dim3 grid((unsigned)(((int64_t)groups * ks + 3) / 4)), block(256);
  if (ks == 4) hipLaunchKernelGGL((dgemv_mx_kernel<MM, R, EPI, 4, XI>), grid, block, lds, s, p);
  else if (ks == 2) hipLaunchKernelGGL((dgemv_mx_kernel<MM, R, EPI, 2, XI>), grid, block, lds, s, p);
  else hipLaunchKernelGGL((dgemv_mx_kernel<MM, R, EPI, 1, XI>), grid, block, lds, s, p);
  return hipGetLastError() == hipSuccess ? 0 : 1;
}

template <int MM, int EPI>
static int launch_r(const Params& p, int r, int ks, hipStream_t s) {
  if (r == 1) return launch_ks<MM, 1, EPI>(p, ks, s);
  if (r == 2) return launch_ks<MM, 2, EPI>(p, ks, s);
  if constexpr (EPI != GLU) {
    if (r == 4) return launch_ks<MM, 4, EPI>(p, ks, s);
  }
  return -6;
}

template <int MM>
static int launch_epi(const Params& p, int epi, int r, int ks, hipStream_t s) {
  if (epi == PLAIN) return launch_r<MM, PLAIN>(p, r, ks, s);
  if (epi == RESID) return launch_r<MM, RESID>(p, r, ks, s);
  if (epi == ROPE_KV) {
    if (r != 1 && r != 2) return -6;
    if (p.xidx) return r == 1 ? launch_ks<MM, 1, ROPE_KV, true>(p, ks, s) : launch_ks<MM, 2, ROPE_KV, true>(p, ks, s);
    return r == 1 ? launch_ks<MM, 1, ROPE_KV>(p, ks, s) : launch_ks<MM, 2, ROPE_KV>(p, ks, s);
  }
  return launch_r<MM, GLU>(p, r, ks, s);
}

}  // namespace dfused_mx

// cfg = 0: rows per wave and k-slices from the shape; cfg = 16 R + KS forces them (tests, tools/bench_mx_decode.py)
// rope (epi = 3 only, else null): the ROPE_KV operands
int dgemv_mx_launch(int epi, const void* x, int64_t ldx, const void* norm_w, float eps, const void* w, int64_t ldw,
                    const void* scale, int64_t lds, void* y, int64_t ldy, int M, int N, int K, int cfg, hipStream_t stream,
                    const DgemvMxRope* rope) {
  using namespace dfused_mx;
  if (epi < PLAIN || epi > ROPE_KV || (epi == ROPE_KV) != (rope != nullptr)) return -1;
  if (M < 1 || M > 3 || N < 1 || K < 32 || (K & 31)) return -1;
  if ((epi == RESID) != (norm_w == nullptr)) return -3;   // PLAIN / GLU carry the norm prologue, RESID does not
  if (norm_w && (size_t)M * K * 2 > 65536) return -2;
  if ((ldw & 15) || (reinterpret_cast<uintptr_t>(w) & 15) || (ldx & 7) || (reinterpret_cast<uintptr_t>(x) & 15)) return -4;
  const int KB = K / 32;
  // ROPE_KV: half the rows are the units a wave owns R of (pairs; two v rows), as GLU's N
  int ks = cfg ? (cfg & 15) : pick_ks(epi == ROPE_KV ? N / 2 : N, KB, epi);
  int r = cfg ? (cfg >> 4) : rows_for(KB, ks, epi);
  if (ks != 1 && ks != 2 && ks != 4) return -6;
  Params p{static_cast<const uint16_t*>(x), ldx, static_cast<const uint16_t*>(norm_w), static_cast<const uint8_t*>(w), ldw,
           static_cast<const uint8_t*>(scale), lds, static_cast<uint16_t*>(y), ldy, eps, M, N, K};
  if (epi == ROPE_KV) {
    const DgemvMxRope& q = *rope;
    if (q.nq < 1 || q.nkv < 1 || q.D < 2 || (q.D & 1) || (int64_t)(q.nq + 2 * q.nkv) * q.D != N || q.T < 1 || M % q.T ||
        q.max_pos < 1)
      return -1;
    if (q.xidx && q.xrows < 1) return -4;
    p.nq = q.nq, p.nkv = q.nkv, p.D = q.D;
    p.cos_t = q.cos_t, p.sin_t = q.sin_t, p.pos = q.pos, p.T = q.T;
    p.kc = static_cast<uint16_t*>(q.kc), p.vc = static_cast<uint16_t*>(q.vc);
    p.c_sb = q.c_sb, p.c_sh = q.c_sh, p.c_sl = q.c_sl;
    p.cache_idx = q.cache_idx, p.Lmax = q.Lmax, p.max_pos = q.max_pos;
    p.xidx = q.xidx, p.xrows = q.xrows, p.xcopy = static_cast<uint16_t*>(q.xcopy);
  }
  if (M == 1) return launch_epi<1>(p, epi, r, ks, stream);
  if (M == 2) return launch_epi<2>(p, epi, r, ks, stream);
  return launch_epi<4>(p, epi, r, ks, stream);
}

}  // namespace nxd
