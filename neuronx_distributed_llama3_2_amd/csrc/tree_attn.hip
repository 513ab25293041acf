// Tree-verification attention (Medusa): M = (Hq / Hkv) * N query rows per (sequence, kv head), N <= 64
// tree nodes, attend over the cached prefix [0, prefix_len[b]) -- visible to every row -- and then over
// the N tree keys, which are NOT in the cache (k_tree / v_tree, views of the QKV buffer) and are visible
// per node through one 64-bit mask word.  prefix_len is a device value: nothing about the launch depends
// on it, so a verification pass has static shapes.
//
// Work split.  Grid (batch x kv head, query-tile group, key split), four waves per workgroup.  A wave
// owns TPW 16-row query tiles (TPW = 1 / 2 / 4 by the number of tiles: up to 4 / 8 / any); their Q^T
// fragments and O accumulators (D / 16 f32x4 per tile) stay in registers for the whole sweep.  The
// register budget at D 128 sets the limit: TPW 4 there (128 O + 64 Q registers, then the scores of four
// tiles) compiled to 268 spilled VGPRs, so D 128 stops at TPW 2 (227 VGPRs + 144 AGPRs, no spill) and
// only D 64 takes TPW 4 (206 + 212, no spill).  Tiles are dealt to the waves round-robin (tile = group *
// 4 TPW + 4 i + wave) so a tree that leaves the last tiles empty still loads all four waves.
//
// Data movement.  The workgroup stages each 64-key K chunk and V chunk in LDS ONCE ([64][D + 8] bf16:
// the 16-byte row pad makes the 16 rows of a fragment read hit 16 different bank groups) and all its
// tiles consume it -- the decode kernel's waves each load their K rows straight from the cache, which
// at 256 rows would read the cache 16 times.  Two LDS buffers: the next chunk's global loads are
// issued into registers before this chunk's MFMAs and stored to the other buffer after them, one
// workgroup barrier per chunk.  A K fragment read from LDS feeds the score MFMAs of all TPW tiles.
//
//   S^T[key][m] = K.Q^T   v_mfma_f32_16x16x32_bf16, K fragments from LDS, lane (mi, g) then holds the
//                         scores of query row mi for keys 16 kt + 4 g + v;
//   softmax               online, log2 domain with the scale folded in, row max / sum over the 4 lanes
//                         of a row with two xor-shuffles (as decode_attn.hip);
//   O[m][d] += P.V        the reduction over the chunk's keys may run in any order, so k index 8 g + j of
//                         step ks stands for key 32 ks + 16 (j / 4) + 4 g + (j % 4): the lane's own
//                         scores ARE its A fragment (no lane shuffles), and the V B-fragment is two
//                         transposed reads (ds_read_b64_tr_b16) of rows 32 ks + 4 g .. + 3 and 16 below.
//
// Masking.  A prefix chunk below prefix_len costs nothing; the chunk holding key prefix_len - 1 takes
// the masked instantiation of the chunk body (workgroup-uniform branch).  Loads of rows past
// prefix_len are clamped to the last valid row, so what those rows hold (anything, NaN included) never
// reaches an MFMA.  The tree chunk is one extra chunk owned by the LAST split (with prefix_len below
// Lmax the least loaded one): score [key j][row m] is kept iff bit j (j < N) of the word of node m / G.
//
// Splits are sized from Lmax (tree_attn_splits: >= 256 keys each, enough of them for ~2 workgroups per
// CU).  A split with no visible key writes neutral partials (m = -inf, l = 0); tree_merge_kernel
// combines them.  With one split the workgroup writes bf16 output directly.  A row with no visible key
// at all yields zeros.  No atomics: results are bit-reproducible.
#include "common.h"
#include "tree_attn.h"

#include <algorithm>
#include <type_traits>

namespace nxd {
namespace tattn {

constexpr int KB = 64;      // keys per chunk
constexpr int NW = 4;       // waves per workgroup
constexpr int PAD = 8;      // bf16 of row padding in the LDS tiles
constexpr int MIN_KPS = 256;

constexpr size_t lds_bytes(int D) { return (size_t)2 * 2 * KB * (D + PAD) * 2; }   // 2 buffers x (K, V)

struct Params {
  const uint16_t* q;
  int64_t q_sb, q_sn, q_sh;
  const uint16_t* kt;
  const uint16_t* vt;
  int64_t t_sb, t_sn, t_sh;
  const uint64_t* mask;
  const uint16_t* kc;
  const uint16_t* vc;
  int64_t c_sb, c_sh, c_sl;
  const int* cache_idx;
  const int* prefix_len;
  uint16_t* out;
  int64_t o_sb, o_sn, o_sh;
  float* po;
  float* pm;
  float* pl;
  int B, N, Hq, Hkv, Bc, Lmax;
  int nsplit, kps;       // key splits; prefix keys per split (multiple of KB)
  float scale_log2;      // softmax scale * log2(e)
};
static_assert(std::is_trivially_copyable<Params>::value, "kernel-argument struct");

typedef __attribute__((address_space(3))) short4_t lds_s4_t;
typedef short short8_t __attribute__((ext_vector_type(8)));

template <int D, int TPW>
__global__ void __launch_bounds__(64 * NW) tree_attn_kernel(Params p) {
  constexpr int NS = D / 32;      // k-steps of the score MFMA
  constexpr int NDT = D / 16;     // 16-wide d tiles of the output
  constexpr int LD = D + PAD;     // LDS row stride
  constexpr int CPR = D / 8;      // 16-byte pieces per row
  constexpr int NL = KB * CPR / (64 * NW);   // pieces per thread per tile
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* lds = reinterpret_cast<uint16_t*>(smem);   // [2][K | V][KB][LD]
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int mi = lane & 15, g = lane >> 4;
  const int bh = blockIdx.x, grp = blockIdx.y, split = blockIdx.z;
  const int b = bh / p.Hkv, hkv = bh % p.Hkv;
  const int G = p.Hq / p.Hkv, M = G * p.N;
  const int cb = min(max(p.cache_idx ? p.cache_idx[b] : b, 0), p.Bc - 1);
  const int plen = min(max(p.prefix_len[b], 0), p.Lmax);
  const uint16_t* kbase = p.kc + (int64_t)cb * p.c_sb + (int64_t)hkv * p.c_sh;
  const uint16_t* vbase = p.vc + (int64_t)cb * p.c_sb + (int64_t)hkv * p.c_sh;
  const uint16_t* ktree = p.kt + (int64_t)b * p.t_sb + (int64_t)hkv * p.t_sh;
  const uint16_t* vtree = p.vt + (int64_t)b * p.t_sb + (int64_t)hkv * p.t_sh;

  // this split's chunks: its prefix keys [kbeg, kend), then (last split) the tree chunk
  const int kbeg = split * p.kps, kend = min(plen, kbeg + p.kps);
  const int npre = kend > kbeg ? (kend - kbeg + KB - 1) / KB : 0;
  const int nch = npre + (split == p.nsplit - 1 ? 1 : 0);

  // Q^T fragments of this wave's tiles: lane (mi, g) holds Q[row mi of the tile][32 s + 8 g .. + 7];
  // rows >= M are zero and see no tree key
  const int tile0 = grp * NW * TPW + wid;
  bf16x8_t qf[TPW][NS];
  uint64_t mw[TPW];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    const int m = (tile0 + NW * i) * 16 + mi;
    const int n = m / G, gg = m % G;
    mw[i] = 0;
    if (m < M) {
      const uint64_t w = p.mask[n];
      mw[i] = p.N >= 64 ? w : w & ((1ull << p.N) - 1);
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      u32x4_t v = {0, 0, 0, 0};
      if (m < M)
        v = *reinterpret_cast<const u32x4_t*>(p.q + (int64_t)b * p.q_sb + (int64_t)n * p.q_sn +
                                               (int64_t)(hkv * G + gg) * p.q_sh + 32 * s + 8 * g);
      qf[i][s] = __builtin_bit_cast(bf16x8_t, v);
    }
  }

  float run_m[TPW], run_l[TPW];   // stats of query row mi of each tile (log2 domain)
  f32x4_t o[TPW][NDT];
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
    run_m[i] = -INFINITY;
    run_l[i] = 0.f;
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt) o[i][dt] = f32x4_t{0.f, 0.f, 0.f, 0.f};
  }

  // chunk c -> registers (rows past the last valid one are clamped to it), registers -> LDS buffer
  u32x4_t kr[NL], vr[NL];
  auto gload = [&](int c) {
    const bool tree = c >= npre;
    const uint16_t* ks = tree ? ktree : kbase;
    const uint16_t* vs = tree ? vtree : vbase;
    const int64_t sl = tree ? p.t_sn : p.c_sl;
    const int k0 = tree ? 0 : kbeg + c * KB, last = tree ? p.N - 1 : plen - 1;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + 64 * NW * i, key = idx / CPR, c8 = idx % CPR;
      const int64_t off = (int64_t)min(k0 + key, last) * sl + 8 * c8;
      kr[i] = *reinterpret_cast<const u32x4_t*>(ks + off);
      vr[i] = *reinterpret_cast<const u32x4_t*>(vs + off);
    }
  };
  auto lstore = [&](int buf) {
    uint16_t* kt = lds + buf * 2 * KB * LD;
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + 64 * NW * i, key = idx / CPR, c8 = idx % CPR;
      *reinterpret_cast<u32x4_t*>(kt + key * LD + 8 * c8) = kr[i];
      *reinterpret_cast<u32x4_t*>(kt + KB * LD + key * LD + 8 * c8) = vr[i];
    }
  };

  // one chunk from LDS buffer buf; MASKED: vis[i] bit 4 kt + v tells whether this lane's score of key
  // 16 kt + 4 g + v is kept for tile i
  const bool wave_on = tile0 * 16 < M;
  auto chunk = [&](auto masked_c, int buf, const uint32_t* vis) {
    constexpr bool MASKED = decltype(masked_c)::value;
    const uint16_t* kt = lds + buf * 2 * KB * LD;
    const uint16_t* vt = kt + KB * LD;
    f32x4_t sc[TPW][4];
#pragma unroll
    for (int i = 0; i < TPW; ++i)
#pragma unroll
      for (int t = 0; t < 4; ++t) sc[i][t] = f32x4_t{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < 4; ++t)
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const u32x4_t kw = *reinterpret_cast<const u32x4_t*>(kt + (16 * t + mi) * LD + 32 * s + 8 * g);
        const bf16x8_t ka = __builtin_bit_cast(bf16x8_t, kw);
#pragma unroll
        for (int i = 0; i < TPW; ++i) sc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ka, qf[i][s], sc[i][t], 0, 0, 0);
      }
#pragma unroll
    for (int i = 0; i < TPW; ++i) {
      if ((tile0 + NW * i) * 16 >= M) continue;   // wave-uniform: an empty tile
      float cm = -INFINITY;
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          float sv = sc[i][t][v] * p.scale_log2;
          if constexpr (MASKED) sv = ((vis[i] >> (4 * t + v)) & 1u) ? sv : -INFINITY;
          sc[i][t][v] = sv;
          cm = fmaxf(cm, sv);
        }
      cm = fmaxf(cm, __shfl_xor(cm, 16, 64));
      cm = fmaxf(cm, __shfl_xor(cm, 32, 64));
      const float nm = fmaxf(run_m[i], cm);
      const float mu = nm == -INFINITY ? 0.f : nm;
      const float alpha = run_m[i] == -INFINITY ? 0.f : exp2f(run_m[i] - mu);
      float ls = 0.f;
      uint32_t p2[4][2];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        float e[4];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          e[v] = exp2f(sc[i][t][v] - mu);
          ls += e[v];
        }
        p2[t][0] = pack2bf(e[0], e[1]);
        p2[t][1] = pack2bf(e[2], e[3]);
      }
      ls += __shfl_xor(ls, 16, 64);
      ls += __shfl_xor(ls, 32, 64);
      run_l[i] = run_l[i] * alpha + ls;
      run_m[i] = nm;
      // rescale O rows 4 g + v by their row's alpha (held by lane 4 g + v)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float a = __shfl(alpha, 4 * g + v, 64);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) o[i][dt][v] *= a;
      }
      // P.V with k index 8 g + j of step ks <-> key 32 ks + 16 (j / 4) + 4 g + (j % 4)
      const int qrow = mi >> 2, pc = mi & 3;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const u32x4_t pw = {p2[2 * ks][0], p2[2 * ks][1], p2[2 * ks + 1][0], p2[2 * ks + 1][1]};
        const bf16x8_t pf = __builtin_bit_cast(bf16x8_t, pw);
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
          const uint16_t* a = vt + (32 * ks + 4 * g + qrow) * LD + 16 * dt + 4 * pc;
          const short4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)a);
          const short4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s4_t*)(a + 16 * LD));
          const short8_t v8 = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          o[i][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pf, __builtin_bit_cast(bf16x8_t, v8), o[i][dt], 0, 0, 0);
        }
      }
    }
  };

  if (nch > 0) {
    gload(0);
    lstore(0);
  }
  __syncthreads();
  for (int c = 0; c < nch; ++c) {
    if (c + 1 < nch) gload(c + 1);   // in flight while this chunk's MFMAs run
    if (wave_on) {
      const bool tree = c >= npre;
      if (tree || kbeg + (c + 1) * KB > plen) {   // the tree chunk, or the one holding key prefix_len - 1
        uint32_t vis[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
          vis[i] = 0;
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            const int rest = plen - (kbeg + c * KB + 16 * t + 4 * g);   // prefix keys from this lane's first on
            const uint32_t pre = rest >= 4 ? 0xFu : rest <= 0 ? 0u : (1u << rest) - 1u;
            vis[i] |= (tree ? (uint32_t)(mw[i] >> (16 * t + 4 * g)) & 0xFu : pre) << (4 * t);
          }
        }
        chunk(std::true_type{}, c & 1, vis);
      } else {
        chunk(std::false_type{}, c & 1, nullptr);
      }
    }
    if (c + 1 < nch) lstore((c + 1) & 1);
    __syncthreads();
  }

  // ---- results: lane holds O[row 4 g + v][16 dt + mi] of each tile; the row's stats sit in lane 4 g + v
  const int64_t pbase = ((int64_t)bh * p.nsplit + split) * M;
#pragma unroll
  for (int i = 0; i < TPW; ++i) {
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const float L = __shfl(run_l[i], 4 * g + v, 64), mx = __shfl(run_m[i], 4 * g + v, 64);
      const int m = (tile0 + NW * i) * 16 + 4 * g + v;
      if (m >= M) continue;
      if (p.nsplit == 1) {
        const float inv = L > 0.f ? 1.f / L : 0.f;
        uint16_t* dst = p.out + (int64_t)b * p.o_sb + (int64_t)(m / G) * p.o_sn + (int64_t)(hkv * G + m % G) * p.o_sh + mi;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) dst[16 * dt] = f2bf(o[i][dt][v] * inv);
      } else {
        float* dst = p.po + (pbase + m) * D + mi;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) dst[16 * dt] = o[i][dt][v];
        if (mi == 0) {
          p.pm[pbase + m] = mx;
          p.pl[pbase + m] = L;
        }
      }
    }
  }
}

// Split partials -> bf16 output: one workgroup of D threads per (batch, kv head, query row)
template <int D>
__global__ void __launch_bounds__(D) tree_merge_kernel(Params p) {
  const int G = p.Hq / p.Hkv, M = G * p.N;
  const int bh = blockIdx.x / M, m = blockIdx.x % M, d = threadIdx.x;
  const int b = bh / p.Hkv, hkv = bh % p.Hkv;
  const int64_t base = (int64_t)bh * p.nsplit * M + m;
  float gm = -INFINITY;
  for (int s = 0; s < p.nsplit; ++s) gm = fmaxf(gm, p.pm[base + (int64_t)s * M]);
  float L = 0.f, acc = 0.f;
  for (int s = 0; s < p.nsplit; ++s) {
    const float ms = p.pm[base + (int64_t)s * M];
    if (ms == -INFINITY) continue;   // block-uniform: a split that saw no key
    const float w = exp2f(ms - gm);
    L += w * p.pl[base + (int64_t)s * M];
    acc += w * p.po[(base + (int64_t)s * M) * D + d];
  }
  p.out[(int64_t)b * p.o_sb + (int64_t)(m / G) * p.o_sn + (int64_t)(hkv * G + m % G) * p.o_sh + d] =
      f2bf(L > 0.f ? acc / L : 0.f);
}

// tiles per wave for M query rows: as few as cover them in one tile group, up to 4 (D 64) / 2 (D 128)
static int tiles_per_wave(int M, int D) {
  const int tiles = (M + 15) / 16;
  return tiles <= NW ? 1 : (tiles <= 2 * NW || D == 128) ? 2 : 4;
}

// CUs of the current device, asked on every call (a cached attribute of the runtime: no state of ours to
// go stale in a multi-device or multi-threaded process); 256 (MI355X) if the runtime will not say
static int compute_units() {
  int dev = 0, n = 0;
  if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0)
    n = 256;
  return n;
}

static bool covered(int B, int N, int Hq, int Hkv, int D, int Lmax) {
  if (B < 1 || N < 1 || N > 64 || Hkv < 1 || Hq < Hkv || Hq % Hkv || (D != 64 && D != 128) || Lmax < 1) return false;
  return (int64_t)(Hq / Hkv) * N <= 512 && (int64_t)B * Hkv <= INT32_MAX / 1024;
}

// prefix keys per split (a multiple of KB, at least MIN_KPS): enough splits for two workgroups per CU
static int keys_per_split(int B, int N, int Hq, int Hkv, int D, int Lmax) {
  const int M = (Hq / Hkv) * N, tpw = tiles_per_wave(M, D);
  const int64_t wgs = (int64_t)B * Hkv * ceil_div(ceil_div(M, 16), NW * tpw);
  const int64_t want = std::max<int64_t>(1, 2 * compute_units() / wgs);
  const int64_t kps = ceil_div64(ceil_div64(Lmax, want), KB) * KB;
  return (int)std::max<int64_t>(kps, MIN_KPS);
}

template <int D, int TPW>
static hipError_t launch_attn(dim3 grid, hipStream_t stream, const Params& p) {
  auto kernel = tree_attn_kernel<D, TPW>;
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)lds_bytes(D));
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kernel, grid, dim3(64 * NW), lds_bytes(D), stream, p);
  return hipGetLastError();
}

}  // namespace tattn

int tree_attn_splits(int B, int N, int Hq, int Hkv, int D, int Lmax) {
  if (!tattn::covered(B, N, Hq, Hkv, D, Lmax)) return -1;
  return ceil_div(Lmax, tattn::keys_per_split(B, N, Hq, Hkv, D, Lmax));
}

int tree_attn_launch(const TreeAttnArgs& a, int nsplit) {
  using namespace tattn;
  if (!covered(a.B, a.N, a.Hq, a.Hkv, a.D, a.Lmax) || a.Bc < 1) return -1;
  const int kps = keys_per_split(a.B, a.N, a.Hq, a.Hkv, a.D, a.Lmax);
  if (nsplit != ceil_div(a.Lmax, kps) || nsplit > 65535) return -1;
  if (nsplit > 1 && (a.po == nullptr || a.pm == nullptr || a.pl == nullptr)) return -1;
  Params p{};
  p.q = static_cast<const uint16_t*>(a.q); p.q_sb = a.q_sb; p.q_sn = a.q_sn; p.q_sh = a.q_sh;
  p.kt = static_cast<const uint16_t*>(a.k_tree); p.vt = static_cast<const uint16_t*>(a.v_tree);
  p.t_sb = a.t_sb; p.t_sn = a.t_sn; p.t_sh = a.t_sh;
  p.mask = a.mask_words;
  p.kc = static_cast<const uint16_t*>(a.kc); p.vc = static_cast<const uint16_t*>(a.vc);
  p.c_sb = a.c_sb; p.c_sh = a.c_sh; p.c_sl = a.c_sl;
  p.cache_idx = a.cache_idx; p.prefix_len = a.prefix_len;
  p.out = static_cast<uint16_t*>(a.out); p.o_sb = a.o_sb; p.o_sn = a.o_sn; p.o_sh = a.o_sh;
  p.po = a.po; p.pm = a.pm; p.pl = a.pl;
  p.B = a.B; p.N = a.N; p.Hq = a.Hq; p.Hkv = a.Hkv; p.Bc = a.Bc; p.Lmax = a.Lmax;
  p.nsplit = nsplit; p.kps = kps;
  p.scale_log2 = a.scale * 1.44269504088896340736f;
  const int M = (a.Hq / a.Hkv) * a.N, tpw = tiles_per_wave(M, a.D);
  const dim3 grid(a.B * a.Hkv, ceil_div(ceil_div(M, 16), NW * tpw), nsplit);
  hipError_t e;
  if (a.D == 64)
    e = tpw == 1 ? launch_attn<64, 1>(grid, a.stream, p) : tpw == 2 ? launch_attn<64, 2>(grid, a.stream, p) : launch_attn<64, 4>(grid, a.stream, p);
  else
    e = tpw == 1 ? launch_attn<128, 1>(grid, a.stream, p) : launch_attn<128, 2>(grid, a.stream, p);
  if (e != hipSuccess) return (int)e;
  if (nsplit > 1) {
    if (a.D == 64)
      hipLaunchKernelGGL(tree_merge_kernel<64>, dim3(a.B * a.Hkv * M), dim3(64), 0, a.stream, p);
    else
      hipLaunchKernelGGL(tree_merge_kernel<128>, dim3(a.B * a.Hkv * M), dim3(128), 0, a.stream, p);
    e = hipGetLastError();
  }
  return (int)e;
}

}  // namespace nxd
