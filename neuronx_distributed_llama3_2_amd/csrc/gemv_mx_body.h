// Body of the MXFP4 skinny-GEMM kernels of gemv_mx.hip, included inside a kernel template
// <int MM, int ROWS, bool GLU> that has a `Params p` in scope (the dense kernel's argument, or the
// per-pair operands the expert kernel derives): wave (blockIdx.x * 4 + wave in block) owns ROWS
// output columns of the one [M, K] x [Nw, K]^T product p describes.  Kept as text, not as a device
// function, so that the dense kernel compiles to exactly the code it had before the expert kernel
// shared it.
  constexpr int NW = GLU ? 2 * ROWS : ROWS;  // weight rows per wave
  const int lane = threadIdx.x & 63;
  const int wave = (blockIdx.x * 4) + (threadIdx.x >> 6);
  const int n0 = wave * ROWS;
  if (n0 >= p.N) return;
  int wrow[NW];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int n = min(n0 + r, p.N - 1);  // rows past N are clamped (and not stored)
    wrow[r] = n;
    if (GLU) wrow[ROWS + r] = n + p.N;
  }
  float acc[MM][NW];
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < NW; ++r) acc[m][r] = 0.f;

  const int KB = p.K >> 5;  // blocks per row; lanes past it do nothing
  for (int kb = lane; kb < KB; kb += 64) {
    u32x4_t wv[NW];
    float sc[NW];
#pragma unroll
    for (int r = 0; r < NW; ++r) {
      wv[r] = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t*>(p.w + (int64_t)wrow[r] * p.ldw + (int64_t)kb * 16));
      sc[r] = e8m0(p.scale[(int64_t)wrow[r] * p.lds + kb]);
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
      W8 wb[NW];
#pragma unroll
      for (int r = 0; r < NW; ++r) wb[r] = cvt8(wv[r][d], sc[r]);
#pragma unroll
      for (int m = 0; m < MM; ++m) {
        if (m < p.M) {
          const u32x4_t xv = *reinterpret_cast<const u32x4_t*>(p.x + (int64_t)m * p.ldx + (int64_t)kb * 32 + d * 8);
#pragma unroll
          for (int r = 0; r < NW; ++r) acc[m][r] = dot8(xv, wb[r], acc[m][r]);
        }
      }
    }
  }
#pragma unroll
  for (int m = 0; m < MM; ++m)
#pragma unroll
    for (int r = 0; r < NW; ++r) acc[m][r] = wave_sum(acc[m][r]);
  if (lane != 0) return;
#pragma unroll
  for (int m = 0; m < MM; ++m) {
    if (m >= p.M) continue;
#pragma unroll
    for (int r = 0; r < ROWS; ++r) {
      const int n = n0 + r;
      if (n >= p.N) continue;
      float v = acc[m][r];
      if (p.bias) v += bf2f(p.bias[wrow[r]]);
      if (GLU) {
        float u = acc[m][ROWS + r];
        if (p.bias) u += bf2f(p.bias[wrow[ROWS + r]]);
        v = v / (1.f + __expf(-v)) * u;
      }
      p.y[(int64_t)m * p.ldy + n] = f2bf(v);
    }
  }
