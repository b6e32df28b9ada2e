// dmf_pca.hip — band reduction of the primary scene: the two device stages of a PCA in front of the network.
//   band_sum_kernel / band_mean_kernel     mean [C] in double, a fixed tree
//   band_cov_kernel / band_cov_finish      cov [C][C] in double from fp32 products on the fp32 matrix cores
//   band_project_kernel                    y [N][K] = (x - mean) basis, one pass over x, on the fp32 matrix cores
// The eigen-decomposition between them runs on the host in float64 (utils/spectral.py).  The entry points dmf_band_moments and
// dmf_band_project live here too (host code at the end of the file) and report by return code, as dmf_spatial.hip's do.  No
// float atomics, every sum in a fixed order that depends on (N, C) only: the same bits on every run.  No BLAS.
//
// Products.  v_mfma_f32_16x16x4_f32 is bit for bit a k-ordered fmaf chain (exact fp32, no reduced-precision path on gfx950).
// Lane l gives A[l & 15][l >> 4] and B[l >> 4][l & 15] and gets D[4 (l >> 4) + r][l & 15] in register r.
//   * covariance: k is the pixel.  A workgroup of 4 waves owns one 64 x 64 macro tile (I <= J) of band pairs and a slice of the
//     pixels; wave w owns the 16-band row strip w and the column tiles t of it that lie in the upper triangle (t >= w where
//     I == J).  Pixels go through LDS 64 at a time as d = x - (float)mean, [pixel][band] with a pixel DMF_PCA_LDS
//     = 80 floats apart (the 4 pixels of one operand fall on banks 16 apart: no conflict), zero-filled past C and past the
//     run's end (a zero adds +0 to the chain).  Both sides are staged, also where they are the same bands.  The fp32 accumulators cover one run
//     of DMF_PCA_RUN pixels (runs are [q R, (q + 1) R) of the pixel index, whatever the slicing), then are added to double
//     accumulators in registers and cleared: a slice adds its runs in ascending order, the finishing launch adds the slices
//     in ascending order, divides by N - 1 and writes cov[i][j] and cov[j][i] from the one sum.
//   * projection: k is the band.  A workgroup owns 64 pixels, wave w 16 of them and all K columns (NT = ceil(K / 16) column
//     tiles, NT accumulators); bands go through LDS 64 at a time, the centred pixels [pixel][band] 68 floats apart (16 pixels
//     x 4 bands of one operand: 64 different banks), the basis rows [band][k] 80 apart.  y[n][k] is one fmaf chain over the
//     bands in ascending order.
// Means.  A slice of pixels and 64 bands per workgroup; thread (g, b) sums band b of the pixels n0 + g + 4 i in double as four
// interleaved chains (i mod 4), added (s0 + s1) + (s2 + s3); the four g of a band are added (0 + 1) + (2 + 3); band_mean_kernel
// adds the slices as 16 interleaved chains and a fixed tree, and divides by N.
// All global offsets are 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_pca_tiles.h"               // the constants, pca_plan, pca_pair_index and cov_steps: shared with dmf_noise.hip

namespace dmf {

constexpr int PROJ_PX = 64;              // pixels per workgroup of the projection
constexpr int PROJ_CB = 64;              // bands per LDS chunk of the projection
constexpr int PROJ_XS = 68;              // floats from one staged pixel to the next

// ------------------------------------------------------------------------------ means
__global__ __launch_bounds__(256) void band_sum_kernel(const float* __restrict__ x, int64_t N, int C, int64_t pitch,
                                                       int64_t px_per_slice, double* __restrict__ part /* [slices][C] */) {
  __shared__ double sums[4][64];
  const int b = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int64_t n0 = (int64_t)blockIdx.x * px_per_slice;
  const int64_t n1 = n0 + px_per_slice < N ? n0 + px_per_slice : N;
  const int c = blockIdx.y * 64 + b;                     // one group of 64 bands per blockIdx.y
  double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
  if (c < C) {
    const float* col = x + c;
    int64_t n = n0 + g;
    for (; n + 12 < n1; n += 16) {
      const float v0 = col[n * pitch], v1 = col[(n + 4) * pitch], v2 = col[(n + 8) * pitch], v3 = col[(n + 12) * pitch];
      s0 += (double)v0; s1 += (double)v1; s2 += (double)v2; s3 += (double)v3;
    }
    if (n < n1) s0 += (double)col[n * pitch];
    if (n + 4 < n1) s1 += (double)col[(n + 4) * pitch];
    if (n + 8 < n1) s2 += (double)col[(n + 8) * pitch];
  }
  sums[g][b] = (s0 + s1) + (s2 + s3);
  __syncthreads();
  if (g == 0 && c < C) part[(int64_t)blockIdx.x * C + c] = (sums[0][b] + sums[1][b]) + (sums[2][b] + sums[3][b]);
}

// mean[c] = (the slices' sums: 16 interleaved chains, slice q in chain q % 16, then the fixed tree ((0 + 8) + (4 + 12)) + ...) / N
__global__ __launch_bounds__(1024) void band_mean_kernel(const double* __restrict__ part, int slices, int C, int64_t N,
                                                         double* __restrict__ mean) {
  __shared__ double t[16][64];
  const int b = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int c = blockIdx.x * 64 + b;
  double s = 0.;
  if (c < C) {
#pragma unroll 4
    for (int q = g; q < slices; q += 16) s += part[(int64_t)q * C + c];
  }
  t[g][b] = s;
  __syncthreads();
  if (g != 0 || c >= C) return;
  double v[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) v[i] = t[i][b];
#pragma unroll
  for (int w = 8; w > 0; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) v[i] += v[i + w];
  mean[c] = v[0] / (double)N;
}

// ------------------------------------------------------------------------------ covariance
// (pca_pair_index and cov_steps, the products of one staged chunk: dmf_pca_tiles.h)
__global__ __launch_bounds__(256) void band_cov_kernel(const float* __restrict__ x, int64_t N, int C, int64_t pitch,
                                                       const double* __restrict__ mean, int Cm, int64_t runs, int64_t runs_per_slice,
                                                       double* __restrict__ part /* [slices][pairs][64][64] */) {
  __shared__ float da[PCA_PX * PCA_LDS], db[PCA_PX * PCA_LDS];
  __shared__ float ma[PCA_MT], mb[PCA_MT];
  int I = 0, J = (int)blockIdx.x;                        // pair index -> (I, J), I <= J, row by row of the upper triangle
  while (J >= Cm - I) { J -= Cm - I; ++I; }
  J += I;
  const bool diag = I == J;
  if (threadIdx.x < 2 * PCA_MT) {
    const int c = (threadIdx.x < PCA_MT ? I : J) * PCA_MT + (threadIdx.x & (PCA_MT - 1));
    (threadIdx.x < PCA_MT ? ma : mb)[threadIdx.x & (PCA_MT - 1)] = c < C ? (float)mean[c] : 0.f;
  }
  __syncthreads();
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, lk = l >> 4, li = l & 15;
  // column tiles t0 .. 3 of the wave's row strip are computed: those of the upper triangle (a strip past C: none).  Of a macro
  // tile that C cuts, the column tiles past C are zero-filled, computed and dropped: no branch inside the chunk's products.
  const int t0 = I * PCA_MT + 16 * w >= C ? 4 : diag ? w : 0;
  bool on[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) on[t] = t >= t0 && J * PCA_MT + 16 * t < C;
  double dacc[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dacc[t][r] = 0.;
  const int64_t run0 = (int64_t)blockIdx.y * runs_per_slice;
  const int64_t run1 = run0 + runs_per_slice < runs ? run0 + runs_per_slice : runs;
  const int64_t pbeg = run0 * PCA_R, pend = run1 * PCA_R < N ? run1 * PCA_R : N;      // this slice's pixels: whole runs, the last to N

  // Thread (sp, sc) stages band sc of the pixels p0 + sp + 4 q of a chunk.  The loads are UNCONDITIONAL, from a clamped pixel
  // and band, and masked when they are stored (a load under a lane condition becomes a branch with its own wait); the loads of
  // chunk k + 1 are issued before the products of chunk k.
  constexpr int NQ = PCA_PX * PCA_MT / 256;
  const int sp = threadIdx.x >> 6, sc = threadIdx.x & 63;
  const int ca = I * PCA_MT + sc, cb = J * PCA_MT + sc;
  const float* xa = x + (ca < C ? ca : C - 1);
  const float* xb = x + (cb < C ? cb : C - 1);
  const float m_a = ma[sc], m_b = mb[sc];
  float va[NQ], vb[NQ];
  auto issue = [&](int64_t p0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int64_t n = p0 + sp + 4 * q < N ? p0 + sp + 4 * q : N - 1;
      va[q] = xa[n * pitch];
      vb[q] = xb[n * pitch];                             // (a diagonal tile reads the same address twice: no branch here)
    }
  };
  pca_f32x4 acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = (pca_f32x4){0.f, 0.f, 0.f, 0.f};
  issue(pbeg);
  for (int64_t p0 = pbeg; p0 < pend; p0 += PCA_PX) {
    if (p0 != pbeg && p0 % PCA_R == 0) {                 // (uniform) a run is complete: its fp32 sums go to the double ones
#pragma unroll
      for (int t = 0; t < 4; ++t) {
#pragma unroll
        for (int r = 0; r < 4; ++r) dacc[t][r] += (double)acc[t][r];
        acc[t] = (pca_f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    __syncthreads();                                     // the previous chunk has been read
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const bool in = p0 + sp + 4 * q < pend;            // zero-filled past the slice's (= the scene's) end and past C
      da[(sp + 4 * q) * PCA_LDS + sc] = in && ca < C ? va[q] - m_a : 0.f;
      db[(sp + 4 * q) * PCA_LDS + sc] = in && cb < C ? vb[q] - m_b : 0.f;
    }
    if (p0 + PCA_PX < pend) issue(p0 + PCA_PX);
    __syncthreads();
    const float* pa = da + lk * PCA_LDS + 16 * w + li;
    const float* pb = db + lk * PCA_LDS + li;
    switch (t0) {                                        // (uniform) the wave's first column tile; 4: nothing to do
      case 0: cov_steps<0>(pa, pb, acc); break;
      case 1: cov_steps<1>(pa, pb, acc); break;
      case 2: cov_steps<2>(pa, pb, acc); break;
      case 3: cov_steps<3>(pa, pb, acc); break;
      default: break;
    }
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) dacc[t][r] += (double)acc[t][r];
  double* out = part + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (PCA_MT * PCA_MT);
#pragma unroll
  for (int t = 0; t < 4; ++t)
    if (on[t]) {
#pragma unroll
      for (int r = 0; r < 4; ++r) out[(16 * w + 4 * lk + r) * PCA_MT + 16 * t + li] = dacc[t][r];
    }
}

// cov[i][j] = cov[j][i] = (the slices' partial sums, in ascending order) / (N - 1); one thread per (i, j), i <= j
__global__ __launch_bounds__(256) void band_cov_finish_kernel(const double* __restrict__ part, int slices, int pairs, int Cm, int C,
                                                              int64_t N, double* __restrict__ cov) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * C) return;
  const int i = idx / C, j = idx - i * C;
  if (i > j) return;
  const double* p = part + (int64_t)pca_pair_index(i >> 6, j >> 6, Cm) * (PCA_MT * PCA_MT) + (i & 63) * PCA_MT + (j & 63);
  double s = 0.;
  for (int q = 0; q < slices; ++q) s += p[(int64_t)q * pairs * (PCA_MT * PCA_MT)];
  const double v = s / (double)(N - 1);
  cov[(int64_t)i * C + j] = v;
  cov[(int64_t)j * C + i] = v;
}

// ------------------------------------------------------------------------------ projection
template <int NT>
__global__ __launch_bounds__(256) void band_project_kernel(const float* __restrict__ x, int64_t N, int C, int64_t pitch,
                                                           const double* __restrict__ mean, const float* __restrict__ basis, int K,
                                                           float* __restrict__ y) {
  __shared__ float xs[PROJ_PX * PROJ_XS];                // [pixel][band] of the chunk, centred
  __shared__ float bs[PROJ_CB * PCA_LDS];                // [band][k] of the chunk
  __shared__ float mf[512];
  for (int c = threadIdx.x; c < C; c += 256) mf[c] = (float)mean[c];
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, lk = l >> 4, li = l & 15;
  const int64_t p0 = (int64_t)blockIdx.x * PROJ_PX;
  pca_f32x4 acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (pca_f32x4){0.f, 0.f, 0.f, 0.f};

  // Thread (sp, sc) stages band c0 + sc of the pixels p0 + sp + 4 q, and elements threadIdx.x + 256 q of the chunk's [64][16 NT]
  // basis block.  Unconditional loads from clamped addresses, masked when stored; the loads of chunk k + 1 are issued before
  // the products of chunk k (band_cov_kernel).
  constexpr int NQ = PROJ_PX * PROJ_CB / 256, KW = 16 * NT, NB = PROJ_CB * KW / 256;
  const int sp = threadIdx.x >> 6, sc = threadIdx.x & 63;
  float vx[NQ], vbs[NB];
  auto issue = [&](int c0) __attribute__((always_inline)) {
    const float* xc = x + (c0 + sc < C ? c0 + sc : C - 1);
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int64_t n = p0 + sp + 4 * q < N ? p0 + sp + 4 * q : N - 1;
      vx[q] = xc[n * pitch];
    }
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int idx = threadIdx.x + 256 * q, r = idx / KW, k = idx - r * KW;
      vbs[q] = basis[(int64_t)(c0 + r < C ? c0 + r : C - 1) * K + (k < K ? k : K - 1)];
    }
  };
  issue(0);
  for (int c0 = 0; c0 < C; c0 += PROJ_CB) {
    __syncthreads();                                     // mf is written; the previous chunk has been read
    const bool cin = c0 + sc < C;
    const float m = cin ? mf[c0 + sc] : 0.f;
#pragma unroll
    for (int q = 0; q < NQ; ++q) xs[(sp + 4 * q) * PROJ_XS + sc] = cin && p0 + sp + 4 * q < N ? vx[q] - m : 0.f;
#pragma unroll
    for (int q = 0; q < NB; ++q) {
      const int idx = threadIdx.x + 256 * q, r = idx / KW, k = idx - r * KW;
      bs[r * PCA_LDS + k] = c0 + r < C && k < K ? vbs[q] : 0.f;
    }
    if (c0 + PROJ_CB < C) issue(c0 + PROJ_CB);
    __syncthreads();
    const int steps = C - c0 < PROJ_CB ? (C - c0 + 3) / 4 : PROJ_CB / 4;     // (uniform) whole steps up to the last band
    if (steps == PROJ_CB / 4) {
#pragma unroll
      for (int kk = 0; kk < PROJ_CB / 4; ++kk) {
        const float a = xs[(16 * w + li) * PROJ_XS + 4 * kk + lk];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[(4 * kk + lk) * PCA_LDS + 16 * t + li], acc[t], 0, 0, 0);
      }
    } else {
      for (int kk = 0; kk < steps; ++kk) {
        const float a = xs[(16 * w + li) * PROJ_XS + 4 * kk + lk];
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bs[(4 * kk + lk) * PCA_LDS + 16 * t + li], acc[t], 0, 0, 0);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int64_t n = p0 + 16 * w + 4 * lk + r;
      const int k = 16 * t + li;
      if (n < N && k < K) y[n * K + k] = acc[t][r];
    }
}

template <int NT>
static hipError_t project_launch(unsigned blocks, const float* x, int64_t N, int C, int64_t pitch, const double* mean, const float* basis,
                                 int K, float* y, hipStream_t st) {
  hipLaunchKernelGGL(band_project_kernel<NT>, dim3(blocks), dim3(256), 0, st, x, N, C, pitch, mean, basis, K, y);
  return hipGetLastError();
}

}  // namespace dmf

using namespace dmf;

extern "C" {

// Return codes (include/dmf.h lists them): this file has no access to the text buffer of dmf_last_error.
int64_t dmf_band_moments_workspace_bytes(int64_t N, int32_t C) {
  if (N < 2 || C < 1 || C > 512) return -1;
  const PcaPlan p = pca_plan(N, C);
  return ((int64_t)p.mslices * C + (int64_t)p.slices * p.pairs * (PCA_MT * PCA_MT)) * (int64_t)sizeof(double);
}

int32_t dmf_band_moments(const float* x, int64_t N, int32_t C, int64_t pitch, double* mean, double* cov, void* workspace, void* stream) {
  if (x == nullptr || mean == nullptr || cov == nullptr || workspace == nullptr) return 1;
  if (N < 2) return 2;
  if (C < 1 || C > 512) return 3;
  if (pitch < C) return 5;
  if (reinterpret_cast<uintptr_t>(x) % 4 || reinterpret_cast<uintptr_t>(mean) % 8 || reinterpret_cast<uintptr_t>(cov) % 8 ||
      reinterpret_cast<uintptr_t>(workspace) % 8)
    return 6;
  if (!pca_extent_ok(N, pitch)) return 8;
  const PcaPlan p = pca_plan(N, C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* mpart = static_cast<double*>(workspace);
  double* cpart = mpart + (int64_t)p.mslices * C;
  hipLaunchKernelGGL(band_sum_kernel, dim3(p.mslices, (C + 63) / 64), dim3(256), 0, st, x, N, C, pitch, p.px_per_slice, mpart);
  if (hipGetLastError() != hipSuccess) return 9;
  hipLaunchKernelGGL(band_mean_kernel, dim3((C + 63) / 64), dim3(1024), 0, st, mpart, p.mslices, C, N, mean);
  if (hipGetLastError() != hipSuccess) return 9;
  hipLaunchKernelGGL(band_cov_kernel, dim3(p.pairs, p.slices), dim3(256), 0, st, x, N, C, pitch, mean, p.Cm, p.runs, p.runs_per_slice,
                     cpart);
  if (hipGetLastError() != hipSuccess) return 9;
  hipLaunchKernelGGL(band_cov_finish_kernel, dim3((C * C + 255) / 256), dim3(256), 0, st, cpart, p.slices, p.pairs, p.Cm, C, N, cov);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

int32_t dmf_band_project(const float* x, int64_t N, int32_t C, int64_t pitch, const double* mean, const float* basis, int32_t K, float* y,
                         void* stream) {
  if (N < 0) return 2;
  if (C < 1 || C > 512) return 3;
  if (K < 1 || K > 64 || K > C) return 4;
  if (pitch < C) return 5;
  if (N == 0) return 0;
  if (x == nullptr || mean == nullptr || basis == nullptr || y == nullptr) return 1;
  if (reinterpret_cast<uintptr_t>(x) % 4 || reinterpret_cast<uintptr_t>(mean) % 8 || reinterpret_cast<uintptr_t>(basis) % 4 ||
      reinterpret_cast<uintptr_t>(y) % 4)
    return 6;
  const int64_t blocks = (N + PROJ_PX - 1) / PROJ_PX;
  if (!pca_extent_ok(N, pitch) || blocks > INT32_MAX) return 8;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const int nt = (K + 15) / 16;
  const hipError_t e = nt == 1   ? project_launch<1>((unsigned)blocks, x, N, C, pitch, mean, basis, K, y, st)
                       : nt == 2 ? project_launch<2>((unsigned)blocks, x, N, C, pitch, mean, basis, K, y, st)
                       : nt == 3 ? project_launch<3>((unsigned)blocks, x, N, C, pitch, mean, basis, K, y, st)
                                 : project_launch<4>((unsigned)blocks, x, N, C, pitch, mean, basis, K, y, st);
  return e == hipSuccess ? 0 : 9;
}

}  // extern "C"
