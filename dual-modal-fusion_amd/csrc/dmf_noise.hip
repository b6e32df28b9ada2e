// dmf_noise.hip — the noise moments of the primary scene: the device stage that `band_reduce_noise` adds in
// front of the noise-adjusted fit (utils/spectral.py, fit_noise_adjusted).
//   band_noise_kernel<DIR> / band_noise_finish_kernel     ncov [C][C] in double from fp32 products of shift differences
// The scene is H x W pixels of C bands, flat pixel p = row W + column.  With s = 1 (DIR 0, the right neighbour) or s = W (DIR 1,
// the pixel below), e_p = x[p] - x[p + s] in fp32 where pixel p has that neighbour and e_p = 0 where it has not (the last
// column, the last row); M pixels have it; ncov = sum_p e_p e_p^T / (2 M), uncentred.
//
// The arithmetic is band_cov_kernel's (dmf_pca.hip; the shared pieces are dmf_pca_tiles.h), with e in the place of d: a
// workgroup of 4 waves owns one 64 x 64 macro tile (I <= J) of band pairs and a slice of whole runs, wave w the 16-band row
// strip w and its column tiles of the upper triangle; pixels go through LDS 64 at a time, [pixel][band] PCA_LDS = 80 floats
// apart (ds_read_b32 banks are (address / 4) mod 32 per half wave: the lanes of a half read 16 consecutive bands of 2 pixels 80
// apart, banks li + 16 lk, no conflict; the stores are 64 consecutive floats); the products are v_mfma_f32_16x16x4_f32 with the
// pixel as k, one fp32 fmaf chain per run [q R, (q + 1) R) of the flat pixel index in pixel order, the runs added in double in
// registers in ascending order, the slices in ascending order by the finishing launch, which divides by 2 M in double and writes
// ncov[i][j] and ncov[j][i] from the one sum.  The product loop has no branch: tiles past C are zero-filled and dropped.
//
// The differences are formed when a chunk is staged.  Both operands are loaded unconditionally from clamped addresses — the
// pixel min(p, N - 1) and the neighbour min(p + s, N - 1), the band min(c, C - 1) — one chunk ahead of the products, and the
// staged value is SELECTED: (p inside the slice, c < C, p has the neighbour) ? a - b : 0.  Nothing outside the H W C values of the
// scene is ever read, and the difference of a pixel without the neighbour, whatever it is, is never used.  Horizontally the
// column of the thread's first pixel is carried from chunk to chunk (one 64-bit remainder per thread at entry, then an add and a
// conditional subtract per staged pixel).
// No float atomics, no allocation, no host synchronisation, no BLAS; every order depends on (H, W, C, direction) only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_pca_tiles.h"

namespace dmf {

template <int DIR>
__global__ __launch_bounds__(256) void band_noise_kernel(const float* __restrict__ x, int64_t N, int W, int C, int64_t pitch, int Cm,
                                                         int64_t runs, int64_t runs_per_slice,
                                                         double* __restrict__ part /* [slices][pairs][64][64] */) {
  __shared__ float da[PCA_PX * PCA_LDS], db[PCA_PX * PCA_LDS];
  int I = 0, J = (int)blockIdx.x;                        // pair index -> (I, J), I <= J, row by row of the upper triangle
  while (J >= Cm - I) { J -= Cm - I; ++I; }
  J += I;
  const bool diag = I == J;
  const int w = threadIdx.x >> 6, l = threadIdx.x & 63, lk = l >> 4, li = l & 15;
  // column tiles t0 .. 3 of the wave's row strip are computed, as in band_cov_kernel
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

  // Thread (sp, sc) stages band sc of the pixels p0 + sp + 4 q of a chunk: four unconditional loads per pixel, the pixel and its
  // neighbour on either side of the macro tile, masked when they are stored.
  constexpr int NQ = PCA_PX * PCA_MT / 256;
  const int sp = threadIdx.x >> 6, sc = threadIdx.x & 63;
  const int ca = I * PCA_MT + sc, cb = J * PCA_MT + sc;
  const float* xa = x + (ca < C ? ca : C - 1);
  const float* xb = x + (cb < C ? cb : C - 1);
  const int64_t step = DIR == 0 ? 1 : W;
  const int64_t vend = N - W;                            // vertical: the pixels below vend have no pixel below them
  const uint32_t uw = (uint32_t)W, r4 = 4u % uw;
  uint32_t col = DIR == 0 ? (uint32_t)((pbeg + sp) % W) : 0u;   // horizontal: the column of the pixel p0 + sp of the chunk to be stored
  float va[NQ], vb[NQ], na[NQ], nb[NQ];
  auto issue = [&](int64_t p0) __attribute__((always_inline)) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int64_t n = p0 + sp + 4 * q < N ? p0 + sp + 4 * q : N - 1;
      const int64_t m = n + step < N ? n + step : N - 1;
      va[q] = xa[n * pitch];
      na[q] = xa[m * pitch];
      vb[q] = xb[n * pitch];
      nb[q] = xb[m * pitch];
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
      const int64_t p = p0 + sp + 4 * q;
      const bool has = DIR == 0 ? col != uw - 1u : p < vend;
      const bool in = p < pend && has;                   // zero past the slice's end, past C and where there is no neighbour
      da[(sp + 4 * q) * PCA_LDS + sc] = in && ca < C ? va[q] - na[q] : 0.f;
      db[(sp + 4 * q) * PCA_LDS + sc] = in && cb < C ? vb[q] - nb[q] : 0.f;
      if (DIR == 0) {                                    // the column four pixels on (after the 16th: of the next chunk's pixel)
        col += r4;
        if (col >= uw) col -= uw;
      }
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

// ncov[i][j] = ncov[j][i] = (the slices' partial sums, in ascending order) / (2 M); one thread per (i, j), i <= j
__global__ __launch_bounds__(256) void band_noise_finish_kernel(const double* __restrict__ part, int slices, int pairs, int Cm, int C,
                                                                int64_t M, double* __restrict__ ncov) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= C * C) return;
  const int i = idx / C, j = idx - i * C;
  if (i > j) return;
  const double* p = part + (int64_t)pca_pair_index(i >> 6, j >> 6, Cm) * (PCA_MT * PCA_MT) + (i & 63) * PCA_MT + (j & 63);
  double s = 0.;
  for (int q = 0; q < slices; ++q) s += p[(int64_t)q * pairs * (PCA_MT * PCA_MT)];
  const double v = s / (2.0 * (double)M);
  ncov[(int64_t)i * C + j] = v;
  ncov[(int64_t)j * C + i] = v;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

int64_t dmf_band_noise_workspace_bytes(int32_t H, int32_t W, int32_t C) {
  if (H < 1 || W < 1 || (int64_t)H * W < 2 || C < 1 || C > 512) return -1;
  const PcaPlan p = pca_plan((int64_t)H * W, C);
  return (int64_t)p.slices * p.pairs * (PCA_MT * PCA_MT) * (int64_t)sizeof(double);
}

// Return codes: dmf_band_moments's (include/dmf.h), and 7 for a direction outside 0..1.
int32_t dmf_band_noise_moments(const float* x, int32_t H, int32_t W, int32_t C, int64_t pitch, int32_t direction, double* ncov,
                               void* workspace, void* stream) {
  if (x == nullptr || ncov == nullptr || workspace == nullptr) return 1;
  if (direction < 0 || direction > 1) return 7;
  if (H < 1 || W < 1 || (direction == 0 ? W : H) < 2) return 2;          // M < 1: no pixel has the neighbour
  if (C < 1 || C > 512) return 3;
  if (pitch < C) return 5;
  if (reinterpret_cast<uintptr_t>(x) % 4 || reinterpret_cast<uintptr_t>(ncov) % 8 || reinterpret_cast<uintptr_t>(workspace) % 8) return 6;
  const int64_t N = (int64_t)H * W;
  if (!pca_extent_ok(N, pitch)) return 8;
  const int64_t M = direction == 0 ? (int64_t)H * (W - 1) : (int64_t)(H - 1) * W;
  const PcaPlan p = pca_plan(N, C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  double* part = static_cast<double*>(workspace);
  if (direction == 0)
    hipLaunchKernelGGL(band_noise_kernel<0>, dim3(p.pairs, p.slices), dim3(256), 0, st, x, N, W, C, pitch, p.Cm, p.runs, p.runs_per_slice,
                       part);
  else
    hipLaunchKernelGGL(band_noise_kernel<1>, dim3(p.pairs, p.slices), dim3(256), 0, st, x, N, W, C, pitch, p.Cm, p.runs, p.runs_per_slice,
                       part);
  if (hipGetLastError() != hipSuccess) return 9;
  hipLaunchKernelGGL(band_noise_finish_kernel, dim3((C * C + 255) / 256), dim3(256), 0, st, part, p.slices, p.pairs, p.Cm, C, M, ncov);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

}  // extern "C"
