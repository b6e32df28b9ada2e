// dmf_pca_tiles.h — what the two band-pair product kernels share: band_cov_kernel (dmf_pca.hip) and
// band_noise_kernel (dmf_noise.hip).  The tile constants, how the pixels and the band pairs are cut (on the host:
// grid and workspace), the index of a macro-tile pair and the products of one staged chunk.  Stated once, so that both kernels
// have the same runs, the same slices and the same fmaf chains.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dmf.h"

namespace dmf {

typedef float pca_f32x4 __attribute__((ext_vector_type(4)));

constexpr int PCA_R = DMF_PCA_RUN;       // pixels one fp32 accumulator covers
constexpr int PCA_MT = 64;               // bands of a macro tile's side
constexpr int PCA_PX = 64;               // pixels per LDS chunk of the covariance
constexpr int PCA_LDS = 80;              // floats from one staged pixel (covariance) or basis row (projection) to the next
constexpr int PCA_MAX_BLOCKS = 768;      // macro tile pairs x slices of the covariance, at most: one round of 3 workgroups per CU
constexpr int PCA_MEAN_SLICES = 1024;    // slices of the mean, at most
static_assert(PCA_R >= 256 && PCA_R <= 1024 && PCA_R % PCA_PX == 0, "DMF_PCA_RUN");

// How (N, C) is cut: the same on the host (grid, workspace) and nowhere else.
struct PcaPlan {
  int Cm, pairs;                         // macro tiles per side, upper-triangular pairs of them
  int64_t runs, runs_per_slice;          // covariance: runs of R pixels, runs a slice owns
  int slices;
  int64_t px_per_slice;                  // mean: pixels a slice owns
  int mslices;
};

static PcaPlan pca_plan(int64_t N, int C) {
  PcaPlan p;
  p.Cm = (C + PCA_MT - 1) / PCA_MT;
  p.pairs = p.Cm * (p.Cm + 1) / 2;
  p.runs = (N + PCA_R - 1) / PCA_R;
  const int64_t cap = PCA_MAX_BLOCKS / p.pairs;                          // >= 21 at C = 512
  p.runs_per_slice = (p.runs + cap - 1) / cap;
  p.slices = (int)((p.runs + p.runs_per_slice - 1) / p.runs_per_slice);
  const int64_t mcap = p.runs < PCA_MEAN_SLICES ? p.runs : PCA_MEAN_SLICES;
  p.px_per_slice = (N + mcap - 1) / mcap;
  p.mslices = (int)((N + p.px_per_slice - 1) / p.px_per_slice);
  return p;
}

__device__ __forceinline__ int pca_pair_index(int I, int J, int Cm) { return I * Cm - I * (I - 1) / 2 + (J - I); }

// The products of one staged chunk for the column tiles T0 .. 3: pa / pb point at the lane's element of pixel 0.
template <int T0>
__device__ __forceinline__ void cov_steps(const float* pa, const float* pb, pca_f32x4 (&acc)[4]) {
#pragma unroll
  for (int kk = 0; kk < PCA_PX / 4; ++kk) {
    const float a = pa[4 * kk * PCA_LDS];
    float b[4];
#pragma unroll
    for (int t = T0; t < 4; ++t) b[t] = pb[4 * kk * PCA_LDS + 16 * t];
#pragma unroll
    for (int t = T0; t < 4; ++t) acc[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b[t], acc[t], 0, 0, 0);
  }
}

// N pixels of `pitch` floats each are addressable with 64-bit byte offsets
static bool pca_extent_ok(int64_t N, int64_t pitch) { return N <= INT64_MAX / 8 / pitch; }

}  // namespace dmf
