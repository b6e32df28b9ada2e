// dmf_spatial.hip — spatial regularisation of class maps by a scene-guided bilateral filter: the class
// probabilities of a pixel are averaged over its (2r + 1)^2 window, every neighbour weighted by how close it is and how
// similar the scene is there (edge-preserving filtering, Kang et al. 2014; one mean-field step of a pairwise CRF).
//   prob_scatter_kernel       softmax of every row of logits [B, K], scattered into a pixel-major map prob [H, W, K] with mask
//   spatial_affinity_kernel   aff [H W][n] from the resident primary scene, once per scene
//   spatial_filter_kernel     one iteration: out = (sum_k aff mask p) / (sum_k aff mask), with the argmax written to a label map
// The entry points dmf_prob_scatter, dmf_spatial_affinity and dmf_spatial_filter live here too (host code at the end of the
// file) and report by return code, as dmf_augment.hip's do.  Plain HIP C++; no float atomics, every sum in a fixed order: the
// same bits on every run.
//
// Tiles.  The affinity and the filter give a workgroup of 256 threads a 16 x 16 tile of pixels, one pixel per thread, with its
// halo of r pixels: TW x TW pixels, TW = 16 + 2 r <= 22.  What a pixel needs of its n = (2r + 1)^2 neighbours is read from
// LDS at compile-time offsets from the thread's own cell (r is a template parameter), and the n partial sums (affinity) or the
// n weights (filter) of a pixel live in registers.
//   * affinity: the halo tile at 224 bands is 433 KB, so the bands go through LDS in chunks of AFF_CB = 16, widened to fp32: a
//     pixel is AFF_S = 20 floats apart from the next (16-byte aligned float4 reads; 16 consecutive pixels at stride 20 dwords
//     fall on 16 different 4-bank slots of the 64 banks).  With the output staging below that is 26 / 32 / 50 KB of LDS per
//     workgroup at r = 1 / 2 / 3, six to three workgroups on a CU's 160 KB (at r = 3 the 164 registers allow three too).  A chunk past C is zero-filled and adds +0 to every sum.  Every
//     chunk reads bands the others do not: the scene is read once, apart from the halo overlap.
//   * filter: the classes go through LDS in chunks of KC = 16 (K <= 4: 4) at an odd stride of KC + 1 floats per pixel
//     (4-byte reads of 64 different pixels: no bank conflict); 22 x 22 x 17 floats is 33 KB.  A neighbour that is outside the
//     scene or has mask 0 is staged as zeros, so nothing that an unmasked cell of prob_in may hold reaches a sum.
//   * both write through LDS: a thread leaves its n (or KC) results at an odd stride, and the workgroup then stores the tile
//     row by row, consecutive lanes to consecutive addresses; the filter reads its aff rows the same way, contiguous n-float
//     rows of 16 pixels at a time.  The scene's base needs element alignment only: it is read element by element.
// All global offsets are 64-bit: 50 M pixels x 49 floats is 9.8 GB.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_rows.h"

namespace dmf {

// ------------------------------------------------------------------------------ probability scatter
// softmax_stats_kernel's rows and softmax terms (dmf_rows.h): p[pred] = 1 / Z is its conf.
template <int L>
__global__ __launch_bounds__(256) void prob_scatter_kernel(const float* __restrict__ logits, int B, int K,
                                                           const float* __restrict__ inv_temp, const int32_t* __restrict__ xy, int W,
                                                           float* __restrict__ prob, uint8_t* __restrict__ mask) {
  const int c = row_column<L>();
  const int64_t r = row_index<L>();
  const bool row = r < B;
  const float beta = inv_temp != nullptr ? inv_temp[0] : 1.f;
  const RowSoftmax s = row_softmax<L>(row && c < K ? logits[(size_t)r * K + c] : -INFINITY, c, beta);
  const float Z = row_sum<L>(s.e);
  if (!row || c >= K) return;
  const int64_t o = (int64_t)xy[2 * r] * W + xy[2 * r + 1];
  prob[o * K + c] = s.e / Z;
  if (c == 0) mask[o] = 1;
}

// ------------------------------------------------------------------------------ tiles
constexpr int SP_T = 16;                 // tile edge in pixels; SP_T * SP_T threads
constexpr int SP_THREADS = SP_T * SP_T;
constexpr int AFF_CB = 16;               // bands per LDS chunk of the affinity
constexpr int AFF_S = AFF_CB + 4;        // floats from one pixel of the chunk to the next

__host__ __device__ constexpr int sp_tw(int r) { return SP_T + 2 * r; }
__host__ __device__ constexpr int sp_n(int r) { return (2 * r + 1) * (2 * r + 1); }
__host__ __device__ constexpr int sp_max(int a, int b) { return a > b ? a : b; }
// floats of LDS: the staged chunk, later the workgroup's results
__host__ __device__ constexpr int aff_lds_floats(int r) { return sp_max(sp_tw(r) * sp_tw(r) * AFF_S, SP_THREADS * sp_n(r)); }
// the filter: prob tile [TW TW][KC + 1], results [256][KC + 1], mask tile [TW TW] — or, before them, the aff rows [256][n]
__host__ __device__ constexpr int filt_lds_floats(int r, int kc) {
  return sp_max(sp_tw(r) * sp_tw(r) * (kc + 1) + SP_THREADS * (kc + 1) + sp_tw(r) * sp_tw(r), SP_THREADS * sp_n(r));
}

__device__ __forceinline__ float sp_widen(float v) { return v; }
__device__ __forceinline__ float sp_widen(__half v) { return __half2float(v); }

// Store the workgroup's res [256][n] (thread-major in LDS) as the rows of its tile: pixel (i0 + ty, j0 + tx) owns the n floats
// at ((i W + j) n); consecutive idx are consecutive addresses along a tile row.
template <int N>
__device__ __forceinline__ void sp_store_rows(const float* res, float* __restrict__ out, int i0, int j0, int H, int W) {
  for (int idx = threadIdx.x; idx < SP_THREADS * N; idx += SP_THREADS) {
    const int p = idx / N, k = idx - p * N;
    const int i = i0 + p / SP_T, j = j0 + p % SP_T;
    if (i < H && j < W) out[((int64_t)i * W + j) * N + k] = res[idx];
  }
}

// ------------------------------------------------------------------------------ affinity
template <int R, typename T>
__global__ __launch_bounds__(SP_THREADS) void spatial_affinity_kernel(const T* __restrict__ scene, int pitch, int H, int W, int C,
                                                                      float cs, float cr, int tiles_x, float* __restrict__ aff) {
  constexpr int TW = sp_tw(R), N = sp_n(R), D = 2 * R + 1;
  extern __shared__ __attribute__((aligned(16))) float sp_lds[];
  const int tile_i = (int)(blockIdx.x / (unsigned)tiles_x);
  const int i0 = tile_i * SP_T, j0 = (int)(blockIdx.x - (unsigned)tile_i * (unsigned)tiles_x) * SP_T;
  const int ty = threadIdx.x / SP_T, tx = threadIdx.x % SP_T;
  const float* own = sp_lds + ((ty + R) * TW + tx + R) * AFF_S;
  float acc[N];
#pragma unroll
  for (int k = 0; k < N; ++k) acc[k] = 0.f;

  for (int c0 = 0; c0 < C; c0 += AFF_CB) {
    __syncthreads();                                     // the previous chunk has been read
    for (int idx = threadIdx.x; idx < TW * TW * AFF_CB; idx += SP_THREADS) {
      const int p = idx / AFF_CB, c = idx - p * AFF_CB;
      const int i = i0 - R + p / TW, j = j0 - R + p % TW;
      float v = 0.f;
      if (i >= 0 && i < H && j >= 0 && j < W && c0 + c < C) v = sp_widen(scene[((int64_t)i * pitch + j) * C + c0 + c]);
      sp_lds[p * AFF_S + c] = v;
    }
    __syncthreads();
    float4 a[AFF_CB / 4];
#pragma unroll
    for (int q = 0; q < AFF_CB / 4; ++q) a[q] = reinterpret_cast<const float4*>(own)[q];
#pragma unroll
    for (int k = 0; k < N; ++k) {
      const float4* nb = reinterpret_cast<const float4*>(own + ((k / D - R) * TW + (k % D - R)) * AFF_S);
      float s = acc[k];
#pragma unroll
      for (int q = 0; q < AFF_CB / 4; ++q) {
        const float4 b = nb[q];
        const float d0 = a[q].x - b.x, d1 = a[q].y - b.y, d2 = a[q].z - b.z, d3 = a[q].w - b.w;
        s = fmaf(d0, d0, s); s = fmaf(d1, d1, s); s = fmaf(d2, d2, s); s = fmaf(d3, d3, s);
      }
      acc[k] = s;
    }
  }
  __syncthreads();                                       // the last chunk has been read: LDS now takes the results
  const int i = i0 + ty, j = j0 + tx;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    const int di = k / D - R, dj = k % D - R;
    float v = 0.f;
    if (i + di >= 0 && i + di < H && j + dj >= 0 && j + dj < W) {
      const float d2 = acc[k] / (float)C;
      v = (di == 0 && dj == 0) ? 1.f : expf(-__fadd_rn(__fmul_rn((float)(di * di + dj * dj), cs), __fmul_rn(d2, cr)));
    }
    sp_lds[threadIdx.x * N + k] = v;
  }
  __syncthreads();
  sp_store_rows<N>(sp_lds, aff, i0, j0, H, W);
}

template <int R, typename T>
static hipError_t affinity_launch(const void* scene, int pitch, int H, int W, int C, float cs, float cr, int tiles_x, unsigned blocks,
                                  float* aff, hipStream_t st) {
  hipLaunchKernelGGL((spatial_affinity_kernel<R, T>), dim3(blocks), dim3(SP_THREADS), (size_t)aff_lds_floats(R) * sizeof(float), st,
                     static_cast<const T*>(scene), pitch, H, W, C, cs, cr, tiles_x, aff);
  return hipGetLastError();
}

template <typename T>
static hipError_t affinity_radius(int r, const void* scene, int pitch, int H, int W, int C, float cs, float cr, int tiles_x,
                                  unsigned blocks, float* aff, hipStream_t st) {
  if (r == 1) return affinity_launch<1, T>(scene, pitch, H, W, C, cs, cr, tiles_x, blocks, aff, st);
  if (r == 2) return affinity_launch<2, T>(scene, pitch, H, W, C, cs, cr, tiles_x, blocks, aff, st);
  return affinity_launch<3, T>(scene, pitch, H, W, C, cs, cr, tiles_x, blocks, aff, st);
}

// ------------------------------------------------------------------------------ filter
template <int R, int KC>
__global__ __launch_bounds__(SP_THREADS) void spatial_filter_kernel(const float* __restrict__ prob_in, const uint8_t* __restrict__ mask,
                                                                    const float* __restrict__ aff, int H, int W, int K, int tiles_x,
                                                                    float* __restrict__ prob_out, int32_t* __restrict__ label_map) {
  constexpr int TW = sp_tw(R), N = sp_n(R), D = 2 * R + 1, S = KC + 1;
  extern __shared__ __attribute__((aligned(16))) float sp_lds[];
  float* ptile = sp_lds;                                 // [TW TW][S]
  float* res = ptile + TW * TW * S;                      // [256][S]
  float* mtile = res + SP_THREADS * S;                   // [TW TW]: 1 for a neighbour inside the scene with mask 1
  const int tile_i = (int)(blockIdx.x / (unsigned)tiles_x);
  const int i0 = tile_i * SP_T, j0 = (int)(blockIdx.x - (unsigned)tile_i * (unsigned)tiles_x) * SP_T;
  const int ty = threadIdx.x / SP_T, tx = threadIdx.x % SP_T;
  const int i = i0 + ty, j = j0 + tx;
  const bool inside = i < H && j < W;

  // the aff rows of the tile, 16 pixels x n contiguous floats at a time, into [256][n]; then each thread's own row to registers
  for (int idx = threadIdx.x; idx < SP_THREADS * N; idx += SP_THREADS) {
    const int p = idx / N, k = idx - p * N;
    const int pi = i0 + p / SP_T, pj = j0 + p % SP_T;
    sp_lds[idx] = pi < H && pj < W ? aff[((int64_t)pi * W + pj) * N + k] : 0.f;
  }
  __syncthreads();
  float w[N];
#pragma unroll
  for (int k = 0; k < N; ++k) w[k] = sp_lds[threadIdx.x * N + k];
  __syncthreads();                                       // the aff rows are in registers: LDS now takes the tiles
  for (int p = threadIdx.x; p < TW * TW; p += SP_THREADS) {
    const int pi = i0 - R + p / TW, pj = j0 - R + p % TW;
    mtile[p] = pi >= 0 && pi < H && pj >= 0 && pj < W && mask[(int64_t)pi * W + pj] != 0 ? 1.f : 0.f;
  }
  __syncthreads();
  const int cell = (ty + R) * TW + tx + R;
  const bool live = inside && mtile[cell] != 0.f;
  float den = 0.f;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    w[k] *= mtile[cell + (k / D - R) * TW + (k % D - R)];      // aff * mask(y): exact, the mask is 0 or 1
    den += w[k];
  }
  float best = -INFINITY;
  int best_c = 0;

  for (int c0 = 0; c0 < K; c0 += KC) {
    const int kc = K - c0 < KC ? K - c0 : KC;            // classes of this chunk
    if (c0 > 0) __syncthreads();                         // the previous chunk's results have been stored
    for (int idx = threadIdx.x; idx < TW * TW * KC; idx += SP_THREADS) {
      const int p = idx / KC, c = idx - p * KC;
      float v = 0.f;
      if (c < kc && mtile[p] != 0.f) {
        const int pi = i0 - R + p / TW, pj = j0 - R + p % TW;
        v = prob_in[((int64_t)pi * W + pj) * K + c0 + c];
      }
      ptile[p * S + c] = v;
    }
    __syncthreads();
    const float* centre = ptile + cell * S;
    for (int c = 0; c < kc; ++c) {
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < N; ++k) s = fmaf(w[k], centre[((k / D - R) * TW + (k % D - R)) * S + c], s);
      const float o = live ? s / den : 0.f;
      if (o > best) { best = o; best_c = c0 + c; }       // strict: the first maximal index
      res[threadIdx.x * S + c] = o;
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < SP_THREADS * kc; idx += SP_THREADS) {
      const int p = idx / kc, c = idx - p * kc;
      const int pi = i0 + p / SP_T, pj = j0 + p % SP_T;
      if (pi < H && pj < W) prob_out[((int64_t)pi * W + pj) * K + c0 + c] = res[p * S + c];
    }
  }
  if (live) label_map[(int64_t)i * W + j] = best_c;
}

template <int R, int KC>
static hipError_t filter_launch(const float* prob_in, const uint8_t* mask, const float* aff, int H, int W, int K, int tiles_x,
                                unsigned blocks, float* prob_out, int32_t* label_map, hipStream_t st) {
  hipLaunchKernelGGL((spatial_filter_kernel<R, KC>), dim3(blocks), dim3(SP_THREADS), (size_t)filt_lds_floats(R, KC) * sizeof(float), st,
                     prob_in, mask, aff, H, W, K, tiles_x, prob_out, label_map);
  return hipGetLastError();
}

template <int KC>
static hipError_t filter_radius(int r, const float* prob_in, const uint8_t* mask, const float* aff, int H, int W, int K, int tiles_x,
                                unsigned blocks, float* prob_out, int32_t* label_map, hipStream_t st) {
  if (r == 1) return filter_launch<1, KC>(prob_in, mask, aff, H, W, K, tiles_x, blocks, prob_out, label_map, st);
  if (r == 2) return filter_launch<2, KC>(prob_in, mask, aff, H, W, K, tiles_x, blocks, prob_out, label_map, st);
  return filter_launch<3, KC>(prob_in, mask, aff, H, W, K, tiles_x, blocks, prob_out, label_map, st);
}

// the largest tile of either kernel stays below the 64 KB a launch may ask for without an attribute
static_assert(aff_lds_floats(3) * sizeof(float) <= 65536 && filt_lds_floats(3, 16) * sizeof(float) <= 65536, "LDS per workgroup");

// tiles of a scene -> (tiles_x, workgroups); false where a grid does not hold them
static bool sp_grid(int H, int W, int& tiles_x, unsigned& blocks) {
  const int64_t tx = ((int64_t)W + SP_T - 1) / SP_T, ty = ((int64_t)H + SP_T - 1) / SP_T;
  if (tx * ty > INT32_MAX) return false;
  tiles_x = (int)tx;
  blocks = (unsigned)(tx * ty);
  return true;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

// Return codes (include/dmf.h lists them): this file has no access to the text buffer of dmf_last_error.
int32_t dmf_prob_scatter(const float* logits, int32_t B, int32_t K, const float* inv_temp, const int32_t* xy, int32_t W, float* prob,
                         uint8_t* mask, void* stream) {
  if (logits == nullptr || xy == nullptr || prob == nullptr || mask == nullptr) return 1;
  if (B < 0 || W < 1) return 2;
  if (K < 1 || K > DMF_KMAX) return 3;
  if (B == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = for_row_lanes(K, [&](auto L) {
    hipLaunchKernelGGL(prob_scatter_kernel<decltype(L)::value>, row_blocks<decltype(L)::value>(B), dim3(256), 0, st, logits, B, K,
                       inv_temp, xy, W, prob, mask);
    return hipGetLastError();
  });
  return e == hipSuccess ? 0 : 9;
}

int32_t dmf_spatial_affinity(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C, int32_t r,
                             float cs, float cr, float* aff, void* stream) {
  if (scene == nullptr || aff == nullptr) return 1;
  if (H < 1 || W < 1 || C < 1) return 2;
  if (r < 1 || r > 3) return 4;
  if (elem_bytes != 2 && elem_bytes != 4) return 5;
  if (pitch_pixels < W) return 6;
  int tiles_x;
  unsigned blocks;
  if (reinterpret_cast<uintptr_t>(scene) % elem_bytes || !sp_grid(H, W, tiles_x, blocks)) return 8;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = elem_bytes == 2 ? affinity_radius<__half>(r, scene, pitch_pixels, H, W, C, cs, cr, tiles_x, blocks, aff, st)
                                       : affinity_radius<float>(r, scene, pitch_pixels, H, W, C, cs, cr, tiles_x, blocks, aff, st);
  return e == hipSuccess ? 0 : 9;
}

int32_t dmf_spatial_filter(const float* prob_in, const uint8_t* mask, const float* aff, int32_t H, int32_t W, int32_t K, int32_t r,
                           float* prob_out, int32_t* label_map, void* stream) {
  if (prob_in == nullptr || mask == nullptr || aff == nullptr || prob_out == nullptr || label_map == nullptr) return 1;
  if (H < 1 || W < 1) return 2;
  if (K < 1 || K > DMF_KMAX) return 3;
  if (r < 1 || r > 3) return 4;
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(prob_in), b0 = reinterpret_cast<uintptr_t>(prob_out);
  const uintptr_t bytes = (uintptr_t)H * (uintptr_t)W * (uintptr_t)K * sizeof(float);
  if (a0 < b0 + bytes && b0 < a0 + bytes) return 7;
  int tiles_x;
  unsigned blocks;
  if (!sp_grid(H, W, tiles_x, blocks)) return 8;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = K <= 4 ? filter_radius<4>(r, prob_in, mask, aff, H, W, K, tiles_x, blocks, prob_out, label_map, st)
                              : filter_radius<16>(r, prob_in, mask, aff, H, W, K, tiles_x, blocks, prob_out, label_map, st);
  return e == hipSuccess ? 0 : 9;
}

}  // extern "C"
