// dmf_attr.hip — attribute profiles of the reduced bands: area openings and closings of the first P principal
// components at a ladder of n area thresholds, stacked as extra bands in front of the network (`band_profile: area`).
//   at_range_init_kernel / at_range_kernel   the exact min / max of every profiled component (dmf_attr_quantise)
//   at_quantise_kernel                       the uint8 planes q and L - 1 - q, and range [P][2]
//   at_local_kernel                          per (tile, plane): the tile-local union-find of {q >= t} for every level t of the batch
//   at_border_kernel                         per (plane, level): atomicMin links across tile borders
//   at_root_kernel                           per (plane, level): every pixel's root (paths shortened), the size of every root
//   at_count_kernel                          per plane: the pixel's owner adds the batch's qualifying levels to count
//   at_stack_kernel                          the profile [H][W][C] from count and range (dmf_attr_stack)
// The definition is in integers from the quantiser on (include/dmf.h states it): the opening of q at threshold a is, per pixel x,
// the number of levels t in 1..q(x) at which the 4-connected component of {q >= t} holding x has at least a pixels.  The sets are
// nested, so that number is also the largest such level.  The closing is the opening of L - 1 - q, read back as L - 1 - count.
//
// The min / max are integer atomicMin / atomicMax on the order-preserving unsigned image of the canonicalised float (sign bit
// flipped for x >= 0, all bits for x < 0): exact, whatever order the blocks arrive in.  The quantiser works in double with a
// subtract, a multiply and a divide in that order (nothing to contract), value() with a multiply, a divide and an add.
//
// One dmf_attr_area_levels call takes the levels first .. first + levels - 1 of all 2 P planes with four launches and reads
// nothing back.  Level l of plane s has its own parent and size planes in the workspace ([2 P][T][H W] int32 each), so the levels
// of a batch never meet.  The labelling is dmf_regions.hip's on the predicate "both pixels >= t": a 16 x 16 tile stages its q once
// and labels level after level in LDS (levels ascend and the sets are nested: a tile without a pixel >= t leaves the loop), the
// border launch links across tiles, the root launch finds every pixel's root and counts it, one atomicAdd per run of equal roots
// in a wave.  Only the cells of pixels with q >= t are ever written or read at level t: every parent value read was written by
// this call's at_local_kernel or by an atomicMin with a raster index, so it is a raster index of the image; a size cell is zeroed
// by at_local_kernel at every pixel >= t, and roots are such pixels.
// TERMINATION.  As dmf_region_prims.h argues: links go to the smaller index, a parent cell only ever decreases, and every value
// it held is a member of the same set.  `uf_find` walks strictly downwards through indices >= 0 and ends; `uf_unite` retries
// with what the cell held, which is smaller than the root it tried to link; at_root_kernel shortens a path by atomicMin with
// the root it found, which is again a decrease to a member of the same set, and no set is joined in that launch, so the root
// cells (parent == self) do not move under it.
// count [2 P][n][H W] uint8: the thread that owns pixel x is the only writer of its cells; calls on one stream are ordered; the
// call with first_level 1 stores, later calls add.  No atomics touch count.  No float atomics, no allocation, no host
// synchronisation.  Raster indices are int32 (H W < 2^31), offsets 64-bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_region_prims.h"

namespace dmf {

constexpr int AT_T = 16;                   // tile edge of the local labelling (dmf_regions.hip's): AT_T * AT_T threads
constexpr int AT_THREADS = AT_T * AT_T;
constexpr int AT_RANGE_PER = 4;            // pixels per thread of the range pass

struct AttrAreas { int32_t a[DMF_ATTR_NMAX]; };

__device__ __forceinline__ float attr_canon(float x) { return x + 0.0f; }       // -0 -> +0; everything else as it is

// the order-preserving unsigned image of a float: a < b as floats <=> key(a) < key(b) as unsigned (finite values, -0 canonicalised)
__device__ __forceinline__ unsigned attr_key(float v) {
  const unsigned b = __float_as_uint(v);
  return (b >> 31) ? ~b : b ^ 0x80000000u;
}
__device__ __forceinline__ float attr_unkey(unsigned k) { return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k); }

// ------------------------------------------------------------------------------ range and quantiser
__global__ __launch_bounds__(128) void at_range_init_kernel(int P, unsigned* __restrict__ keys /* [P][2]: min, max */) {
  const int t = (int)threadIdx.x;
  if (t < 2 * P) keys[t] = (t & 1) ? 0u : 0xffffffffu;
}

__global__ __launch_bounds__(256) void at_range_kernel(const float* __restrict__ scores, int64_t pixels, int64_t pitch, unsigned* keys) {
  __shared__ unsigned wmin[4], wmax[4];
  const int p = (int)blockIdx.z;
  unsigned lo = 0xffffffffu, hi = 0u;
#pragma unroll
  for (int e = 0; e < AT_RANGE_PER; ++e) {
    const int64_t x = ((int64_t)blockIdx.x * AT_RANGE_PER + e) * 256 + threadIdx.x;
    if (x < pixels) {
      const unsigned k = attr_key(attr_canon(scores[x * pitch + p]));
      lo = k < lo ? k : lo;
      hi = k > hi ? k : hi;
    }
  }
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned a = (unsigned)__shfl_xor((int)lo, d), b = (unsigned)__shfl_xor((int)hi, d);
    lo = a < lo ? a : lo;
    hi = b > hi ? b : hi;
  }
  const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
  if (lane == 0) { wmin[wave] = lo; wmax[wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) {
      lo = wmin[w] < lo ? wmin[w] : lo;
      hi = wmax[w] > hi ? wmax[w] : hi;
    }
    if (lo <= hi) {                                      // (a block past the image holds no pixel)
      atomicMin(keys + 2 * p, lo);
      atomicMax(keys + 2 * p + 1, hi);
    }
  }
}

// q = min(L - 1, floor(((f - lo) L) / (hi - lo))) in double: subtract, multiply, divide, in that order; 0 where hi == lo
__device__ __forceinline__ int attr_quantise_one(float f, float lo, float hi, int L) {
#pragma clang fp contract(off)
  if (!(hi > lo)) return 0;
  const double d = (double)f - (double)lo;
  const double m = d * (double)L;
  const double v = m / ((double)hi - (double)lo);
  const double fl = floor(v);
  int q = fl >= (double)(L - 1) ? L - 1 : (int)fl;     // (f is in lo..hi; anything else, a NaN included, lands in 0..L - 1 too)
  if (!(fl >= 0.0)) q = 0;
  return q;
}

// value(c) = (float)(lo + (c (hi - lo)) / L) in double: multiply, divide, add, in that order
__device__ __forceinline__ float attr_value(int c, float lo, float hi, int L) {
#pragma clang fp contract(off)
  const double span = (double)hi - (double)lo;
  const double m = (double)c * span;
  const double v = m / (double)L;
  return (float)((double)lo + v);
}

__global__ __launch_bounds__(256) void at_quantise_kernel(const float* __restrict__ scores, int64_t pixels, int64_t pitch, int P, int L,
                                                          const unsigned* __restrict__ keys, uint8_t* __restrict__ q /* [2 P][H W] */,
                                                          float* __restrict__ range /* [P][2] */) {
  const int p = (int)blockIdx.z;
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  const float lo = attr_unkey(keys[2 * p]), hi = attr_unkey(keys[2 * p + 1]);
  const int v = attr_quantise_one(attr_canon(scores[x * pitch + p]), lo, hi, L);
  q[(int64_t)p * pixels + x] = (uint8_t)v;
  q[(int64_t)(P + p) * pixels + x] = (uint8_t)(L - 1 - v);
  if (x == 0) { range[2 * p] = lo; range[2 * p + 1] = hi; }
}

// ------------------------------------------------------------------------------ the levels of a batch
// Block (tile, plane): the tile's q is staged once; level after level its union-find is built in LDS and written to the level's
// parent plane as raster indices (a pixel's local index grows with its raster index: the local root is the tile's smallest).
__global__ __launch_bounds__(AT_THREADS) void at_local_kernel(const uint8_t* __restrict__ q, int H, int W, int tiles_x, int first, int levels,
                                                              int T, int32_t* __restrict__ parent, int32_t* __restrict__ size) {
  __shared__ int up[AT_THREADS];
  __shared__ int lev[AT_THREADS];
  const int t = (int)threadIdx.x, ty = t / AT_T, tx = t % AT_T;
  const int tile_i = (int)(blockIdx.x / (unsigned)tiles_x);
  const int i0 = tile_i * AT_T, j0 = (int)(blockIdx.x - (unsigned)tile_i * (unsigned)tiles_x) * AT_T;
  const int i = i0 + ty, j = j0 + tx;
  const bool inside = i < H && j < W;
  const int64_t pixels = (int64_t)H * W, x = (int64_t)i * W + j;
  const int plane = (int)blockIdx.z;
  const int mine = inside ? (int)q[(int64_t)plane * pixels + x] : -1;         // outside the image: below every level
  lev[t] = mine;
  for (int l = 0; l < levels; ++l) {
    const int th = first + l;
    // (also the barrier between the level before, which read `up`, and this one; and the one that makes lev visible)
    if (!__syncthreads_or(mine >= th)) break;            // (uniform) no pixel >= th here, nor at any level above
    up[t] = t;
    __syncthreads();
    if (mine >= th) {                                    // (the pixel to the left of, or above, a pixel inside is inside)
      if (tx > 0 && lev[t - 1] >= th) uf_unite(up, t, t - 1);
      if (ty > 0 && lev[t - AT_T] >= th) uf_unite(up, t, t - AT_T);
    }
    __syncthreads();
    if (mine >= th) {
      const int r = uf_find(up, t);
      const int64_t cell = ((int64_t)plane * T + l) * pixels + x;
      parent[cell] = (int32_t)((int64_t)(i0 + r / AT_T) * W + j0 + r % AT_T);
      size[cell] = 0;
    }
  }
}

// blockIdx.z = plane * levels + l.  The pixel pairs across tile borders that are both >= t.
__global__ __launch_bounds__(256) void at_border_kernel(const uint8_t* __restrict__ q, int W, int64_t pixels, int first, int levels, int T,
                                                        int32_t* parent) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  const int i = (int)(x / W), j = (int)(x - (int64_t)i * W);
  const bool top = i > 0 && i % AT_T == 0, left = j > 0 && j % AT_T == 0;
  if (!top && !left) return;
  const int plane = (int)(blockIdx.z / (unsigned)levels), l = (int)blockIdx.z - plane * levels, th = first + l;
  const uint8_t* qp = q + (int64_t)plane * pixels;
  if ((int)qp[x] < th) return;
  int32_t* par = parent + ((int64_t)plane * T + l) * pixels;
  if (top && (int)qp[x - W] >= th) uf_unite(par, (int)x, (int)(x - W));
  if (left && (int)qp[x - 1] >= th) uf_unite(par, (int)x, (int)(x - 1));
}

// blockIdx.z = plane * levels + l.  No set is joined here: every pixel >= t finds its root, shortens its own path to it (a
// decrease, by atomicMin) and the root's size grows by the run's length, one atomicAdd per run of equal roots in a wave.
__global__ __launch_bounds__(256) void at_root_kernel(const uint8_t* __restrict__ q, int64_t pixels, int first, int levels, int T,
                                                      int32_t* parent, int32_t* size) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int plane = (int)(blockIdx.z / (unsigned)levels), l = (int)blockIdx.z - plane * levels, th = first + l;
  const int64_t base = ((int64_t)plane * T + l) * pixels;
  int32_t* par = parent + base;
  int key = -1;
  if (x < pixels && (int)q[(int64_t)plane * pixels + x] >= th) {
    key = uf_find(par, (int)x);
    if (uf_load(par, x) != key) atomicMin(par + x, key);
  }
  int last;                                              // (every lane of the wave is here: the run is formed by shuffles)
  const bool head = run_head(key, last);
  if (head && key >= 0) atomicAdd(size + base + key, last - (int)(threadIdx.x & 63) + 1);
}

// Block (256 pixels, plane).  The owner of pixel x walks the batch's levels 1 <= t <= q(x) and the n thresholds.
__global__ __launch_bounds__(256) void at_count_kernel(const uint8_t* __restrict__ q, int64_t pixels, int first, int levels, int T, int n,
                                                       AttrAreas areas, const int32_t* __restrict__ parent, const int32_t* __restrict__ size,
                                                       uint8_t* __restrict__ count /* [2 P][n][H W] */) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  const int plane = (int)blockIdx.z;
  const int qx = (int)q[(int64_t)plane * pixels + x];
  int add[DMF_ATTR_NMAX];
#pragma unroll
  for (int a = 0; a < DMF_ATTR_NMAX; ++a) add[a] = 0;
  for (int l = 0; l < levels && first + l <= qx; ++l) {
    const int64_t base = ((int64_t)plane * T + l) * pixels;
    const int s = size[base + uf_find(parent + base, (int)x)];
#pragma unroll
    for (int a = 0; a < DMF_ATTR_NMAX; ++a) add[a] += (a < n && s >= areas.a[a]) ? 1 : 0;
  }
#pragma unroll
  for (int a = 0; a < DMF_ATTR_NMAX; ++a)
    if (a < n) {
      uint8_t* cell = count + ((int64_t)plane * n + a) * pixels + x;
      *cell = (uint8_t)((first == 1 ? 0 : (int)*cell) + add[a]);       // (at most L - 1 <= 255 levels in all)
    }
}

// ------------------------------------------------------------------------------ stack
// out[pixel][c], c fastest: per profiled component the closings from the largest area down, the component, the openings from the
// smallest up; then the components P .. K - 1 as the scores hold them.
__global__ __launch_bounds__(256) void at_stack_kernel(const float* __restrict__ scores, int64_t pixels, int K, int64_t pitch, int P, int n, int L,
                                                       const uint8_t* __restrict__ count, const float* __restrict__ range,
                                                       float* __restrict__ out) {
  const int C = K + 2 * n * P, G = 2 * n + 1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= pixels * C) return;
  const int64_t px = idx / C;
  const int c = (int)(idx - px * C);
  float v;
  if (c < P * G) {
    const int p = c / G, b = c - p * G;
    if (b == n) {
      v = attr_canon(scores[px * pitch + p]);
    } else {
      const int level = b < n ? L - 1 - (int)count[((int64_t)(P + p) * n + (n - 1 - b)) * pixels + px]
                              : (int)count[((int64_t)p * n + (b - n - 1)) * pixels + px];
      v = attr_value(level, range[2 * p], range[2 * p + 1], L);
    }
  } else {
    v = scores[px * pitch + P + (c - P * G)];
  }
  out[idx] = v;
}

// ------------------------------------------------------------------------------ host
struct AttrSpace {                                       // the workspace, every part 16-byte aligned
  int64_t keys, parent, size, bytes;
};

static AttrSpace attr_space(int64_t pixels, int P, int T) {
  AttrSpace s;
  const int64_t planes = up16((int64_t)2 * P * T * pixels * (int64_t)sizeof(int32_t));
  s.keys = 0;
  s.parent = up16((int64_t)2 * P * (int64_t)sizeof(uint32_t));
  s.size = s.parent + planes;
  s.bytes = s.size + planes;
  return s;
}

static inline bool attr_extent_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && (int64_t)H * W < DMF_ATTR_PIXELS_MAX; }

static inline bool attr_areas_ok(const int32_t* areas, int32_t n) {
  if (n < 1 || n > DMF_ATTR_NMAX) return false;
  for (int i = 0; i < n; ++i)
    if (areas[i] < 1 || (i > 0 && areas[i] <= areas[i - 1])) return false;
  return true;
}

static inline bool attr_aligned(const void* p, int to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

}  // namespace dmf

using namespace dmf;

extern "C" {

// Return codes (include/dmf.h lists them): this file has no access to the text buffer of dmf_last_error.
int64_t dmf_attr_workspace_bytes(int32_t H, int32_t W, int32_t P, int32_t n, int32_t T) {
  if (!attr_extent_ok(H, W) || P < 1 || P > 64 || n < 1 || n > DMF_ATTR_NMAX || T < 1 || T > DMF_ATTR_BATCH_MAX) return -1;
  return attr_space((int64_t)H * W, P, T).bytes;
}

int32_t dmf_attr_quantise(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P, int32_t L, uint8_t* q, float* range,
                          void* workspace, int64_t workspace_bytes, void* stream) {
  if (scores == nullptr || q == nullptr || range == nullptr || workspace == nullptr) return 1;
  if (!attr_extent_ok(H, W)) return 2;
  if (K < 1 || K > 64 || P < 1 || P > K) return 3;
  if (pitch < K) return 5;
  if (L < 2 || L > DMF_ATTR_LEVELS_MAX) return 11;
  const int64_t pixels = (int64_t)H * W;
  if (pixels > INT64_MAX / 4 / pitch) return 8;
  const AttrSpace sp = attr_space(pixels, P, 1);
  if (workspace_bytes < sp.parent) return 12;
  if (!attr_aligned(scores, 4) || !attr_aligned(range, 4) || !attr_aligned(workspace, 16)) return 6;
  const void* outs[3] = {q, range, workspace};
  const uint64_t out_bytes[3] = {(uint64_t)2 * P * pixels, (uint64_t)2 * P * sizeof(float), (uint64_t)sp.parent};
  const void* ins[1] = {scores};
  const uint64_t in_bytes[1] = {(uint64_t)(((pixels - 1) * pitch + K) * (int64_t)sizeof(float))};
  if (any_overlap(outs, out_bytes, 3, ins, in_bytes, 1)) return 7;
  hipStream_t st = static_cast<hipStream_t>(stream);
  unsigned* keys = static_cast<unsigned*>(workspace);
  DMF_LAUNCH(at_range_init_kernel, 1, 128, P, keys);
  DMF_LAUNCH(at_range_kernel, dim3(blocks_of(pixels, 256 * AT_RANGE_PER), 1, P), 256, scores, pixels, pitch, keys);
  DMF_LAUNCH(at_quantise_kernel, dim3(blocks_of(pixels, 256), 1, P), 256, scores, pixels, pitch, P, L, keys, q, range);
  return 0;
}

int32_t dmf_attr_area_levels(const uint8_t* q, int32_t H, int32_t W, int32_t P, const int32_t* areas, int32_t n, int32_t L, int32_t first_level,
                             int32_t levels, int32_t T, uint8_t* count, void* workspace, int64_t workspace_bytes, void* stream) {
  if (q == nullptr || areas == nullptr || count == nullptr || workspace == nullptr) return 1;
  if (!attr_extent_ok(H, W)) return 2;
  if (P < 1 || P > 64) return 3;
  if (!attr_areas_ok(areas, n)) return 4;
  if (L < 2 || L > DMF_ATTR_LEVELS_MAX) return 11;
  if (T < 1 || T > DMF_ATTR_BATCH_MAX || levels < 1 || levels > T || first_level < 1 || first_level + levels - 1 > L - 1) return 10;
  const int64_t pixels = (int64_t)H * W;
  const AttrSpace sp = attr_space(pixels, P, T);
  if (workspace_bytes < sp.bytes) return 12;
  if (!attr_aligned(workspace, 16)) return 6;
  const void* outs[2] = {count, workspace};
  const uint64_t out_bytes[2] = {(uint64_t)2 * P * n * pixels, (uint64_t)sp.bytes};
  const void* ins[1] = {q};
  const uint64_t in_bytes[1] = {(uint64_t)2 * P * pixels};
  if (any_overlap(outs, out_bytes, 2, ins, in_bytes, 1)) return 7;
  const int64_t tx = ((int64_t)W + AT_T - 1) / AT_T, ty = ((int64_t)H + AT_T - 1) / AT_T;
  if (tx * ty > INT32_MAX) return 8;
  AttrAreas aa = {};
  for (int i = 0; i < n; ++i) aa.a[i] = areas[i];
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* parent = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + sp.parent);
  int32_t* size = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + sp.size);
  const unsigned per = blocks_of(pixels, 256);
  DMF_LAUNCH(at_local_kernel, dim3((unsigned)(tx * ty), 1, 2 * P), AT_THREADS, q, H, W, (int)tx, first_level, levels, T, parent, size);
  DMF_LAUNCH(at_border_kernel, dim3(per, 1, 2 * P * levels), 256, q, W, pixels, first_level, levels, T, parent);
  DMF_LAUNCH(at_root_kernel, dim3(per, 1, 2 * P * levels), 256, q, pixels, first_level, levels, T, parent, size);
  DMF_LAUNCH(at_count_kernel, dim3(per, 1, 2 * P), 256, q, pixels, first_level, levels, T, n, aa, parent, size, count);
  return 0;
}

int32_t dmf_attr_stack(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P, int32_t n, int32_t L, const uint8_t* count,
                       const float* range, float* out, void* stream) {
  if (scores == nullptr || count == nullptr || range == nullptr || out == nullptr) return 1;
  if (!attr_extent_ok(H, W)) return 2;
  if (K < 1 || K > 64 || P < 1 || P > K) return 3;
  if (n < 1 || n > DMF_ATTR_NMAX) return 4;
  if (pitch < K) return 5;
  if (L < 2 || L > DMF_ATTR_LEVELS_MAX) return 11;
  if (!attr_aligned(scores, 4) || !attr_aligned(range, 4) || !attr_aligned(out, 4)) return 6;
  const int64_t pixels = (int64_t)H * W, total = pixels * (K + 2 * n * P), blocks = (total + 255) / 256;
  if (blocks > INT32_MAX || pixels > INT64_MAX / 4 / pitch) return 8;
  const void* outs[1] = {out};
  const uint64_t out_bytes[1] = {(uint64_t)total * sizeof(float)};
  const void* ins[3] = {scores, count, range};
  const uint64_t in_bytes[3] = {(uint64_t)(((pixels - 1) * pitch + K) * (int64_t)sizeof(float)), (uint64_t)2 * P * n * pixels,
                                (uint64_t)2 * P * sizeof(float)};
  if (any_overlap(outs, out_bytes, 1, ins, in_bytes, 3)) return 7;
  hipStream_t st = static_cast<hipStream_t>(stream);
  DMF_LAUNCH(at_stack_kernel, (unsigned)blocks, 256, scores, pixels, K, pitch, P, n, L, count, range, out);
  return 0;
}

}  // extern "C"
