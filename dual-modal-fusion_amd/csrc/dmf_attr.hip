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
//
// SEVERAL ATTRIBUTES (dmf_attr_multi_levels).  The same components, measured three ways: pixel count, bounding box,
// sum and sum of squares of q.  The thresholds are areas ++ diagonals ++ stds and count keeps its shape, so the quantiser and the
// stack serve unchanged.  at_local_kernel and at_border_kernel are shared as they are; three kernels are new:
//   at_multi_init_kernel<BOX, STD>    per (plane, level): the identities of the accumulators, at the root cells alone
//   at_multi_root_kernel<BOX, STD>    at_root_kernel, and per run of equal roots in a wave one atomic per accumulator
//   at_multi_count_kernel<BOX, STD>   at_count_kernel with the n criteria of dmf_attr_criteria.h at the root's cell
// BOX / STD say which plane sets exist: one that was not asked for is neither allocated nor touched.
// INITIALISATION.  at_multi_init_kernel runs after the border launch and before the root launch.  By then the forest is final (the
// root launch joins no sets), so the roots are exactly the pixels >= t with parent == self, and the kernel stores INT32_MAX / -1
// (min / max of column and row) and 0 (the sums) there and nowhere else.  The root launch's atomics go to the cell of a root
// that some pixel >= t found, and the count launch reads the cell of such a root: both touch initialised cells only, whatever the
// workspace held before.  size is zeroed by at_local_kernel, as above.  So the workspace still needs no clearing.
// THE RUN OF A WAVE is a stretch of consecutive raster indices x0 .. x1, so its box is known from its two ends: rows row(x0) ..
// row(x1); columns col(x0) .. col(x1) when both ends lie in one row, and 0 .. W - 1 otherwise (the run then holds the last pixel
// of one row and the first of the next).  Rows shorter than a wave are thereby covered, and the box costs no shuffle.  The two
// sums are reduced over the run with run_sum's segmented shuffles, packed into one 64-bit word (sum q <= 64 255 in the low half,
// sum q^2 <= 64 255^2 in the high half: no carry crosses).  The head issues atomicAdd int32 (size), atomicMin / atomicMax int32
// (box), atomicAdd uint64 (sums): one 64-bit atomic per sum and run, not partial sums staged per tile — the roots of a tile's
// pixels are not known to be few, so a tile has no table to stage into, and an atomic that returns nothing costs its issuer a
// few cycles; after the wave's reduction there are as many of them as there are size atomics.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_attr_criteria.h"
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

// ------------------------------------------------------------------------------ several attributes
struct AttrThresholds { int32_t t[DMF_ATTR_NMAX]; };     // areas ++ diagonals ++ stds

struct AttrPlanes {                                      // [2 P][T][H W] each; a set that was not asked for is NULL and not read
  int32_t *xmin, *xmax, *ymin, *ymax;
  u64 *sum_q, *sum_q2;
};

// blockIdx.z = plane * levels + l.  After the border launch the roots are the pixels >= t with parent == self.
template <bool BOX, bool STD>
__global__ __launch_bounds__(256) void at_multi_init_kernel(const uint8_t* __restrict__ q, int64_t pixels, int first, int levels, int T,
                                                            const int32_t* __restrict__ parent, AttrPlanes pl) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  const int plane = (int)(blockIdx.z / (unsigned)levels), l = (int)blockIdx.z - plane * levels, th = first + l;
  if ((int)q[(int64_t)plane * pixels + x] < th) return;
  const int64_t cell = ((int64_t)plane * T + l) * pixels + x;
  if (parent[cell] != (int32_t)x) return;
  if (BOX) {
    pl.xmin[cell] = INT32_MAX; pl.xmax[cell] = -1;
    pl.ymin[cell] = INT32_MAX; pl.ymax[cell] = -1;
  }
  if (STD) { pl.sum_q[cell] = 0; pl.sum_q2[cell] = 0; }
}

// at_root_kernel, and the run's head adds the run to every accumulator of its root (the file head says how the run is reduced).
template <bool BOX, bool STD>
__global__ __launch_bounds__(256) void at_multi_root_kernel(const uint8_t* __restrict__ q, int W, int64_t pixels, int first, int levels, int T,
                                                            int32_t* parent, int32_t* size, AttrPlanes pl) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int plane = (int)(blockIdx.z / (unsigned)levels), l = (int)blockIdx.z - plane * levels, th = first + l;
  const int64_t base = ((int64_t)plane * T + l) * pixels;
  int32_t* par = parent + base;
  int key = -1, qv = 0;
  if (x < pixels) {
    qv = (int)q[(int64_t)plane * pixels + x];
    if (qv >= th) {
      key = uf_find(par, (int)x);
      if (uf_load(par, x) != key) atomicMin(par + x, key);
    }
  }
  int last;                                              // (every lane of the wave is here: the run is formed by shuffles)
  const bool head = run_head(key, last);
  const int lane = (int)(threadIdx.x & 63);
  long long sums = 0;
  if (STD) sums = run_sum(key >= 0 ? ((long long)(qv * qv) << 32) | (long long)qv : 0ll, last);
  if (head && key >= 0) {
    const int64_t cell = base + key;
    atomicAdd(size + cell, last - lane + 1);
    if (BOX) {
      const int x0 = (int)x, x1 = x0 + (last - lane);    // (the lanes of a run with key >= 0 hold pixels of the image)
      const int i0 = x0 / W, i1 = x1 / W;
      const bool rows = i1 > i0;                         // the run holds the end of a row and the start of the next
      atomicMin(pl.xmin + cell, rows ? 0 : x0 - i0 * W);
      atomicMax(pl.xmax + cell, rows ? W - 1 : x1 - i1 * W);
      atomicMin(pl.ymin + cell, i0);
      atomicMax(pl.ymax + cell, i1);
    }
    if (STD) {
      atomicAdd(pl.sum_q + cell, (u64)(unsigned)(sums & 0xffffffffll));
      atomicAdd(pl.sum_q2 + cell, (u64)sums >> 32);
    }
  }
}

// at_count_kernel with the criteria of dmf_attr_criteria.h: thresholds 0 .. na - 1 are areas, na .. nd - 1 diagonals, nd .. n - 1 stds.
template <bool BOX, bool STD>
__global__ __launch_bounds__(256) void at_multi_count_kernel(const uint8_t* __restrict__ q, int64_t pixels, int first, int levels, int T, int na,
                                                             int nd, int n, AttrThresholds tau, const int32_t* __restrict__ parent,
                                                             const int32_t* __restrict__ size, AttrPlanes pl,
                                                             uint8_t* __restrict__ count /* [2 P][n][H W] */) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  const int plane = (int)blockIdx.z;
  const int qx = (int)q[(int64_t)plane * pixels + x];
  int add[DMF_ATTR_NMAX];
#pragma unroll
  for (int a = 0; a < DMF_ATTR_NMAX; ++a) add[a] = 0;
  for (int l = 0; l < levels && first + l <= qx; ++l) {
    const int64_t cell = ((int64_t)plane * T + l) * pixels + uf_find(parent + ((int64_t)plane * T + l) * pixels, (int)x);
    const uint32_t s = (uint32_t)size[cell];
    int32_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
    u64 sq = 0, sq2 = 0;
    if (BOX) { x0 = pl.xmin[cell]; x1 = pl.xmax[cell]; y0 = pl.ymin[cell]; y1 = pl.ymax[cell]; }
    if (STD) { sq = pl.sum_q[cell]; sq2 = pl.sum_q2[cell]; }
#pragma unroll
    for (int a = 0; a < DMF_ATTR_NMAX; ++a) {
      const uint32_t t = (uint32_t)tau.t[a];
      bool ok = false;
      if (a < na) ok = attr_crit_area(s, t);
      else if (BOX && a < nd) ok = attr_crit_diagonal(x0, x1, y0, y1, t);
      else if (STD && a < n) ok = attr_crit_std(s, sq, sq2, t);
      add[a] += ok ? 1 : 0;
    }
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

struct AttrMultiSpace {                                  // attr_space, then the four box planes, then the two sums: as asked for
  AttrSpace area;
  int64_t box, sums, bytes;
};

static AttrMultiSpace attr_multi_space(int64_t pixels, int P, int T, bool box, bool std_) {
  AttrMultiSpace s;
  s.area = attr_space(pixels, P, T);
  const int64_t cells = (int64_t)2 * P * T * pixels;
  s.box = s.area.bytes;
  s.sums = s.box + (box ? 4 * up16(cells * (int64_t)sizeof(int32_t)) : 0);
  s.bytes = s.sums + (std_ ? 2 * up16(cells * (int64_t)sizeof(uint64_t)) : 0);
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

// the three launches of a batch that depend on which plane sets exist
template <bool BOX, bool STD>
static int32_t attr_multi_launch(const uint8_t* q, int W, int64_t pixels, int P, int first, int levels, int T, int na, int nd, int n,
                                 const AttrThresholds& tau, int32_t* parent, int32_t* size, const AttrPlanes& pl, uint8_t* count, hipStream_t st) {
  const unsigned per = blocks_of(pixels, 256);
  const auto root = at_multi_root_kernel<BOX, STD>;      // (a name with a comma does not pass through DMF_LAUNCH)
  const auto tally = at_multi_count_kernel<BOX, STD>;
  if constexpr (BOX || STD) {                            // (areas alone: size is the only accumulator, and at_local_kernel zeroes it)
    const auto init = at_multi_init_kernel<BOX, STD>;
    DMF_LAUNCH(init, dim3(per, 1, 2 * P * levels), 256, q, pixels, first, levels, T, (const int32_t*)parent, pl);
  }
  DMF_LAUNCH(root, dim3(per, 1, 2 * P * levels), 256, q, W, pixels, first, levels, T, parent, size, pl);
  DMF_LAUNCH(tally, dim3(per, 1, 2 * P), 256, q, pixels, first, levels, T, na, nd, n, tau, (const int32_t*)parent, (const int32_t*)size, pl, count);
  return 0;
}

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

int64_t dmf_attr_multi_workspace_bytes(int32_t H, int32_t W, int32_t P, int32_t n_diag, int32_t n_std, int32_t T) {
  if (!attr_extent_ok(H, W) || P < 1 || P > 64 || n_diag < 0 || n_diag >= DMF_ATTR_NMAX || n_std < 0 || n_std >= DMF_ATTR_NMAX ||
      n_diag + n_std >= DMF_ATTR_NMAX || T < 1 || T > DMF_ATTR_BATCH_MAX)
    return -1;
  if (n_std > 0 && (int64_t)H * W > DMF_ATTR_STD_PIXELS_MAX) return -1;
  return attr_multi_space((int64_t)H * W, P, T, n_diag > 0, n_std > 0).bytes;
}

int32_t dmf_attr_multi_levels(const uint8_t* q, int32_t H, int32_t W, int32_t P, const int32_t* thresholds, int32_t n_area, int32_t n_diag,
                              int32_t n_std, int32_t L, int32_t first_level, int32_t levels, int32_t T, uint8_t* count, void* workspace,
                              int64_t workspace_bytes, void* stream) {
  if (q == nullptr || thresholds == nullptr || count == nullptr || workspace == nullptr) return 1;
  if (!attr_extent_ok(H, W)) return 2;
  if (P < 1 || P > 64) return 3;
  if (!attr_areas_ok(thresholds, n_area)) return 4;
  if (L < 2 || L > DMF_ATTR_LEVELS_MAX) return 11;
  if (n_diag < 0 || n_std < 0 || (int64_t)n_area + n_diag + n_std > DMF_ATTR_NMAX) return 14;
  const int32_t n = n_area + n_diag + n_std;
  for (int i = n_area; i < n; ++i) {
    const bool first_of_its_kind = i == n_area || i == n_area + n_diag;
    if (thresholds[i] < 1 || (!first_of_its_kind && thresholds[i] <= thresholds[i - 1])) return 14;
    if (i >= n_area + n_diag && thresholds[i] > L - 1) return 14;
  }
  const int64_t pixels = (int64_t)H * W;
  if (n_std > 0 && pixels > DMF_ATTR_STD_PIXELS_MAX) return 13;
  if (T < 1 || T > DMF_ATTR_BATCH_MAX || levels < 1 || levels > T || first_level < 1 || first_level + levels - 1 > L - 1) return 10;
  const bool box = n_diag > 0, std_ = n_std > 0;
  const AttrMultiSpace sp = attr_multi_space(pixels, P, T, box, std_);
  if (workspace_bytes < sp.bytes) return 12;
  if (!attr_aligned(workspace, 16)) return 6;
  const void* outs[2] = {count, workspace};
  const uint64_t out_bytes[2] = {(uint64_t)2 * P * n * pixels, (uint64_t)sp.bytes};
  const void* ins[1] = {q};
  const uint64_t in_bytes[1] = {(uint64_t)2 * P * pixels};
  if (any_overlap(outs, out_bytes, 2, ins, in_bytes, 1)) return 7;
  const int64_t tx = ((int64_t)W + AT_T - 1) / AT_T, ty = ((int64_t)H + AT_T - 1) / AT_T;
  if (tx * ty > INT32_MAX) return 8;
  AttrThresholds tau = {};
  for (int i = 0; i < n; ++i) tau.t[i] = thresholds[i];
  hipStream_t st = static_cast<hipStream_t>(stream);
  char* w = static_cast<char*>(workspace);
  int32_t* parent = reinterpret_cast<int32_t*>(w + sp.area.parent);
  int32_t* size = reinterpret_cast<int32_t*>(w + sp.area.size);
  const int64_t cells = (int64_t)2 * P * T * pixels;
  const int64_t box_plane = up16(cells * (int64_t)sizeof(int32_t)), sum_plane = up16(cells * (int64_t)sizeof(uint64_t));
  AttrPlanes pl = {};
  if (box) {
    pl.xmin = reinterpret_cast<int32_t*>(w + sp.box);
    pl.xmax = reinterpret_cast<int32_t*>(w + sp.box + box_plane);
    pl.ymin = reinterpret_cast<int32_t*>(w + sp.box + 2 * box_plane);
    pl.ymax = reinterpret_cast<int32_t*>(w + sp.box + 3 * box_plane);
  }
  if (std_) {
    pl.sum_q = reinterpret_cast<u64*>(w + sp.sums);
    pl.sum_q2 = reinterpret_cast<u64*>(w + sp.sums + sum_plane);
  }
  const unsigned per = blocks_of(pixels, 256);
  DMF_LAUNCH(at_local_kernel, dim3((unsigned)(tx * ty), 1, 2 * P), AT_THREADS, q, H, W, (int)tx, first_level, levels, T, parent, size);
  DMF_LAUNCH(at_border_kernel, dim3(per, 1, 2 * P * levels), 256, q, W, pixels, first_level, levels, T, parent);
  const int na = n_area, nd = n_area + n_diag;
  if (box && std_) return attr_multi_launch<true, true>(q, W, pixels, P, first_level, levels, T, na, nd, n, tau, parent, size, pl, count, st);
  if (box) return attr_multi_launch<true, false>(q, W, pixels, P, first_level, levels, T, na, nd, n, tau, parent, size, pl, count, st);
  if (std_) return attr_multi_launch<false, true>(q, W, pixels, P, first_level, levels, T, na, nd, n, tau, parent, size, pl, count, st);
  return attr_multi_launch<false, false>(q, W, pixels, P, first_level, levels, T, na, nd, n, tau, parent, size, pl, count, st);
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
