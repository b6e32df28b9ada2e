// dmf_region_prims.h — what the superpixel translation units (dmf_segments.hip, dmf_regions.hip, dmf_region_graph.hip) share,
// each stated once: the union-find, the runs of a wave, the scan, comp's range check, DESIGN.md 24's kept rule, the 2^-36 fixed
// point, the first maximal class, and the host helpers of their entry points.  include/dmf.h promises this arithmetic bit for bit.
// Every function is inlined into the kernel that calls it; no kernel is defined here (each file's code object registers its own).
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

namespace dmf {

constexpr int SCAN = 4;                    // consecutive cells per thread of the scan
constexpr int SCAN_BLOCK = 256 * SCAN;
constexpr int QBITS = 36;                  // the fixed point of the mean vote and of the feature sums: q = rint(clamp(a, 0, 1) 2^36)

using u64 = unsigned long long;

// ------------------------------------------------------------------------------ union-find
// Links go to the smaller index (Komura 2015; Playne and Hawick 2018): a parent is never larger than its child, so the root of a
// set is its smallest index, which is the canonical answer whatever order the links were made in.
// A parent cell only ever decreases, and every value it held is a member of the same set.  So a read that another XCD's L2
// serves late yields an earlier parent: `find` then stops at a node that has been linked on since, the atomicMin on that node
// returns what the cell really holds, and the loop goes on from there.  The atomics decide; the loads only shorten the way.
__device__ __forceinline__ int uf_load(const int* p, int64_t a) { return __hip_atomic_load(p + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_find(const int* p, int a) {
  for (int up = uf_load(p, a); up != a; up = uf_load(p, a)) a = up;
  return a;
}

// a and b become one set.  The larger root is linked to the smaller by atomicMin; where another link got there first, what the
// cell held before still has to meet b, and is smaller than a: the loop ends.
__device__ __forceinline__ void uf_unite(int* p, int a, int b) {
  a = uf_find(p, a);
  b = uf_find(p, b);
  while (a != b) {
    if (a < b) { const int t = a; a = b; b = t; }
    const int old = atomicMin(p + a, b);
    if (old == a) break;
    a = old;
  }
}

// ------------------------------------------------------------------------------ runs of equal keys in a wave
// Consecutive lanes hold consecutive pixels.  Lanes that hold the same key in a run of consecutive pixels combine before they
// touch memory (a region may be the whole scene): the run's head adds the run's length, or the run's segmented sum.
// -> true in the first lane of every run of equal keys; `last` = the run's last lane.
__device__ __forceinline__ bool run_head(int key, int& last) {
  const int lane = threadIdx.x & 63;
  const int before = __shfl_up(key, 1);
  const bool head = lane == 0 || before != key;
  const u64 heads = __ballot(head);
  const u64 above = lane == 63 ? 0ull : heads >> (lane + 1);          // the heads after this lane
  last = above ? lane + (__ffsll(above) - 1) : 63;
  return head;
}

// The sum of v over the lanes from this one to `last`: in a run's head, the run's sum.
__device__ __forceinline__ long long run_sum(long long v, int last) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int lo = __shfl_down((int)(v & 0xffffffffll), d);
    const int hi = __shfl_down((int)(v >> 32), d);
    if (lane + d <= last) v += (long long)(((u64)(unsigned)hi << 32) | (unsigned)lo);
  }
  return v;
}

// ------------------------------------------------------------------------------ components, sizes, the kept rule
// comp as the merges read it: a value outside the image stands for the pixel itself, so nothing is indexed out of range.
__device__ __forceinline__ int comp_root(const int32_t* comp, int64_t x, int64_t pixels) {
  const int c = comp[x];
  return (unsigned)c < (u64)pixels ? c : (int)x;
}

__device__ __forceinline__ u64 size_key(int size, int root) { return ((u64)(unsigned)size << 32) | (unsigned)~root; }

// (the body of rg_size_kernel / gm_size_kernel) size[root] by integer atomics, one per run of equal roots in a wave
__device__ __forceinline__ void size_per_root(const int32_t* comp, int64_t pixels, int32_t* size) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int key = x < pixels ? comp_root(comp, x, pixels) : -1;
  int last;
  const bool head = run_head(key, last);
  if (head && key >= 0) atomicAdd(size + key, last - (int)(threadIdx.x & 63) + 1);
}

// (the body of rg_main_kernel / gm_main_kernel) per label the 64-bit atomicMax of (size, complement of root): its main component
__device__ __forceinline__ void main_per_label(const int32_t* labels, const int32_t* comp, const int32_t* size, int64_t pixels, int n_labels,
                                               u64* best) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels || comp_root(comp, x, pixels) != (int)x) return;
  const int l = labels[x];
  if ((unsigned)l < (unsigned)n_labels) atomicMax(best + l, size_key(size[x], (int)x));
}

// DESIGN.md 24's rule for root x: size >= min_size, or root 0, or the main component of a label in 0..n_labels - 1.
__device__ __forceinline__ bool kept_rule(const int32_t* labels, const int32_t* size, const u64* best, int64_t x, int n_labels, int min_size) {
  const int l = labels[x], n = size[x];
  return n >= min_size || x == 0 || ((unsigned)l < (unsigned)n_labels && best[l] == size_key(n, (int)x));
}

// ------------------------------------------------------------------------------ scan
// -> the exclusive prefix of v over the workgroup's 256 threads; total = the sum.
__device__ __forceinline__ int block_scan(int v, int* cell, int& total) {
  const int t = threadIdx.x;
  cell[t] = v;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int add = t >= d ? cell[t - d] : 0;
    __syncthreads();
    cell[t] += add;
    __syncthreads();
  }
  const int incl = cell[t];
  total = cell[255];
  __syncthreads();
  return incl - v;
}

// (the body of rg_scan_kernel / gm_scan_kernel) flag [cells] becomes its exclusive prefix inside every block of SCAN_BLOCK cells;
// sums[b] = the block's total.  A macro: as a function the two kernels add in another operand order (profiles/region_prims.md).
#define DMF_SCAN_IN_BLOCKS(flag, cells, sums)                                  \
  do {                                                                         \
    __shared__ int cell[256];                                                  \
    const int64_t x0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * SCAN;       \
    int f[SCAN], mine = 0;                                                     \
    _Pragma("unroll") for (int e = 0; e < SCAN; ++e) {                         \
      f[e] = x0 + e < (cells) ? (flag)[x0 + e] : 0;                            \
      mine += f[e];                                                            \
    }                                                                          \
    int total;                                                                 \
    int run = block_scan(mine, cell, total);                                   \
    _Pragma("unroll") for (int e = 0; e < SCAN; ++e) {                         \
      if (x0 + e < (cells)) (flag)[x0 + e] = run;                              \
      run += f[e];                                                             \
    }                                                                          \
    if (threadIdx.x == 0) (sums)[blockIdx.x] = total;                          \
  } while (0)

// (the body of rg_scan_blocks_kernel / gm_scan_blocks_kernel) One workgroup: sums [blocks] becomes its exclusive prefix;
// total_out[0] = the sum of all.
__device__ __forceinline__ void scan_block_totals(int32_t* sums, int64_t blocks, int32_t* total_out) {
  __shared__ int cell[256];
  int carry = 0;
  for (int64_t b0 = 0; b0 < blocks; b0 += 256) {
    const int64_t b = b0 + threadIdx.x;
    const int v = b < blocks ? sums[b] : 0;
    int total;
    const int before = block_scan(v, cell, total);
    if (b < blocks) sums[b] = carry + before;
    carry += total;
  }
  if (threadIdx.x == 0) total_out[0] = carry;
}

// ------------------------------------------------------------------------------ values
__device__ __forceinline__ long long quantise(float a) {
  const float in = a > 0.f ? (a < 1.f ? a : 1.f) : 0.f;              // a NaN counts as 0
  return (long long)rintf(in * (float)(1ll << QBITS));              // (a power of two: the product is exact)
}

// `int cls` = the first maximal class of row [K] (strict >: the first maximal index).  dmf_segments.hip's kernels, which had
// the loop written out, take the macro: with the function their loop comes out in another order (profiles/region_prims.md).
#define DMF_FIRST_MAX(row, K, cls)                       \
  float cls##_top = (row)[0];                            \
  int cls = 0;                                           \
  for (int c = 1; c < (K); ++c) {                        \
    const float v = (row)[c];                            \
    if (v > cls##_top) { cls##_top = v; cls = c; }       \
  }

__device__ __forceinline__ int first_max(const float* row, int K) {
  DMF_FIRST_MAX(row, K, cls)
  return cls;
}

__device__ __forceinline__ float widen(float a) { return a; }
__device__ __forceinline__ float widen(__half a) { return __half2float(a); }

// ------------------------------------------------------------------------------ host
static inline bool overlap(const void* a, uint64_t abytes, const void* b, uint64_t bbytes) {
  const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
  return a0 < b0 + bbytes && b0 < a0 + abytes;
}

// outputs against inputs and against each other (a NULL output is absent) -> true where two of them meet
static inline bool any_overlap(const void* const* outs, const uint64_t* out_bytes, int n_out, const void* const* ins, const uint64_t* in_bytes,
                               int n_in) {
  for (int o = 0; o < n_out; ++o) {
    if (outs[o] == nullptr) continue;
    for (int p = 0; p < n_in; ++p)
      if (overlap(outs[o], out_bytes[o], ins[p], in_bytes[p])) return true;
    for (int p = o + 1; p < n_out; ++p)
      if (outs[p] != nullptr && overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return true;
  }
  return false;
}

static inline unsigned blocks_of(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }      // (n < 2^31: the grid holds it)

static inline int64_t up16(int64_t n) { return (n + 15) / 16 * 16; }

// the bytes of a band-innermost scene of H rows, `pitch` pixels apart, from its first to the last one read
static inline uint64_t scene_bytes(int elem_bytes, int pitch, int H, int W, int C) { return (((uint64_t)(H - 1) * pitch + W) * C) * elem_bytes; }

}  // namespace dmf

// launch on the entry point's stream `st`; the entry point returns 9 where the launch failed
#define DMF_LAUNCH(kernel, grid, block, ...)                                        \
  do {                                                                              \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, st, __VA_ARGS__);        \
    if (hipGetLastError() != hipSuccess) return 9;                                  \
  } while (0)
