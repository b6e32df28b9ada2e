// dmf_region_graph.hip — connected superpixels, the spectrum-aware fragment merge: fragments join the adjacent
// group with the nearest mean spectrum, groups of fragments grow, and a group that reaches min_size becomes a region (a Boruvka
// style merge over the region adjacency graph).  include/dmf.h states the arithmetic.  The union-find, the runs of a wave, the
// scan, comp's range check, DESIGN.md 24's kept rule, the quantiser and the host helpers are dmf_region_prims.h's, shared with
// dmf_regions.hip; gm_size_kernel, gm_main_kernel and the two scan kernels wrap its bodies.
//   gm_zero_kernel         sizes, region sizes, per-label maxima, statistics, round counters and the feature sums start at 0
//   gm_size_kernel         size[root] by integer atomics, one per run of equal roots in a wave
//   gm_main_kernel         per label the 64-bit atomicMax of (size, complement of root): its main component
//   gm_count_kernel        (dmf_region_graph_count) the number of components and of fragments
//   gm_flag_kernel         flag[x] = 1 at a root; gm_scan_kernel / gm_scan_blocks_kernel: its exclusive scan = the dense index
//   gm_init_kernel         per component: pixel count, kept flag, a group of its own
//   gm_sums_kernel         sum[component][band] += q(scene) by 64-bit integer atomics, one per run of equal components in a wave
//   gm_begin_kernel        a round starts: a group that reached min_size becomes kept, the active groups are counted, the means
//   gm_pairs_kernel<0>     every 4-neighbour pixel pair of two groups: d in double, atomicMin of its bit pattern per active group
//   gm_pairs_kernel<1>     the pairs that attain the minimum: atomicMin of the neighbour's id
//   gm_unite_kernel        every active group is united with its choice: links to the smaller index by atomicMin
//   gm_end_kernel          groups flattened; the sums, counts and kept flags of the absorbed roots added to the new root's
//   gm_rflag_kernel, the scan again, gm_final_kernel      dense region ids in ascending order of the groups' roots, region sizes
// The number of rounds follows from the number of fragments (the active groups at least halve per round), so the host enqueues
// that many and reads nothing; a round that finds no active group returns at once.  Integer atomics only: sums add exactly, a
// minimum is a minimum and the root of a set is its smallest index whatever the order, so no order of execution can change a bit.
// All global offsets are 64-bit.  comp is range-checked before every use, and so is every index derived from it.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_region_prims.h"

namespace dmf {
namespace gm {

constexpr int ROUNDS_MAX = DMF_REGION_GRAPH_ROUNDS_MAX;
constexpr int NONE = 0x7fffffff;           // no choice yet

// Pixel 0 is a root whatever comp holds (dmf_regions.hip lets comp decide there too).
__device__ __forceinline__ bool gm_is_root(const int32_t* comp, int64_t x, int64_t pixels) { return x == 0 || comp_root(comp, x, pixels) == (int)x; }

// The dense component index of pixel x: the scanned flag at its root, held inside 0..n - 1 (n >= 1) whatever comp holds
// (dmf_regions.hip's rg_final_kernel reads the same cells without the clamp).
__device__ __forceinline__ int gm_index(const int32_t* comp, const int32_t* prefix, const int32_t* sums, int64_t x, int64_t pixels, int n) {
  const int r = comp_root(comp, x, pixels);
  const int c = prefix[r] + sums[r / SCAN_BLOCK];
  return c < 0 ? 0 : (c < n ? c : n - 1);
}

__device__ __forceinline__ int gm_ncomp(const int32_t* ncell, int cap) {
  const int n = ncell[0];
  return n < 1 ? 1 : (n < cap ? n : cap);
}

// ------------------------------------------------------------------------------ set-up
// (a grid-stride loop: the grid is capped at 65,536 blocks; rg_zero_kernel has one cell per thread)
__global__ __launch_bounds__(256) void gm_zero_kernel(int64_t pixels, int n_labels, int64_t cells, int32_t* __restrict__ size,
                                                      int32_t* __restrict__ region_size, u64* __restrict__ best_label,
                                                      int32_t* __restrict__ stats, int n_stats, int32_t* __restrict__ nactive,
                                                      u64* __restrict__ gsum) {
  const int64_t step = (int64_t)gridDim.x * 256;
  for (int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x; x < cells || x < pixels || x < n_labels || x < ROUNDS_MAX; x += step) {
    if (x < pixels) {
      size[x] = 0;
      if (region_size != nullptr) region_size[x] = 0;
    }
    if (x < n_labels) best_label[x] = 0;
    if (x < n_stats) stats[x] = 0;
    if (x < ROUNDS_MAX && nactive != nullptr) nactive[x] = 0;
    if (x < cells) gsum[x] = 0;
  }
}

__global__ __launch_bounds__(256) void gm_size_kernel(const int32_t* __restrict__ comp, int64_t pixels, int32_t* size) {
  size_per_root(comp, pixels, size);
}

__global__ __launch_bounds__(256) void gm_main_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                      const int32_t* __restrict__ size, int64_t pixels, int n_labels, u64* best_label) {
  main_per_label(labels, comp, size, pixels, n_labels, best_label);
}

__global__ __launch_bounds__(256) void gm_count_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                       const int32_t* __restrict__ size, const u64* __restrict__ best_label, int64_t pixels,
                                                       int n_labels, int min_size, int32_t* counts) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool root = false, kept = false;
  if (x < pixels) {
    root = gm_is_root(comp, x, pixels);
    kept = root && kept_rule(labels, size, best_label, x, n_labels, min_size);
  }
  const u64 roots = __ballot(root), frags = __ballot(root && !kept);
  if ((threadIdx.x & 63) == 0) {
    if (roots) atomicAdd(counts, __popcll(roots));
    if (frags) atomicAdd(counts + 1, __popcll(frags));
  }
}

__global__ __launch_bounds__(256) void gm_flag_kernel(const int32_t* __restrict__ comp, int64_t pixels, int32_t* __restrict__ flag) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x < pixels) flag[x] = gm_is_root(comp, x, pixels) ? 1 : 0;
}

__global__ __launch_bounds__(256) void gm_scan_kernel(int32_t* flag, int64_t cells, int32_t* __restrict__ sums) {
  DMF_SCAN_IN_BLOCKS(flag, cells, sums);
}

__global__ __launch_bounds__(256) void gm_scan_blocks_kernel(int32_t* sums, int64_t blocks, int32_t* __restrict__ total_out) {
  scan_block_totals(sums, blocks, total_out);
}

__global__ __launch_bounds__(256) void gm_init_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                      const int32_t* __restrict__ size, const u64* __restrict__ best_label,
                                                      const int32_t* __restrict__ prefix, const int32_t* __restrict__ sums,
                                                      const int32_t* __restrict__ ncell, int cap, int64_t pixels, int n_labels, int min_size,
                                                      int32_t* __restrict__ gn, int32_t* __restrict__ kept, int32_t* __restrict__ gpa,
                                                      int32_t* __restrict__ stats) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  if (x == 0) stats[1] = ncell[0];
  if (!gm_is_root(comp, x, pixels)) return;
  const int c = prefix[x] + sums[x / SCAN_BLOCK];
  if ((unsigned)c >= (unsigned)gm_ncomp(ncell, cap)) return;
  gn[c] = size[x];
  kept[c] = kept_rule(labels, size, best_label, x, n_labels, min_size) ? 1 : 0;
  gpa[c] = c;
}

template <typename T>
__global__ __launch_bounds__(256) void gm_sums_kernel(const T* __restrict__ scene, int pitch, int W, int C, const int32_t* __restrict__ comp,
                                                      const int32_t* __restrict__ prefix, const int32_t* __restrict__ sums,
                                                      const int32_t* __restrict__ ncell, int cap, int64_t pixels, u64* gsum) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int key = -1;
  if (x < pixels) key = gm_index(comp, prefix, sums, x, pixels, gm_ncomp(ncell, cap));
  int last;
  const bool head = run_head(key, last);
  const bool add = head && key >= 0;
  if (__ballot(key >= 0) == 0) return;                   // (the whole wave)
  const int64_t px = key >= 0 ? x : 0;                   // a row that is no pixel's is never read
  const int i = (int)(px / W), j = (int)(px - (int64_t)i * W);
  const T* row = scene + ((int64_t)i * pitch + j) * C;
  for (int b = 0; b < C; ++b) {
    const long long q = key >= 0 ? quantise(widen(row[b])) : 0;
    const long long n = run_sum(q, last);
    if (add && n) atomicAdd(gsum + (int64_t)key * C + b, (u64)n);
  }
}

// ------------------------------------------------------------------------------ one round
// One wave per component c.  Every component copies its group into the working forest; a group's root takes the kept flag its
// pixel count earns, is counted when it is still active, clears its minimum and its choice, and forms its mean.
__global__ __launch_bounds__(256) void gm_begin_kernel(const int32_t* __restrict__ ncell, int cap, int C, int min_size, int round,
                                                       const int32_t* __restrict__ gpa, int32_t* __restrict__ gpb,
                                                       const int32_t* __restrict__ gn, int32_t* __restrict__ kept, u64* __restrict__ best,
                                                       int32_t* __restrict__ choice, const u64* __restrict__ gsum, double* __restrict__ mean,
                                                       int32_t* nactive, int32_t* stats) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= gm_ncomp(ncell, cap)) return;
  if (round > 0 && nactive[round - 1] == 0) return;      // finished: nactive[round] stays 0
  const int g = gpa[c];
  if (lane == 0) gpb[c] = g;
  if (g != (int)c) return;
  const int n = gn[c];
  if (lane == 0) {
    const int k = (kept[c] != 0 || n >= min_size) ? 1 : 0;
    kept[c] = k;
    best[c] = ~0ull;
    choice[c] = NONE;
    if (!k) {
      atomicAdd(nactive + round, 1);
      atomicMax(stats + 3, round + 1);
    }
  }
  const double div = (double)n * (double)(1ll << QBITS);            // exact: n < 2^27
  for (int b = lane; b < C; b += 64) mean[c * C + b] = (double)(long long)gsum[c * C + b] / div;
}

// d(f, g) = sum_b (m_f[b] - m_g[b])^2, the bands in ascending order, every operation rounded on its own: nothing is contracted.
__device__ __forceinline__ double gm_distance(const double* __restrict__ mf, const double* __restrict__ mg, int C) {
  double d = 0.0;
  for (int b = 0; b < C; ++b) {
    const double t = __dsub_rn(mf[b], mg[b]);
    d = __dadd_rn(d, __dmul_rn(t, t));
  }
  return d;
}

__device__ __forceinline__ void gm_min64(u64* cell, u64 v) {
  if (v < __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(cell, v);      // (a cell only decreases)
}

__device__ __forceinline__ void gm_min32(int* cell, int v) {
  if (v < __hip_atomic_load(cell, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMin(cell, v);
}

// PASS 0: the distance of the pair goes into `slot` and into the minimum of either active group; PASS 1: where it is the minimum,
// the other group's id goes into the choice.  f and g are indices this file wrote: below the component count.
template <int PASS>
__device__ __forceinline__ void gm_pair(int f, int g, int C, const int32_t* __restrict__ kept, const double* __restrict__ mean, u64* slot,
                                        u64* best, int32_t* choice) {
  if (f == g) return;
  const bool af = kept[f] == 0, ag = kept[g] == 0;
  if (!af && !ag) return;
  if (PASS == 0) {
    const u64 bits = (u64)__double_as_longlong(gm_distance(mean + (int64_t)f * C, mean + (int64_t)g * C, C));      // d >= 0 for what dmf_label_components left: ordered as integers (foreign comp may give a NaN: any order, in range)
    *slot = bits;
    if (af) gm_min64(best + f, bits);
    if (ag) gm_min64(best + g, bits);
  } else {
    const u64 bits = *slot;
    if (af && best[f] == bits) gm_min32(choice + f, g);
    if (ag && best[g] == bits) gm_min32(choice + g, f);
  }
}

template <int PASS>
__global__ __launch_bounds__(256) void gm_pairs_kernel(const int32_t* __restrict__ comp, const int32_t* __restrict__ prefix,
                                                       const int32_t* __restrict__ sums, const int32_t* __restrict__ ncell, int cap, int W,
                                                       int64_t pixels, int C, int round, const int32_t* __restrict__ nactive,
                                                       const int32_t* __restrict__ gpa, const int32_t* __restrict__ kept,
                                                       const double* __restrict__ mean, u64* dright, u64* ddown, u64* best, int32_t* choice) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels || nactive[round] == 0) return;
  const int n = gm_ncomp(ncell, cap);
  const int f = gpa[gm_index(comp, prefix, sums, x, pixels, n)];
  const int j = (int)(x % W);
  if (j + 1 < W) gm_pair<PASS>(f, gpa[gm_index(comp, prefix, sums, x + 1, pixels, n)], C, kept, mean, dright + x, best, choice);
  if (x + W < pixels) gm_pair<PASS>(f, gpa[gm_index(comp, prefix, sums, x + W, pixels, n)], C, kept, mean, ddown + x, best, choice);
}

__global__ __launch_bounds__(256) void gm_unite_kernel(const int32_t* __restrict__ ncell, int cap, int round, const int32_t* __restrict__ nactive,
                                                       const int32_t* __restrict__ gpa, const int32_t* __restrict__ kept,
                                                       const int32_t* __restrict__ choice, int32_t* gpb) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int n = gm_ncomp(ncell, cap);
  if (c >= n || nactive[round] == 0) return;
  if (gpa[c] != (int)c || kept[c] != 0) return;
  const int to = choice[c];
  if ((unsigned)to < (unsigned)n) uf_unite(gpb, (int)c, to);
}

// One wave per component: its group's new root (the working forest is immutable now; a parent is smaller than its child, so the
// walk ends).  A root of the round's start that is one no longer adds its sums, its count and its kept flag to the new root's.
__global__ __launch_bounds__(256) void gm_end_kernel(const int32_t* __restrict__ ncell, int cap, int C, int round,
                                                     const int32_t* __restrict__ nactive, int32_t* gpa, const int32_t* __restrict__ gpb,
                                                     int32_t* gn, int32_t* kept, u64* gsum) {
  const int lane = threadIdx.x & 63;
  const int64_t c = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (c >= gm_ncomp(ncell, cap) || nactive[round] == 0) return;
  const bool was = gpa[c] == (int)c;
  int r = (int)c;
  for (int up = gpb[r]; up < r; up = gpb[r]) r = up;
  if (was && r != (int)c) {
    for (int b = lane; b < C; b += 64) atomicAdd(gsum + (int64_t)r * C + b, gsum[c * C + b]);
    if (lane == 0) {
      atomicAdd(gn + r, gn[c]);
      if (kept[c] != 0) atomicOr(kept + r, 1);
    }
  }
  if (lane == 0) gpa[c] = r;
}

// ------------------------------------------------------------------------------ regions
__global__ __launch_bounds__(256) void gm_rflag_kernel(const int32_t* __restrict__ ncell, int cap, const int32_t* __restrict__ gpa,
                                                       int32_t* __restrict__ rid) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c < cap) rid[c] = (c < gm_ncomp(ncell, cap) && gpa[c] == (int)c) ? 1 : 0;
}

__global__ __launch_bounds__(256) void gm_final_kernel(const int32_t* __restrict__ comp, const int32_t* __restrict__ prefix,
                                                       const int32_t* __restrict__ sums, const int32_t* __restrict__ ncell, int cap,
                                                       int64_t pixels, const int32_t* __restrict__ gpa, const int32_t* __restrict__ rid,
                                                       const int32_t* __restrict__ rsums, int32_t* __restrict__ region, int32_t* region_size,
                                                       int32_t* stats) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int key = -1;
  if (x < pixels) {
    const int g = gpa[gm_index(comp, prefix, sums, x, pixels, gm_ncomp(ncell, cap))];
    key = rid[g] + rsums[g / SCAN_BLOCK];
    region[x] = key;
    if (x == 0) stats[2] = stats[1] - stats[0];
  }
  int last;
  const bool head = run_head(key, last);
  if (head && (unsigned)key < (u64)pixels) atomicAdd(region_size + key, last - (int)(threadIdx.x & 63) + 1);
}

// ------------------------------------------------------------------------------ host
struct Space {                                           // the workspace, every part 16-byte aligned
  int64_t best_label, size, prefix, sums, ncell, nactive, dright, ddown, gn, kept, gpa, gpb, choice, rid, rsums, best, gsum, mean, bytes;
};

static Space space(int64_t pixels, int64_t C, int64_t n_labels, int64_t cap) {
  Space s;
  const int64_t plane = up16(pixels * 4), cplane = up16(cap * 4);
  int64_t at = 0;
  auto take = [&at](int64_t bytes) { const int64_t was = at; at += up16(bytes); return was; };
  s.best_label = take(n_labels * 8);
  s.size = take(plane);
  s.prefix = take(plane);
  s.sums = take((pixels + SCAN_BLOCK - 1) / SCAN_BLOCK * 4);
  s.ncell = take(16);
  s.nactive = take(ROUNDS_MAX * 4);
  s.dright = take(pixels * 8);
  s.ddown = take(pixels * 8);
  s.gn = take(cplane);
  s.kept = take(cplane);
  s.gpa = take(cplane);
  s.gpb = take(cplane);
  s.choice = take(cplane);
  s.rid = take(cplane);
  s.rsums = take((cap + SCAN_BLOCK - 1) / SCAN_BLOCK * 4);
  s.best = take(cap * 8);
  s.gsum = take(cap * C * 8);
  s.mean = take(cap * C * 8);
  s.bytes = at;
  return s;
}

static int rounds_of(int64_t fragments) {                // 1 + floor(log2(fragments)): the active groups at least halve per round
  int r = 0;
  for (; fragments > 0; fragments >>= 1) ++r;
  return r;
}

}  // namespace gm
}  // namespace dmf

using namespace dmf;
using namespace dmf::gm;

extern "C" {

int64_t dmf_region_graph_workspace_bytes(int32_t H, int32_t W, int32_t C, int32_t n_labels, int32_t components) {
  if (H < 1 || W < 1 || C < 1 || n_labels < 0 || (int64_t)H * W >= DMF_REGION_VOTE_PIXELS_MAX) return -1;
  if (components < 1 || components > (int64_t)H * W) return -1;
  return space((int64_t)H * W, C, n_labels, components).bytes;
}

int32_t dmf_region_graph_count(const int32_t* labels, const int32_t* comp, int32_t H, int32_t W, int32_t n_labels, int32_t min_size,
                               int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  if (labels == nullptr || comp == nullptr || counts == nullptr || workspace == nullptr) return 1;
  if (H < 1 || W < 1) return 2;
  if (min_size < 1) return 14;
  if (n_labels < 0) return 15;
  const int64_t pixels = (int64_t)H * W;
  if (pixels >= DMF_REGION_VOTE_PIXELS_MAX) return 13;
  const Space s = space(pixels, 1, n_labels, 1);
  if (workspace_bytes < s.bytes) return 12;
  if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(labels) % 4 || reinterpret_cast<uintptr_t>(comp) % 4 ||
      reinterpret_cast<uintptr_t>(counts) % 4)
    return 8;
  const uint64_t plane = (uint64_t)pixels * sizeof(int32_t);
  const void* outs[2] = {counts, workspace};
  const uint64_t out_bytes[2] = {2 * sizeof(int32_t), (uint64_t)s.bytes};
  const void* ins[2] = {labels, comp};
  const uint64_t in_bytes[2] = {plane, plane};
  if (any_overlap(outs, out_bytes, 2, ins, in_bytes, 2)) return 7;
  char* base = static_cast<char*>(workspace);
  u64* best_label = reinterpret_cast<u64*>(base + s.best_label);
  int32_t* size = reinterpret_cast<int32_t*>(base + s.size);
  const int64_t zero = pixels > n_labels ? pixels : n_labels;
  const unsigned grid = blocks_of(pixels, 256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  // (counts stands in for the statistics: its two cells start at 0; no region sizes, no round counters, no sums)
  DMF_LAUNCH(gm_zero_kernel, blocks_of(zero, 256), 256, pixels, n_labels, (int64_t)0, size, (int32_t*)nullptr, best_label, counts, 2,
            (int32_t*)nullptr, (u64*)nullptr);
  DMF_LAUNCH(gm_size_kernel, grid, 256, comp, pixels, size);
  DMF_LAUNCH(gm_main_kernel, grid, 256, labels, comp, size, pixels, n_labels, best_label);
  DMF_LAUNCH(gm_count_kernel, grid, 256, labels, comp, size, best_label, pixels, n_labels, min_size, counts);
  return 0;
}

int32_t dmf_region_graph_merge(const int32_t* labels, const int32_t* comp, const void* scene, int32_t elem_bytes, int32_t pitch_pixels,
                               int32_t H, int32_t W, int32_t C, int32_t n_labels, int32_t min_size, int32_t components, int32_t fragments,
                               int32_t* region, int32_t* region_size, int32_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (labels == nullptr || comp == nullptr || scene == nullptr || region == nullptr || region_size == nullptr || stats == nullptr ||
      workspace == nullptr)
    return 1;
  if (H < 1 || W < 1 || C < 1) return 2;
  if (elem_bytes != 2 && elem_bytes != 4) return 5;
  if (pitch_pixels < W) return 6;
  if (min_size < 1) return 14;
  if (n_labels < 0) return 15;
  const int64_t pixels = (int64_t)H * W;
  if (pixels >= DMF_REGION_VOTE_PIXELS_MAX) return 13;
  if (components < 1 || components > pixels || fragments < 0 || fragments >= components) return 16;
  const Space s = space(pixels, C, n_labels, components);
  if (workspace_bytes < s.bytes) return 12;
  if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(scene) % elem_bytes || reinterpret_cast<uintptr_t>(labels) % 4 ||
      reinterpret_cast<uintptr_t>(comp) % 4 || reinterpret_cast<uintptr_t>(region) % 4 || reinterpret_cast<uintptr_t>(region_size) % 4 ||
      reinterpret_cast<uintptr_t>(stats) % 4)
    return 8;
  const int64_t cells = (int64_t)components * C;
  const uint64_t plane = (uint64_t)pixels * sizeof(int32_t);
  const void* outs[4] = {region, region_size, stats, workspace};
  const uint64_t out_bytes[4] = {plane, plane, 4 * sizeof(int32_t), (uint64_t)s.bytes};
  const void* ins[3] = {labels, comp, scene};
  const uint64_t in_bytes[3] = {plane, plane, scene_bytes(elem_bytes, pitch_pixels, H, W, C)};
  if (any_overlap(outs, out_bytes, 4, ins, in_bytes, 3)) return 7;
  char* base = static_cast<char*>(workspace);
  u64* best_label = reinterpret_cast<u64*>(base + s.best_label);
  int32_t* size = reinterpret_cast<int32_t*>(base + s.size);
  int32_t* prefix = reinterpret_cast<int32_t*>(base + s.prefix);
  int32_t* sums = reinterpret_cast<int32_t*>(base + s.sums);
  int32_t* ncell = reinterpret_cast<int32_t*>(base + s.ncell);
  int32_t* nactive = reinterpret_cast<int32_t*>(base + s.nactive);
  u64* dright = reinterpret_cast<u64*>(base + s.dright);
  u64* ddown = reinterpret_cast<u64*>(base + s.ddown);
  int32_t* gn = reinterpret_cast<int32_t*>(base + s.gn);
  int32_t* kept = reinterpret_cast<int32_t*>(base + s.kept);
  int32_t* gpa = reinterpret_cast<int32_t*>(base + s.gpa);
  int32_t* gpb = reinterpret_cast<int32_t*>(base + s.gpb);
  int32_t* choice = reinterpret_cast<int32_t*>(base + s.choice);
  int32_t* rid = reinterpret_cast<int32_t*>(base + s.rid);
  int32_t* rsums = reinterpret_cast<int32_t*>(base + s.rsums);
  u64* best = reinterpret_cast<u64*>(base + s.best);
  u64* gsum = reinterpret_cast<u64*>(base + s.gsum);
  double* mean = reinterpret_cast<double*>(base + s.mean);
  const int cap = components;
  const int64_t scan_blocks = (pixels + SCAN_BLOCK - 1) / SCAN_BLOCK, rscan_blocks = ((int64_t)cap + SCAN_BLOCK - 1) / SCAN_BLOCK;
  int64_t zero = cells > pixels ? cells : pixels;
  if (zero < n_labels) zero = n_labels;
  if (zero < ROUNDS_MAX) zero = ROUNDS_MAX;
  const int64_t zero_blocks = (zero + 255) / 256;
  const unsigned grid = blocks_of(pixels, 256), grid_c = blocks_of(cap, 256), grid_w = blocks_of(cap, 4);
  hipStream_t st = static_cast<hipStream_t>(stream);
  DMF_LAUNCH(gm_zero_kernel, (unsigned)(zero_blocks < 65536 ? zero_blocks : 65536), 256, pixels, n_labels, cells, size, region_size, best_label, stats,
            4, nactive, gsum);
  DMF_LAUNCH(gm_size_kernel, grid, 256, comp, pixels, size);
  DMF_LAUNCH(gm_main_kernel, grid, 256, labels, comp, size, pixels, n_labels, best_label);
  DMF_LAUNCH(gm_flag_kernel, grid, 256, comp, pixels, prefix);
  DMF_LAUNCH(gm_scan_kernel, (unsigned)scan_blocks, 256, prefix, pixels, sums);
  DMF_LAUNCH(gm_scan_blocks_kernel, 1, 256, sums, scan_blocks, ncell);
  DMF_LAUNCH(gm_init_kernel, grid, 256, labels, comp, size, best_label, prefix, sums, ncell, cap, pixels, n_labels, min_size, gn, kept, gpa, stats);
  if (elem_bytes == 4)
    DMF_LAUNCH(gm_sums_kernel<float>, grid, 256, static_cast<const float*>(scene), pitch_pixels, W, C, comp, prefix, sums, ncell, cap, pixels, gsum);
  else
    DMF_LAUNCH(gm_sums_kernel<__half>, grid, 256, static_cast<const __half*>(scene), pitch_pixels, W, C, comp, prefix, sums, ncell, cap, pixels, gsum);
  const int rounds = rounds_of(fragments);               // <= ROUNDS_MAX: fragments < 2^27
  for (int k = 0; k < rounds; ++k) {
    DMF_LAUNCH(gm_begin_kernel, grid_w, 256, ncell, cap, C, min_size, k, gpa, gpb, gn, kept, best, choice, gsum, mean, nactive, stats);
    DMF_LAUNCH(gm_pairs_kernel<0>, grid, 256, comp, prefix, sums, ncell, cap, W, pixels, C, k, nactive, gpa, kept, mean, dright, ddown, best, choice);
    DMF_LAUNCH(gm_pairs_kernel<1>, grid, 256, comp, prefix, sums, ncell, cap, W, pixels, C, k, nactive, gpa, kept, mean, dright, ddown, best, choice);
    DMF_LAUNCH(gm_unite_kernel, grid_c, 256, ncell, cap, k, nactive, gpa, kept, choice, gpb);
    DMF_LAUNCH(gm_end_kernel, grid_w, 256, ncell, cap, C, k, nactive, gpa, gpb, gn, kept, gsum);
  }
  DMF_LAUNCH(gm_rflag_kernel, grid_c, 256, ncell, cap, gpa, rid);
  DMF_LAUNCH(gm_scan_kernel, (unsigned)rscan_blocks, 256, rid, (int64_t)cap, rsums);
  DMF_LAUNCH(gm_scan_blocks_kernel, 1, 256, rsums, rscan_blocks, stats);
  DMF_LAUNCH(gm_final_kernel, grid, 256, comp, prefix, sums, ncell, cap, pixels, gpa, rid, rsums, region, region_size, stats);
  return 0;
}

}  // extern "C"
