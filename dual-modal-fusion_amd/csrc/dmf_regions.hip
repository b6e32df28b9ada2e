// dmf_regions.hip — connected superpixels: the 4-connected components of a label image, the merge of small
// fragments into the component before them, dense region ids, and a vote over regions of any shape.
//   cc_local_kernel       a 16 x 16 tile's union-find in LDS -> parent [H W]: the raster index of the pixel's root inside the tile
//   cc_border_kernel      the pixel pairs across tile borders with equal labels: integer atomicMin links to the smaller root
//   cc_flatten_kernel     comp [H W]: every pixel follows parent (now immutable) to its root
//   rg_zero_kernel        sizes, region sizes, the per-label maxima and the three statistics start at 0
//   rg_size_kernel        size[root] by integer atomics, one per run of equal roots in a wave
//   rg_main_kernel        per label the 64-bit atomicMax of (size, complement of root): its main component
//   rg_target_kernel      per root: kept (its own target) or the component left of / above the root; the kept flags
//   rg_scan_kernel        the exclusive scan of the kept flags over raster order, per block of 1,024 pixels
//   rg_scan_blocks_kernel one workgroup scans the block totals -> R
//   rg_final_kernel       region [H W]: every pixel chases the immutable targets from its root to a kept one; region sizes
//   rv_zero_kernel, rv_sum_kernel, rv_finish_kernel, rv_label_kernel      the vote: 64-bit integer sums, regprob, labels
// The entry points dmf_region_workspace_bytes, dmf_region_vote_workspace_bytes, dmf_label_components, dmf_region_merge and
// dmf_region_vote live here too (host code at the end of the file) and report by return code, as dmf_segments.hip's do.
// Plain HIP C++; integer atomics only, so no order of execution can change a bit.  include/dmf.h states the arithmetic.
// The union-find, the runs of a wave, the scan, comp's range check, the kept rule, the quantiser and the host helpers are
// dmf_region_prims.h's, shared with dmf_region_graph.hip; rg_size_kernel, rg_main_kernel and the two scan kernels wrap its bodies.
//
// The labelling is the header's union-find on raster indices: the root of a component is its smallest raster index.  Three
// launches whatever the image holds; a one-pixel spiral only makes the chains that `find` walks longer.  A pixel's local index
// inside a tile grows with its raster index, so the tile-local root is the tile's smallest raster index.  All global offsets
// are 64-bit.  A label is only compared; comp, which dmf_region_merge does index with, is range-checked on every use.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_region_prims.h"

namespace dmf {

constexpr int RG_T = 16;                   // tile edge of the local labelling; RG_T * RG_T threads
constexpr int RG_THREADS = RG_T * RG_T;

// ------------------------------------------------------------------------------ labelling
__global__ __launch_bounds__(RG_THREADS) void cc_local_kernel(const int32_t* __restrict__ labels, int H, int W, int tiles_x,
                                                              int32_t* __restrict__ parent) {
  __shared__ int up[RG_THREADS];
  __shared__ int lab[RG_THREADS];
  const int t = threadIdx.x, ty = t / RG_T, tx = t % RG_T;
  const int tile_i = (int)(blockIdx.x / (unsigned)tiles_x);
  const int i0 = tile_i * RG_T, j0 = (int)(blockIdx.x - (unsigned)tile_i * (unsigned)tiles_x) * RG_T;
  const int i = i0 + ty, j = j0 + tx;
  const bool inside = i < H && j < W;
  const int64_t x = (int64_t)i * W + j;
  lab[t] = inside ? labels[x] : 0;
  up[t] = t;
  __syncthreads();
  if (inside) {                                          // (the pixel to the left of, or above, a pixel inside is inside)
    if (tx > 0 && lab[t - 1] == lab[t]) uf_unite(up, t, t - 1);
    if (ty > 0 && lab[t - RG_T] == lab[t]) uf_unite(up, t, t - RG_T);
  }
  __syncthreads();
  if (inside) {
    const int r = uf_find(up, t);
    parent[x] = (int32_t)((int64_t)(i0 + r / RG_T) * W + j0 + r % RG_T);
  }
}

__global__ __launch_bounds__(256) void cc_border_kernel(const int32_t* __restrict__ labels, int W, int64_t pixels, int32_t* parent) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  const int i = (int)(x / W), j = (int)(x - (int64_t)i * W);
  const bool top = i > 0 && i % RG_T == 0, left = j > 0 && j % RG_T == 0;
  if (!top && !left) return;
  const int l = labels[x];
  if (top && labels[x - W] == l) uf_unite(parent, (int)x, (int)(x - W));
  if (left && labels[x - 1] == l) uf_unite(parent, (int)x, (int)(x - 1));
}

__global__ __launch_bounds__(256) void cc_flatten_kernel(const int32_t* __restrict__ parent, int64_t pixels, int32_t* __restrict__ comp) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  int a = (int)x;
  for (int up = parent[a]; up != a; up = parent[a]) a = up;
  comp[x] = a;
}

// ------------------------------------------------------------------------------ merge
// (one cell per thread: the grid covers them all; gm_zero_kernel strides instead)
__global__ __launch_bounds__(256) void rg_zero_kernel(int64_t pixels, int n_labels, int32_t* __restrict__ size, int32_t* __restrict__ region_size,
                                                      u64* __restrict__ best, int32_t* __restrict__ stats) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x < pixels) { size[x] = 0; region_size[x] = 0; }
  if (x < n_labels) best[x] = 0;
  if (x < 4) stats[x] = 0;
}

__global__ __launch_bounds__(256) void rg_size_kernel(const int32_t* __restrict__ comp, int64_t pixels, int32_t* size) {
  size_per_root(comp, pixels, size);
}

__global__ __launch_bounds__(256) void rg_main_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                      const int32_t* __restrict__ size, int64_t pixels, int n_labels, u64* best) {
  main_per_label(labels, comp, size, pixels, n_labels, best);
}

__global__ __launch_bounds__(256) void rg_target_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ comp,
                                                        const int32_t* __restrict__ size, const u64* __restrict__ best, int W,
                                                        int64_t pixels, int n_labels, int min_size, int32_t* __restrict__ target,
                                                        int32_t* __restrict__ flag, int32_t* stats) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool root = false, kept = false;
  if (x < pixels) {
    root = comp_root(comp, x, pixels) == (int)x;         // (comp decides for pixel 0 too; gm_is_root makes it a root always)
    int to = (int)x;
    if (root) {
      kept = kept_rule(labels, size, best, x, n_labels, min_size);
      if (!kept) {
        const int j = (int)(x % W);
        to = j > 0 ? comp_root(comp, x - 1, pixels) : comp_root(comp, x - W, pixels);      // (x > 0 and column 0: a row above exists)
      }
    }
    target[x] = to;
    flag[x] = kept ? 1 : 0;
  }
  const u64 roots = __ballot(root), frags = __ballot(root && !kept);
  if ((threadIdx.x & 63) == 0) {
    if (roots) atomicAdd(stats + 1, __popcll(roots));
    if (frags) atomicAdd(stats + 2, __popcll(frags));
  }
}

__global__ __launch_bounds__(256) void rg_scan_kernel(int32_t* flag, int64_t pixels, int32_t* __restrict__ sums) {
  DMF_SCAN_IN_BLOCKS(flag, pixels, sums);
}

__global__ __launch_bounds__(256) void rg_scan_blocks_kernel(int32_t* sums, int64_t blocks, int32_t* __restrict__ stats) {
  scan_block_totals(sums, blocks, stats);                // stats[0] = R
}

__global__ __launch_bounds__(256) void rg_final_kernel(const int32_t* __restrict__ comp, const int32_t* __restrict__ target,
                                                       const int32_t* __restrict__ prefix, const int32_t* __restrict__ sums,
                                                       int64_t pixels, int32_t* __restrict__ region, int32_t* region_size) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int key = -1;
  if (x < pixels) {
    int r = comp_root(comp, x, pixels);
    for (int to = target[r]; to < r; to = target[r]) r = to;           // targets are strictly smaller: the chain ends
    key = prefix[r] + sums[r / SCAN_BLOCK];              // (r is a root; gm_index clamps, this does not)
    region[x] = key;
  }
  int last;
  const bool head = run_head(key, last);
  if (head && key >= 0) atomicAdd(region_size + key, last - (int)(threadIdx.x & 63) + 1);
}

// ------------------------------------------------------------------------------ vote
__global__ __launch_bounds__(256) void rv_zero_kernel(int64_t cells, int R, long long* __restrict__ acc, int32_t* __restrict__ regcount) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < cells) acc[t] = 0;
  if (t < R) regcount[t] = 0;
}

template <int MODE>
__global__ __launch_bounds__(256) void rv_sum_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ mask,
                                                     const int32_t* __restrict__ region, int64_t pixels, int K, int R, long long* acc,
                                                     int32_t* regcount) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int key = -1;
  if (x < pixels && mask[x] != 0) {
    const int r = region[x];
    if ((unsigned)r < (unsigned)R) key = r;
  }
  int last;
  const bool head = run_head(key, last);
  const bool add = head && key >= 0;
  if (add) atomicAdd(regcount + key, last - (int)(threadIdx.x & 63) + 1);
  if (__ballot(key >= 0) == 0) return;                   // (the whole wave)
  const float* row = prob + (key >= 0 ? x : 0) * K;      // a row that is not a member's is never read
  if (MODE == DMF_VOTE_MAJORITY) {
    const int own = key >= 0 ? first_max(row, K) : -1;
    for (int c = 0; c < K; ++c) {
      if (__ballot(own == c) == 0) continue;
      const long long n = run_sum(own == c ? 1 : 0, last);
      if (add && n) atomicAdd(reinterpret_cast<u64*>(acc + (int64_t)key * K + c), (u64)n);
    }
  } else {
    for (int c = 0; c < K; ++c) {
      const long long n = run_sum(key >= 0 ? quantise(row[c]) : 0, last);
      if (add && n) atomicAdd(reinterpret_cast<u64*>(acc + (int64_t)key * K + c), (u64)n);
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void rv_finish_kernel(const long long* __restrict__ acc, const int32_t* __restrict__ regcount, int K,
                                                        int64_t cells, float* __restrict__ regprob) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= cells) return;
  const int n = regcount[t / K];
  float out;
  if (MODE == DMF_VOTE_MAJORITY) out = (float)acc[t];
  else out = n > 0 ? (float)((double)acc[t] / ((double)n * (double)(1ll << QBITS))) : 0.f;
  regprob[t] = out;
}

template <int MODE>
__global__ __launch_bounds__(256) void rv_label_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ mask,
                                                       const int32_t* __restrict__ region, int K, int R, int64_t pixels,
                                                       const float* __restrict__ regprob, int32_t* __restrict__ label_map,
                                                       float* __restrict__ prob_out) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  if (mask[x] == 0) {
    if (prob_out != nullptr)
      for (int c = 0; c < K; ++c) prob_out[x * K + c] = 0.f;
    return;                                              // (the label cell stays; the row of prob is never read)
  }
  const int r = region[x];
  const bool found = (unsigned)r < (unsigned)R;
  const float* row = found ? regprob + (int64_t)r * K : prob + x * K;        // no region: the pixel stands for itself
  const int cls = first_max(row, K);
  label_map[x] = cls;
  if (prob_out != nullptr)
    for (int c = 0; c < K; ++c) prob_out[x * K + c] = (found || MODE == DMF_VOTE_MEAN) ? row[c] : (c == cls ? 1.f : 0.f);
}

// ------------------------------------------------------------------------------ host
struct RegionSpace {                                     // the merge's workspace, every part 16-byte aligned
  int64_t best, size, target, prefix, sums, bytes;
};

static RegionSpace region_space(int64_t pixels, int n_labels) {
  RegionSpace s;
  const int64_t plane = up16(pixels * (int64_t)sizeof(int32_t));
  s.best = 0;
  s.size = up16((int64_t)n_labels * (int64_t)sizeof(u64));
  s.target = s.size + plane;
  s.prefix = s.target + plane;
  s.sums = s.prefix + plane;
  s.bytes = s.sums + up16((pixels + SCAN_BLOCK - 1) / SCAN_BLOCK * (int64_t)sizeof(int32_t));
  return s;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

// Return codes (include/dmf.h lists them): this file has no access to the text buffer of dmf_last_error.
int64_t dmf_region_workspace_bytes(int32_t H, int32_t W, int32_t n_labels) {
  if (H < 1 || W < 1 || n_labels < 0 || (int64_t)H * W >= DMF_REGION_PIXELS_MAX) return -1;
  const int64_t pixels = (int64_t)H * W;
  const int64_t label = up16(pixels * (int64_t)sizeof(int32_t));           // dmf_label_components: parent
  const int64_t merge = region_space(pixels, n_labels).bytes;
  return label > merge ? label : merge;
}

int64_t dmf_region_vote_workspace_bytes(int32_t R, int32_t K) {
  if (R < 1 || K < 1 || K > DMF_KMAX) return -1;
  return up16((int64_t)R * K * (int64_t)sizeof(long long));
}

int32_t dmf_label_components(const int32_t* labels, int32_t H, int32_t W, int32_t* comp, void* workspace, int64_t workspace_bytes,
                             void* stream) {
  if (labels == nullptr || comp == nullptr || workspace == nullptr) return 1;
  if (H < 1 || W < 1) return 2;
  const int64_t pixels = (int64_t)H * W;
  if (pixels >= DMF_REGION_PIXELS_MAX) return 13;
  const int64_t need = up16(pixels * (int64_t)sizeof(int32_t));
  if (workspace_bytes < need) return 12;
  if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(labels) % 4 || reinterpret_cast<uintptr_t>(comp) % 4) return 8;
  const uint64_t plane = (uint64_t)pixels * sizeof(int32_t);
  const void* outs[2] = {comp, workspace};
  const uint64_t out_bytes[2] = {plane, (uint64_t)need};
  const void* ins[1] = {labels};
  const uint64_t in_bytes[1] = {plane};
  if (any_overlap(outs, out_bytes, 2, ins, in_bytes, 1)) return 7;
  const int64_t tx = ((int64_t)W + RG_T - 1) / RG_T, ty = ((int64_t)H + RG_T - 1) / RG_T;
  if (tx * ty > INT32_MAX) return 8;
  int32_t* parent = static_cast<int32_t*>(workspace);
  hipStream_t st = static_cast<hipStream_t>(stream);
  DMF_LAUNCH(cc_local_kernel, (unsigned)(tx * ty), RG_THREADS, labels, H, W, (int)tx, parent);
  DMF_LAUNCH(cc_border_kernel, blocks_of(pixels, 256), 256, labels, W, pixels, parent);
  DMF_LAUNCH(cc_flatten_kernel, blocks_of(pixels, 256), 256, parent, pixels, comp);
  return 0;
}

int32_t dmf_region_merge(const int32_t* labels, const int32_t* comp, int32_t H, int32_t W, int32_t n_labels, int32_t min_size,
                         int32_t* region, int32_t* region_size, int32_t* stats, void* workspace, int64_t workspace_bytes, void* stream) {
  if (labels == nullptr || comp == nullptr || region == nullptr || region_size == nullptr || stats == nullptr || workspace == nullptr) return 1;
  if (H < 1 || W < 1) return 2;
  if (min_size < 1) return 14;
  if (n_labels < 0) return 15;
  const int64_t pixels = (int64_t)H * W;
  if (pixels >= DMF_REGION_PIXELS_MAX) return 13;
  const RegionSpace s = region_space(pixels, n_labels);
  if (workspace_bytes < s.bytes) return 12;
  if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(labels) % 4 || reinterpret_cast<uintptr_t>(comp) % 4 ||
      reinterpret_cast<uintptr_t>(region) % 4 || reinterpret_cast<uintptr_t>(region_size) % 4 || reinterpret_cast<uintptr_t>(stats) % 4)
    return 8;
  const uint64_t plane = (uint64_t)pixels * sizeof(int32_t);
  const void* outs[4] = {region, region_size, stats, workspace};
  const uint64_t out_bytes[4] = {plane, plane, 4 * sizeof(int32_t), (uint64_t)s.bytes};
  const void* ins[2] = {labels, comp};
  const uint64_t in_bytes[2] = {plane, plane};
  if (any_overlap(outs, out_bytes, 4, ins, in_bytes, 2)) return 7;
  char* base = static_cast<char*>(workspace);
  u64* best = reinterpret_cast<u64*>(base + s.best);
  int32_t* size = reinterpret_cast<int32_t*>(base + s.size);
  int32_t* target = reinterpret_cast<int32_t*>(base + s.target);
  int32_t* prefix = reinterpret_cast<int32_t*>(base + s.prefix);
  int32_t* sums = reinterpret_cast<int32_t*>(base + s.sums);
  const int64_t scan_blocks = (pixels + SCAN_BLOCK - 1) / SCAN_BLOCK;
  const int64_t zero = pixels > n_labels ? pixels : n_labels;
  const unsigned grid = blocks_of(pixels, 256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  DMF_LAUNCH(rg_zero_kernel, blocks_of(zero > 4 ? zero : 4, 256), 256, pixels, n_labels, size, region_size, best, stats);
  DMF_LAUNCH(rg_size_kernel, grid, 256, comp, pixels, size);
  DMF_LAUNCH(rg_main_kernel, grid, 256, labels, comp, size, pixels, n_labels, best);
  DMF_LAUNCH(rg_target_kernel, grid, 256, labels, comp, size, best, W, pixels, n_labels, min_size, target, prefix, stats);
  DMF_LAUNCH(rg_scan_kernel, (unsigned)scan_blocks, 256, prefix, pixels, sums);
  DMF_LAUNCH(rg_scan_blocks_kernel, 1, 256, sums, scan_blocks, stats);
  DMF_LAUNCH(rg_final_kernel, grid, 256, comp, target, prefix, sums, pixels, region, region_size);
  return 0;
}

int32_t dmf_region_vote(const float* prob, const uint8_t* mask, const int32_t* region, int32_t H, int32_t W, int32_t K, int32_t R,
                        int32_t mode, float* regprob, int32_t* regcount, int32_t* label_map, float* prob_out, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  if (prob == nullptr || mask == nullptr || region == nullptr || regprob == nullptr || regcount == nullptr || label_map == nullptr ||
      workspace == nullptr)
    return 1;
  if (H < 1 || W < 1 || R < 1) return 2;
  if (K < 1 || K > DMF_KMAX) return 3;
  if (mode != DMF_VOTE_MEAN && mode != DMF_VOTE_MAJORITY) return 11;
  const int64_t pixels = (int64_t)H * W;
  if (pixels >= DMF_REGION_VOTE_PIXELS_MAX) return 13;
  if (R > pixels) return 2;
  const int64_t need = dmf_region_vote_workspace_bytes(R, K);
  if (workspace_bytes < need) return 12;
  if (reinterpret_cast<uintptr_t>(workspace) % 16 || reinterpret_cast<uintptr_t>(prob) % 4 || reinterpret_cast<uintptr_t>(region) % 4 ||
      reinterpret_cast<uintptr_t>(regprob) % 4 || reinterpret_cast<uintptr_t>(regcount) % 4 || reinterpret_cast<uintptr_t>(label_map) % 4 ||
      reinterpret_cast<uintptr_t>(prob_out) % 4)
    return 8;
  const uint64_t n = (uint64_t)pixels;
  const void* ins[3] = {prob, mask, region};
  const uint64_t in_bytes[3] = {n * K * sizeof(float), n, n * sizeof(int32_t)};
  const void* outs[5] = {regprob, regcount, label_map, prob_out, workspace};
  const uint64_t out_bytes[5] = {(uint64_t)R * K * sizeof(float), (uint64_t)R * sizeof(int32_t), n * sizeof(int32_t), n * K * sizeof(float),
                                 (uint64_t)need};
  if (any_overlap(outs, out_bytes, 5, ins, in_bytes, 3)) return 7;
  const int64_t cells = (int64_t)R * K;                  // < 2^27 * 64
  long long* acc = static_cast<long long*>(workspace);
  const unsigned grid = blocks_of(pixels, 256), grid_c = blocks_of(cells, 256);
  hipStream_t st = static_cast<hipStream_t>(stream);
  DMF_LAUNCH(rv_zero_kernel, grid_c, 256, cells, R, acc, regcount);
  if (mode == DMF_VOTE_MEAN) {
    DMF_LAUNCH(rv_sum_kernel<DMF_VOTE_MEAN>, grid, 256, prob, mask, region, pixels, K, R, acc, regcount);
    DMF_LAUNCH(rv_finish_kernel<DMF_VOTE_MEAN>, grid_c, 256, acc, regcount, K, cells, regprob);
    DMF_LAUNCH(rv_label_kernel<DMF_VOTE_MEAN>, grid, 256, prob, mask, region, K, R, pixels, regprob, label_map, prob_out);
  } else {
    DMF_LAUNCH(rv_sum_kernel<DMF_VOTE_MAJORITY>, grid, 256, prob, mask, region, pixels, K, R, acc, regcount);
    DMF_LAUNCH(rv_finish_kernel<DMF_VOTE_MAJORITY>, grid_c, 256, acc, regcount, K, cells, regprob);
    DMF_LAUNCH(rv_label_kernel<DMF_VOTE_MAJORITY>, grid, 256, prob, mask, region, K, R, pixels, regprob, label_map, prob_out);
  }
  return 0;
}

}  // extern "C"
