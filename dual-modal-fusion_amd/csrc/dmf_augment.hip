// dmf_augment.hip — flip / rotate augmentation and test-time augmentation without touching the patch gather.
//   scene_atlas_kernel   the dihedral variants of a resident padded scene [rows, cols, C], stacked along the row axis of one
//                        taller scene: slot s of dst [n_ops * slot_rows, dst_pitch, C] holds variant ops[s] at its top-left
//                        corner, zero elsewhere.  A flipped or transposed patch is then an ordinary patch of the atlas.
//   logits_mean_kernel   the mean over V variants of the logits [V][B][K], with the argmax of the mean.
// The entry points dmf_scene_atlas and dmf_logits_mean live here too (host code at the end of the file).
//
// scene_atlas_kernel is a bandwidth kernel: it moves bits (units of 2, 4, 8 or 16 bytes, the widest that divides the pixel and
// the two base addresses) and never converts.  One launch, one 1-D grid; a workgroup decodes (slot, task) from its index.
// Two regimes:
//   * wide pixels (C * elem_bytes of a few hundred bytes: 200 or 224 bands).  The pixel vector is the coalescing unit: a
//     workgroup owns a run of 1024 units of ONE destination row, its lanes store consecutive units and load the units of the
//     source pixel, which are consecutive inside the pixel whatever the variant does to the pixel's place.  No LDS.
//     Non-transposed variants of narrow pixels take the same path: a destination row is a source row, forwards or backwards.
//   * narrow pixels (the 1- or 3-band aux scene, 4 to 12 bytes; anything up to ATLAS_NARROW bytes) in a TRANSPOSED variant.
//     A destination row is a source column, so the row path would load one pixel per cache line.  A workgroup owns a 32 x 32
//     pixel tile of the destination instead and goes through LDS: it loads with the source column index fastest (row-contiguous
//     in the source), stores with the destination column index fastest (row-contiguous in the destination).  The LDS row is
//     33 pixels: with 4-byte units the transposed read of 32 lanes falls on 32 different banks.  A column- or row-reversed
//     variant only reverses the order in which a 32-pixel span of the source is walked: the same cache lines.
// Filler (the part of a slot its variant does not cover) is written as zero by whichever path owns the slot, so every byte
// of dst is written exactly once.  All global offsets are 64-bit: an atlas of a large panchromatic scene exceeds 2^32 bytes.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_rows.h"

namespace dmf {

constexpr int ATLAS_T = 256;          // threads of a workgroup
constexpr int ATLAS_UPT = 4;          // units per thread of the row path: a workgroup owns ATLAS_T * ATLAS_UPT units of a row
constexpr int ATLAS_TILE = 32;        // tile edge of the transposing path, in pixels
constexpr int ATLAS_NARROW = 48;      // a pixel of at most this many bytes is "narrow" (LDS tile: 32 * 33 * 48 bytes = 49.5 KiB)

struct AtlasArgs {
  const void* src; void* dst;
  int rows, cols, src_pitch, slot_rows, dst_pitch;
  int pw;                 // units per pixel
  int n_ops;
  int ops[8];
  unsigned tile_mask;     // bit s: slot s goes through the LDS tile
  unsigned row_items;     // workgroups of a row-path slot:  slot_rows * row_chunks
  unsigned row_chunks;    // ceil(dst_pitch * pw / (ATLAS_T * ATLAS_UPT))
  unsigned tile_items;    // workgroups of a tile-path slot: tiles_r * tiles_c
  unsigned tiles_c;       // ceil(dst_pitch / ATLAS_TILE)
};

// Source pixel (i, j) of the pixel (a, b) of variant k of a [rows, cols] array; false where the variant does not reach.
//   Y = X^T if k & 4;  rows of Y reversed if k & 2;  columns of Y reversed if k & 1.
__device__ __forceinline__ bool atlas_source(int k, int rows, int cols, int a, int b, int& i, int& j) {
  const int er = (k & 4) ? cols : rows, ec = (k & 4) ? rows : cols;       // extent of the variant
  if (a >= er || b >= ec) return false;
  if (k & 2) a = er - 1 - a;
  if (k & 1) b = ec - 1 - b;
  i = (k & 4) ? b : a;
  j = (k & 4) ? a : b;
  return true;
}

template <typename U> __device__ __forceinline__ U atlas_zero() { return U{}; }
template <> __device__ __forceinline__ uint2 atlas_zero<uint2>() { return make_uint2(0u, 0u); }
template <> __device__ __forceinline__ uint4 atlas_zero<uint4>() { return make_uint4(0u, 0u, 0u, 0u); }

template <typename U>
__global__ __launch_bounds__(ATLAS_T) void scene_atlas_kernel(AtlasArgs a) {
  extern __shared__ uint4 atlas_lds[];                   // the tile path's [32][33] pixels of pw units
  // (slot, item) of this workgroup: the slots follow one another, each with the item count of its path
  unsigned item = blockIdx.x;
  int slot = 0;
  for (; slot < a.n_ops - 1; ++slot) {
    const unsigned n = ((a.tile_mask >> slot) & 1u) ? a.tile_items : a.row_items;
    if (item < n) break;
    item -= n;
  }
  const int k = a.ops[slot];
  const U* src = static_cast<const U*>(a.src);
  U* dst = static_cast<U*>(a.dst);
  const int pw = a.pw;

  if (!((a.tile_mask >> slot) & 1u)) {
    // ---- row path: ATLAS_T * ATLAS_UPT consecutive units of destination row r of the slot
    const int r = (int)(item / a.row_chunks);
    const unsigned chunk = item - (unsigned)r * a.row_chunks;
    const int row_units = a.dst_pitch * pw;                                  // (the host has checked that it fits)
    const int u0 = (int)(chunk * (unsigned)(ATLAS_T * ATLAS_UPT)) + (int)threadIdx.x;
    U* out = dst + ((int64_t)slot * a.slot_rows + r) * row_units;
    U v[ATLAS_UPT];
#pragma unroll
    for (int q = 0; q < ATLAS_UPT; ++q) {
      const int e = u0 + q * ATLAS_T;
      v[q] = atlas_zero<U>();
      if (e < row_units) {
        const int b = e / pw, u = e - b * pw;
        int i, j;
        if (atlas_source(k, a.rows, a.cols, r, b, i, j)) v[q] = src[((int64_t)i * a.src_pitch + j) * pw + u];
      }
    }
#pragma unroll
    for (int q = 0; q < ATLAS_UPT; ++q) {
      const int e = u0 + q * ATLAS_T;
      if (e < row_units) out[e] = v[q];
    }
    return;
  }

  // ---- tile path: destination pixels [a0, a0 + 32) x [b0, b0 + 32) of the slot, through LDS
  U* tile = reinterpret_cast<U*>(atlas_lds);
  const int ta0 = (int)(item / a.tiles_c);
  const int a0 = ta0 * ATLAS_TILE, b0 = (int)(item - (unsigned)ta0 * a.tiles_c) * ATLAS_TILE;
  const int span = ATLAS_TILE * pw;                          // units of 32 pixels
  const int n = ATLAS_TILE * span;                           // units of the tile
  // load: destination ROW index fastest = source column index fastest (k & 4 is set on this path)
  for (int idx = threadIdx.x; idx < n; idx += ATLAS_T) {
    const int tb = idx / span, rem = idx - tb * span;
    const int ta = rem / pw, u = rem - ta * pw;
    int i, j;
    U v = atlas_zero<U>();
    if (a0 + ta < a.slot_rows && b0 + tb < a.dst_pitch && atlas_source(k, a.rows, a.cols, a0 + ta, b0 + tb, i, j))
      v = src[((int64_t)i * a.src_pitch + j) * pw + u];
    tile[(tb * (ATLAS_TILE + 1) + ta) * pw + u] = v;
  }
  __syncthreads();
  // store: destination column index fastest
  for (int idx = threadIdx.x; idx < n; idx += ATLAS_T) {
    const int ta = idx / span, rem = idx - ta * span;
    const int tb = rem / pw, u = rem - tb * pw;
    if (a0 + ta < a.slot_rows && b0 + tb < a.dst_pitch)
      dst[(((int64_t)slot * a.slot_rows + a0 + ta) * a.dst_pitch + b0 + tb) * pw + u] = tile[(tb * (ATLAS_TILE + 1) + ta) * pw + u];
  }
}

template <typename U>
static hipError_t atlas_launch(const AtlasArgs& a, unsigned blocks, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(scene_atlas_kernel<U>, dim3(blocks), dim3(ATLAS_T), lds, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ mean of the variants' logits
// One row per group of L lanes (dmf_rows.h): lane c adds its column over the variants in variant order and divides by
// (float)V; the group then finds the row maximum with its FIRST index.
template <int L>
__global__ __launch_bounds__(256) void logits_mean_kernel(const float* __restrict__ lv, int V, int B, int K,
                                                          float* __restrict__ logits, int32_t* __restrict__ pred) {
  const int c = row_column<L>();
  const int64_t r = row_index<L>();
  const bool live = r < B && c < K;
  float m = -INFINITY;
  if (live) {
    const int64_t o = r * K + c, plane = (int64_t)B * K;
    float s = lv[o];
    for (int v = 1; v < V; ++v) s += lv[v * plane + o];
    m = s / (float)V;
    logits[o] = m;
  }
  if (pred == nullptr) return;
  int first = c;
  row_argmax_first<L>(m, first);
  if (r < B && c == 0) pred[r] = first;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

// Return codes (include/dmf.h lists them): this file has no access to the text buffer of dmf_last_error.
int32_t dmf_scene_atlas(const void* src, int32_t elem_bytes, int32_t rows, int32_t cols, int32_t src_pitch, int32_t C,
                        const int32_t* ops, int32_t n_ops, int32_t slot_rows, int32_t dst_pitch, void* dst, void* stream) {
  if (src == nullptr || dst == nullptr || ops == nullptr) return 1;
  if (rows < 1 || cols < 1 || C < 1 || src_pitch < cols) return 2;
  if (elem_bytes != 2 && elem_bytes != 4) return 3;
  if (n_ops < 1 || n_ops > 8) return 4;
  for (int s = 0; s < n_ops; ++s) {
    if (ops[s] < 0 || ops[s] > 7) return 4;
    const int er = (ops[s] & 4) ? cols : rows, ec = (ops[s] & 4) ? rows : cols;
    if (slot_rows < er || dst_pitch < ec) return 5;
  }
  const int64_t pb = (int64_t)C * elem_bytes;
  const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
  if (s0 % elem_bytes || d0 % elem_bytes) return 6;
  const int64_t src_bytes = (((int64_t)rows - 1) * src_pitch + cols) * pb;
  const int64_t dst_bytes = (int64_t)n_ops * slot_rows * dst_pitch * pb;
  if (s0 < d0 + (uintptr_t)dst_bytes && d0 < s0 + (uintptr_t)src_bytes) return 7;
  int ub = 16;
  while (ub > elem_bytes && (pb % ub || s0 % ub || d0 % ub)) ub >>= 1;
  const int64_t pw = pb / ub;
  // a destination row in units, and the workgroup count, stay inside 32 bits
  if (pw * dst_pitch > INT32_MAX - 2 * ATLAS_T * ATLAS_UPT || pw * src_pitch > INT32_MAX) return 8;
  AtlasArgs a;
  a.src = src; a.dst = dst;
  a.rows = rows; a.cols = cols; a.src_pitch = src_pitch; a.slot_rows = slot_rows; a.dst_pitch = dst_pitch;
  a.pw = (int)pw;
  a.n_ops = n_ops;
  a.tile_mask = 0;
  for (int s = 0; s < 8; ++s) a.ops[s] = s < n_ops ? ops[s] : 0;
  const int64_t row_chunks = (pw * dst_pitch + ATLAS_T * ATLAS_UPT - 1) / (ATLAS_T * ATLAS_UPT);
  const int64_t row_items = row_chunks * slot_rows;
  const int64_t tiles_c = ((int64_t)dst_pitch + ATLAS_TILE - 1) / ATLAS_TILE;
  const int64_t tile_items = tiles_c * (((int64_t)slot_rows + ATLAS_TILE - 1) / ATLAS_TILE);
  int64_t blocks = 0;
  for (int s = 0; s < n_ops; ++s) {
    const bool tile = (ops[s] & 4) && pb <= ATLAS_NARROW;
    if (tile) a.tile_mask |= 1u << s;
    blocks += tile ? tile_items : row_items;
  }
  if (row_items > INT32_MAX || blocks > INT32_MAX) return 8;
  a.row_items = (unsigned)row_items; a.row_chunks = (unsigned)row_chunks;
  a.tile_items = (unsigned)tile_items; a.tiles_c = (unsigned)tiles_c;
  const size_t lds = a.tile_mask ? (size_t)ATLAS_TILE * (ATLAS_TILE + 1) * (size_t)pb : 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipError_t e;
  switch (ub) {
    case 16: e = atlas_launch<uint4>(a, (unsigned)blocks, lds, st); break;
    case 8: e = atlas_launch<uint2>(a, (unsigned)blocks, lds, st); break;
    case 4: e = atlas_launch<uint32_t>(a, (unsigned)blocks, lds, st); break;
    default: e = atlas_launch<uint16_t>(a, (unsigned)blocks, lds, st); break;
  }
  return e == hipSuccess ? 0 : 9;
}

int32_t dmf_logits_mean(const float* logits_v, int32_t V, int32_t B, int32_t K, float* logits, int32_t* pred, void* stream) {
  if (logits_v == nullptr || logits == nullptr) return 1;
  if (V < 1 || B < 0) return 2;
  if (K < 1 || K > DMF_KMAX) return 3;
  if (B == 0) return 0;
  hipStream_t st = static_cast<hipStream_t>(stream);
  const hipError_t e = for_row_lanes(K, [&](auto L) {
    hipLaunchKernelGGL(logits_mean_kernel<decltype(L)::value>, row_blocks<decltype(L)::value>(B), dim3(256), 0, st, logits_v, V, B, K,
                       logits, pred);
    return hipGetLastError();
  });
  return e == hipSuccess ? 0 : 9;
}

}  // extern "C"
