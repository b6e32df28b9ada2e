// dmf_segments.hip — superpixel voting of class maps: the scene is over-segmented into SLIC superpixels in the
// pixel-centric form (every pixel chooses among the up to nine clusters of its own and the adjacent grid cells; a cluster keeps
// its grid index for life: no search, no atomics, no relabelling), and every classified pixel takes its segment's class.
//   slic_init_kernel      centres [Kc][C + 2]: the spectrum and the position of the pixel in the middle of every cell
//   slic_assign_kernel    seg [H W]: the candidate with the smallest D = d2 + cw |x - centre|^2, the first slot on equality
//   slic_partial_kernel   per cell, the sums of its pixels for each of the cell's nine candidates, in one pass over the cell
//   slic_combine_kernel   per cluster, the nine partials of its 3 x 3 cells in a fixed order -> centres, counts
//   vote_sum_kernel       segprob [Kc][K], segcount [Kc]: the mean probabilities (or the class counts) of a segment's masked members
//   vote_label_kernel     label_map, prob_out: every masked pixel takes the row of its segment
// The entry points dmf_slic_workspace_bytes, dmf_slic_init, dmf_slic_assign, dmf_slic_update and dmf_segment_vote live here too
// (host code at the end of the file) and report by return code, as dmf_spatial.hip's do.  Plain HIP C++; no float atomics, every
// sum in a fixed order: the same bits on every run.  include/dmf.h states the arithmetic.  The fp16 widening, the first maximal
// class of a row and the host helpers (overlap, scene bytes, launch and check) are dmf_region_prims.h's.
//
// Memory traffic.  The scene is band-innermost.
//   * assign: a workgroup of 256 threads owns a 16 x 16 tile of pixels, one pixel per thread, whatever S is (S = 4: sixteen cells
//     per workgroup).  The bands go through LDS in chunks of SEG_CB = 16 as the affinity kernel's do (a pixel SEG_PS = 20 floats
//     apart from the next: aligned float4 reads), and with them the same chunk of the centres the tile can name: the cells that
//     16 pixels touch (at most 5 per axis at S >= 4) and one more on either side, SEG_NL x SEG_NL = 49 rows.  A pixel's nine
//     distances live in registers; pixels of one cell read the same centre rows (LDS broadcast).  There is no halo: distances
//     are pixel-to-centre, so the scene is read exactly once.
//   * update: consecutive lanes on consecutive bands.  A wave owns (cell, chunk of 64 bands) and walks the cell's pixels in row
//     order, eight loads in flight; the slot of a pixel is the same in every lane, so which of the nine accumulators takes it is
//     a scalar branch (no indexed registers, no scratch).  The partials [cell][9][C] go to the workspace and a second, small
//     kernel adds the nine that belong to a cluster in double.  The scene is read exactly once.
//   * vote: a wave owns a cluster and walks the 3S x 3S window of its nine cells row by row, 64 columns at a time (seg and mask:
//     one coalesced read per row); the members of a row are then taken in ascending column order, lanes on classes (mean), or
//     counted by class through integer LDS atomics (majority: integers, so the order cannot matter).  prob is read once.
// All global offsets are 64-bit.  A label is never used as an index: it is compared with the indices of the pixel's candidates.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dmf.h"
#include "dmf_region_prims.h"

namespace dmf {

constexpr int SEG_T = 16;                  // tile edge of the assign kernel in pixels; SEG_T * SEG_T threads
constexpr int SEG_THREADS = SEG_T * SEG_T;
constexpr int SEG_CB = 16;                 // bands per LDS chunk of the assign kernel
constexpr int SEG_PS = SEG_CB + 4;         // floats from one staged row to the next
constexpr int SEG_NL = 7;                  // local cluster grid of a tile: the cells 16 pixels touch (<= 5 at S >= 4) and one on either side
constexpr int SEG_BATCH = 8;               // pixels whose loads the update keeps in flight
constexpr int SEG_WAVES = SEG_THREADS / 64;
static_assert((SEG_T - 1 + DMF_SEG_SMIN - 1) / DMF_SEG_SMIN + 1 + 2 <= SEG_NL, "a tile's candidates fit the local grid");

// ------------------------------------------------------------------------------ init
template <typename T>
__global__ __launch_bounds__(256) void slic_init_kernel(const T* __restrict__ scene, int pitch, int H, int W, int C, int S, int gw,
                                                        int64_t total, float* __restrict__ centres) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int k = (int)(t / (C + 2)), c = (int)(t - (int64_t)k * (C + 2));
  const int gi = k / gw, gj = k - gi * gw;
  const int i = min(H - 1, gi * S + S / 2), j = min(W - 1, gj * S + S / 2);
  centres[t] = c < C ? widen(scene[((int64_t)i * pitch + j) * C + c]) : c == C ? (float)i : (float)j;
}

// ------------------------------------------------------------------------------ assign
template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void slic_assign_kernel(const T* __restrict__ scene, int pitch, int H, int W, int C, int S,
                                                                  int gh, int gw, float cw, const float* __restrict__ centres,
                                                                  int tiles_x, int32_t* __restrict__ seg) {
  __shared__ __attribute__((aligned(16))) float pix[SEG_THREADS * SEG_PS];
  __shared__ __attribute__((aligned(16))) float cen[SEG_NL * SEG_NL * SEG_PS];
  __shared__ float cpos[SEG_NL * SEG_NL * 2];
  const int tile_i = (int)(blockIdx.x / (unsigned)tiles_x);
  const int i0 = tile_i * SEG_T, j0 = (int)(blockIdx.x - (unsigned)tile_i * (unsigned)tiles_x) * SEG_T;
  const int ci0 = i0 / S - 1, cj0 = j0 / S - 1;          // the cell of local cluster (0, 0); -1 at the scene's edge
  const int ty = threadIdx.x / SEG_T, tx = threadIdx.x % SEG_T;
  const int i = i0 + ty, j = j0 + tx;
  const bool inside = i < H && j < W;
  const int gi = min(i, H - 1) / S, gj = min(j, W - 1) / S;      // (a thread outside the scene computes with the edge's cell)
  const int li = gi - ci0, lj = gj - cj0;                // 1 .. SEG_NL - 2

  for (int l = threadIdx.x; l < SEG_NL * SEG_NL; l += SEG_THREADS) {
    const int ci = ci0 + l / SEG_NL, cj = cj0 + l % SEG_NL;
    const bool in = ci >= 0 && ci < gh && cj >= 0 && cj < gw;
    const int64_t row = ((int64_t)ci * gw + cj) * (C + 2) + C;
    cpos[2 * l] = in ? centres[row] : 0.f;
    cpos[2 * l + 1] = in ? centres[row + 1] : 0.f;
  }
  float acc[9];
#pragma unroll
  for (int s = 0; s < 9; ++s) acc[s] = 0.f;

  for (int c0 = 0; c0 < C; c0 += SEG_CB) {
    __syncthreads();                                     // the previous chunk has been read
    for (int idx = threadIdx.x; idx < SEG_THREADS * SEG_CB; idx += SEG_THREADS) {
      const int p = idx / SEG_CB, c = idx - p * SEG_CB;
      const int pi = i0 + p / SEG_T, pj = j0 + p % SEG_T;
      float v = 0.f;
      if (pi < H && pj < W && c0 + c < C) v = widen(scene[((int64_t)pi * pitch + pj) * C + c0 + c]);
      pix[p * SEG_PS + c] = v;
    }
    for (int idx = threadIdx.x; idx < SEG_NL * SEG_NL * SEG_CB; idx += SEG_THREADS) {
      const int l = idx / SEG_CB, c = idx - l * SEG_CB;
      const int ci = ci0 + l / SEG_NL, cj = cj0 + l % SEG_NL;
      float v = 0.f;
      if (ci >= 0 && ci < gh && cj >= 0 && cj < gw && c0 + c < C) v = centres[((int64_t)ci * gw + cj) * (C + 2) + c0 + c];
      cen[l * SEG_PS + c] = v;
    }
    __syncthreads();
    float4 a[SEG_CB / 4];
#pragma unroll
    for (int q = 0; q < SEG_CB / 4; ++q) a[q] = reinterpret_cast<const float4*>(pix + threadIdx.x * SEG_PS)[q];
#pragma unroll
    for (int s = 0; s < 9; ++s) {
      const float4* mu = reinterpret_cast<const float4*>(cen + ((li + s / 3 - 1) * SEG_NL + lj + s % 3 - 1) * SEG_PS);
      float sum = acc[s];
#pragma unroll
      for (int q = 0; q < SEG_CB / 4; ++q) {
        const float4 b = mu[q];
        const float d0 = a[q].x - b.x, d1 = a[q].y - b.y, d2 = a[q].z - b.z, d3 = a[q].w - b.w;
        sum = fmaf(d0, d0, sum); sum = fmaf(d1, d1, sum); sum = fmaf(d2, d2, sum); sum = fmaf(d3, d3, sum);
      }
      acc[s] = sum;
    }
  }
  if (!inside) return;
  float best = INFINITY;
  int label = gi * gw + gj;                              // the pixel's own cell: always a candidate
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int u = s / 3 - 1, v = s % 3 - 1;
    if (gi + u < 0 || gi + u >= gh || gj + v < 0 || gj + v >= gw) continue;
    const int l = (li + u) * SEG_NL + lj + v;
    const float di = (float)i - cpos[2 * l], dj = (float)j - cpos[2 * l + 1];
    const float D = __fadd_rn(acc[s] / (float)C, __fmul_rn(cw, __fadd_rn(__fmul_rn(di, di), __fmul_rn(dj, dj))));
    if (D < best) { best = D; label = (gi + u) * gw + gj + v; }      // strict: the first slot on equality
  }
  seg[(int64_t)i * W + j] = label;
}

// ------------------------------------------------------------------------------ update
// The slot of label l among the candidates of cell (gi, gj), 9 where it is none of them: by comparison, never by indexing.
__device__ __forceinline__ int seg_slot(int l, int gi, int gj, int gh, int gw) {
  int slot = 9;
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int ci = gi + s / 3 - 1, cj = gj + s % 3 - 1;
    if (ci >= 0 && ci < gh && cj >= 0 && cj < gw && l == ci * gw + cj) slot = s;
  }
  return slot;
}

#define SEG_ACC(s) case s: a##s += v[e]; n##s += 1; r##s += q / nw; q##s += q % nw; break;
#define SEG_OUT(s) \
  if (live) psum[((int64_t)cell * 9 + s) * C + c] = a##s; \
  if (chunk == 0 && lane == 0) { int32_t* o = pcnt + ((int64_t)cell * 9 + s) * 4; o[0] = n##s; o[1] = r##s; o[2] = q##s; o[3] = 0; }

template <typename T>
__global__ __launch_bounds__(SEG_THREADS) void slic_partial_kernel(const T* __restrict__ scene, int pitch, int H, int W, int C, int S,
                                                                   int gh, int gw, int nb, int64_t items,
                                                                   const int32_t* __restrict__ seg, float* __restrict__ psum,
                                                                   int32_t* __restrict__ pcnt) {
  const int lane = threadIdx.x & 63;
  const int64_t item = (int64_t)blockIdx.x * SEG_WAVES + (threadIdx.x >> 6);
  if (item >= items) return;                             // (the whole wave)
  const int cell = (int)(item / nb), chunk = (int)(item - (int64_t)cell * nb);
  const int gi = cell / gw, gj = cell - gi * gw;
  const int c = chunk * 64 + lane;
  const bool live = c < C;
  const int i0 = gi * S, j0 = gj * S;
  const int nw = min(W, j0 + S) - j0, n = (min(H, i0 + S) - i0) * nw;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, a5 = 0.f, a6 = 0.f, a7 = 0.f, a8 = 0.f;
  int n0 = 0, n1 = 0, n2 = 0, n3 = 0, n4 = 0, n5 = 0, n6 = 0, n7 = 0, n8 = 0;
  int r0 = 0, r1 = 0, r2 = 0, r3 = 0, r4 = 0, r5 = 0, r6 = 0, r7 = 0, r8 = 0;      // sums of the members' rows, from the cell's first
  int q0 = 0, q1 = 0, q2 = 0, q3 = 0, q4 = 0, q5 = 0, q6 = 0, q7 = 0, q8 = 0;      // and of their columns
  for (int b = 0; b < n; b += SEG_BATCH) {
    float v[SEG_BATCH];
    int slot[SEG_BATCH];
#pragma unroll
    for (int e = 0; e < SEG_BATCH; ++e) {
      const int q = b + e;
      v[e] = 0.f;
      slot[e] = 9;
      if (q < n) {
        const int pi = i0 + q / nw, pj = j0 + q % nw;
        slot[e] = seg_slot(seg[(int64_t)pi * W + pj], gi, gj, gh, gw);
        if (live) v[e] = widen(scene[((int64_t)pi * pitch + pj) * C + c]);
      }
    }
#pragma unroll
    for (int e = 0; e < SEG_BATCH; ++e) {
      const int q = b + e;
      switch (__builtin_amdgcn_readfirstlane(slot[e])) {           // the same in every lane: a scalar branch
        SEG_ACC(0) SEG_ACC(1) SEG_ACC(2) SEG_ACC(3) SEG_ACC(4) SEG_ACC(5) SEG_ACC(6) SEG_ACC(7) SEG_ACC(8)
        default: break;
      }
    }
  }
  SEG_OUT(0) SEG_OUT(1) SEG_OUT(2) SEG_OUT(3) SEG_OUT(4) SEG_OUT(5) SEG_OUT(6) SEG_OUT(7) SEG_OUT(8)
}
#undef SEG_ACC
#undef SEG_OUT

// Cluster k = (ci, cj) collects, in ascending slot s of ITS 3 x 3 cells, what cell (ci + u, cj + v) summed for the candidate
// that k is to that cell: slot 8 - s.  Everything is added in double (the positions and counts as integers) and divided once.
__global__ __launch_bounds__(256) void slic_combine_kernel(const float* __restrict__ psum, const int32_t* __restrict__ pcnt, int C, int S,
                                                           int gh, int gw, int64_t total, float* __restrict__ centres,
                                                           int32_t* __restrict__ counts) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= total) return;
  const int k = (int)(t / (C + 2)), c = (int)(t - (int64_t)k * (C + 2));
  const int ci = k / gw, cj = k - ci * gw;
  double sum = 0.0;
  int64_t count = 0, pos = 0;
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int gi = ci + s / 3 - 1, gj = cj + s % 3 - 1;
    if (gi < 0 || gi >= gh || gj < 0 || gj >= gw) continue;
    const int64_t part = ((int64_t)gi * gw + gj) * 9 + (8 - s);
    const int32_t* o = pcnt + part * 4;
    count += o[0];
    if (c < C) sum += (double)psum[part * C + c];
    else if (c == C) pos += (int64_t)o[0] * (gi * S) + o[1];
    else pos += (int64_t)o[0] * (gj * S) + o[2];
  }
  if (c == 0) counts[k] = (int32_t)count;
  if (count > 0) centres[t] = (float)((c < C ? sum : (double)pos) / (double)count);      // no member: the row stays
}

// ------------------------------------------------------------------------------ vote
template <int MODE>
__global__ __launch_bounds__(SEG_THREADS) void vote_sum_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ mask,
                                                               const int32_t* __restrict__ seg, int H, int W, int K, int S, int gh,
                                                               int gw, float* __restrict__ segprob, int32_t* __restrict__ segcount) {
  __shared__ int hist[SEG_WAVES][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k = blockIdx.x * SEG_WAVES + wave;
  const bool active = k < gh * gw;                       // (the whole wave; an idle one walks an empty window)
  const int ci = k / gw, cj = k - ci * gw;
  const int i0 = max(0, (ci - 1) * S), i1 = active ? min(H, (ci + 2) * S) : i0, j0 = max(0, (cj - 1) * S), j1 = min(W, (cj + 2) * S);
  float acc = 0.f;
  int count = 0;
  if (MODE == 1) {
    hist[wave][lane] = 0;
    __syncthreads();
  }
  for (int i = i0; i < i1; ++i) {
    for (int jb = j0; jb < j1; jb += 64) {
      const int j = jb + lane;
      bool member = false;
      if (j < j1) {
        const int64_t x = (int64_t)i * W + j;
        // the pixel's candidates are the clusters around ITS cell: k is one of them exactly when the cell lies in k's 3 x 3
        member = seg[x] == k && mask[x] != 0;
      }
      uint64_t bal = __ballot(member);
      count += __popcll(bal);
      if (MODE == 0) {
        while (bal) {                                    // ascending columns
          const int64_t x = (int64_t)i * W + jb + (__ffsll((unsigned long long)bal) - 1);
          bal &= bal - 1;
          if (lane < K) acc += prob[x * K + lane];
        }
      } else if (member) {
        const float* p = prob + ((int64_t)i * W + j) * K;
        DMF_FIRST_MAX(p, K, cls)
        atomicAdd(&hist[wave][cls], 1);
      }
    }
  }
  if (MODE == 1) __syncthreads();                        // the counts of every lane are in
  if (!active) return;
  if (lane < K) {
    float out;
    if (MODE == 0) out = count > 0 ? acc / (float)count : 0.f;
    else out = (float)hist[wave][lane];
    segprob[(int64_t)k * K + lane] = out;
  }
  if (lane == 0) segcount[k] = count;
}

template <int MODE>
__global__ __launch_bounds__(256) void vote_label_kernel(const float* __restrict__ prob, const uint8_t* __restrict__ mask,
                                                         const int32_t* __restrict__ seg, int W, int K, int S, int gh, int gw,
                                                         int64_t pixels, const float* __restrict__ segprob,
                                                         int32_t* __restrict__ label_map, float* __restrict__ prob_out) {
  const int64_t x = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (x >= pixels) return;
  if (mask[x] == 0) {
    if (prob_out != nullptr)
      for (int c = 0; c < K; ++c) prob_out[x * K + c] = 0.f;
    return;                                              // (the label cell stays; the row of prob is never read)
  }
  const int i = (int)(x / W), j = (int)(x - (int64_t)i * W);
  const int gi = i / S, gj = j / S;
  const int l = seg[x];
  int found = -1;
#pragma unroll
  for (int s = 0; s < 9; ++s) {
    const int ci = gi + s / 3 - 1, cj = gj + s % 3 - 1;
    if (ci >= 0 && ci < gh && cj >= 0 && cj < gw && l == ci * gw + cj) found = ci * gw + cj;
  }
  const float* row = found >= 0 ? segprob + (int64_t)found * K : prob + x * K;     // no segment: the pixel stands for itself
  DMF_FIRST_MAX(row, K, cls)
  label_map[x] = cls;
  if (prob_out != nullptr)
    for (int c = 0; c < K; ++c) prob_out[x * K + c] = (found >= 0 || MODE == 0) ? row[c] : (c == cls ? 1.f : 0.f);
}

// ------------------------------------------------------------------------------ host
struct SegGrid {
  int gh, gw;
  int64_t Kc;
};

static SegGrid seg_grid(int H, int W, int S) {
  SegGrid g;
  g.gh = (H + S - 1) / S;
  g.gw = (W + S - 1) / S;
  g.Kc = (int64_t)g.gh * g.gw;
  return g;
}

// the checks every scene-reading entry point shares -> 0 or the code
static int32_t seg_scene_check(const void* scene, int elem_bytes, int pitch, int H, int W, int C, int S) {
  if (H < 1 || W < 1 || C < 1) return 2;
  if (S < DMF_SEG_SMIN || S > DMF_SEG_SMAX) return 4;
  if (elem_bytes != 2 && elem_bytes != 4) return 5;
  if (pitch < W) return 6;
  if (reinterpret_cast<uintptr_t>(scene) % elem_bytes) return 8;
  return 0;
}

// (refuses a grid beyond 32 bits, which the header's blocks_of leaves to its callers' limits)
static bool seg_blocks(int64_t n, int per, unsigned& blocks) {
  const int64_t b = (n + per - 1) / per;
  if (b > INT32_MAX) return false;
  blocks = (unsigned)b;
  return true;
}

}  // namespace dmf

using namespace dmf;

extern "C" {

// Return codes (include/dmf.h lists them): this file has no access to the text buffer of dmf_last_error.
int64_t dmf_slic_workspace_bytes(int32_t H, int32_t W, int32_t C, int32_t S) {
  if (H < 1 || W < 1 || C < 1 || S < DMF_SEG_SMIN || S > DMF_SEG_SMAX) return -1;
  const SegGrid g = seg_grid(H, W, S);
  return g.Kc * 9 * ((int64_t)C * sizeof(float) + 4 * sizeof(int32_t));
}

int32_t dmf_slic_init(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C, int32_t S,
                      float* centres, void* stream) {
  if (scene == nullptr || centres == nullptr) return 1;
  if (const int32_t rc = seg_scene_check(scene, elem_bytes, pitch_pixels, H, W, C, S)) return rc;
  const SegGrid g = seg_grid(H, W, S);
  const int64_t total = g.Kc * (C + 2);
  if (overlap(centres, (uint64_t)total * sizeof(float), scene, scene_bytes(elem_bytes, pitch_pixels, H, W, C))) return 7;
  unsigned blocks;
  if (g.Kc > INT32_MAX || !seg_blocks(total, 256, blocks)) return 8;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (elem_bytes == 2)
    DMF_LAUNCH(slic_init_kernel<__half>, blocks, 256, static_cast<const __half*>(scene), pitch_pixels, H, W, C, S, g.gw, total, centres);
  else
    DMF_LAUNCH(slic_init_kernel<float>, blocks, 256, static_cast<const float*>(scene), pitch_pixels, H, W, C, S, g.gw, total, centres);
  return 0;
}

int32_t dmf_slic_assign(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C, int32_t S,
                        float compactness, const float* centres, int32_t* seg, void* stream) {
  if (scene == nullptr || centres == nullptr || seg == nullptr) return 1;
  if (const int32_t rc = seg_scene_check(scene, elem_bytes, pitch_pixels, H, W, C, S)) return rc;
  if (!(compactness >= 0.f) || isinf(compactness)) return 10;
  const SegGrid g = seg_grid(H, W, S);
  const uint64_t seg_bytes = (uint64_t)H * W * sizeof(int32_t);
  if (overlap(seg, seg_bytes, scene, scene_bytes(elem_bytes, pitch_pixels, H, W, C)) ||
      overlap(seg, seg_bytes, centres, (uint64_t)g.Kc * (C + 2) * sizeof(float)))
    return 7;
  const int64_t tx = ((int64_t)W + SEG_T - 1) / SEG_T, ty = ((int64_t)H + SEG_T - 1) / SEG_T;
  if (g.Kc > INT32_MAX || tx * ty > INT32_MAX) return 8;
  const double ratio = (double)compactness / (double)S;
  const float cw = (float)(ratio * ratio);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (elem_bytes == 2)
    DMF_LAUNCH(slic_assign_kernel<__half>, (unsigned)(tx * ty), SEG_THREADS, static_cast<const __half*>(scene), pitch_pixels, H, W, C, S, g.gh,
               g.gw, cw, centres, (int)tx, seg);
  else
    DMF_LAUNCH(slic_assign_kernel<float>, (unsigned)(tx * ty), SEG_THREADS, static_cast<const float*>(scene), pitch_pixels, H, W, C, S, g.gh,
               g.gw, cw, centres, (int)tx, seg);
  return 0;
}

int32_t dmf_slic_update(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C, int32_t S,
                        const int32_t* seg, float* centres, int32_t* counts, void* workspace, int64_t workspace_bytes, void* stream) {
  if (scene == nullptr || seg == nullptr || centres == nullptr || counts == nullptr || workspace == nullptr) return 1;
  if (const int32_t rc = seg_scene_check(scene, elem_bytes, pitch_pixels, H, W, C, S)) return rc;
  const int64_t need = dmf_slic_workspace_bytes(H, W, C, S);
  if (workspace_bytes < need) return 12;
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return 8;
  const SegGrid g = seg_grid(H, W, S);
  const void* ins[2] = {scene, seg};
  const uint64_t in_bytes[2] = {scene_bytes(elem_bytes, pitch_pixels, H, W, C), (uint64_t)H * W * sizeof(int32_t)};
  const void* outs[3] = {centres, counts, workspace};
  const uint64_t out_bytes[3] = {(uint64_t)g.Kc * (C + 2) * sizeof(float), (uint64_t)g.Kc * sizeof(int32_t), (uint64_t)need};
  if (any_overlap(outs, out_bytes, 3, ins, in_bytes, 2)) return 7;
  const int nb = (C + 63) / 64;
  const int64_t items = g.Kc * nb, total = g.Kc * (C + 2);
  unsigned blocks_p, blocks_c;
  if (g.Kc > INT32_MAX || !seg_blocks(items, SEG_WAVES, blocks_p) || !seg_blocks(total, 256, blocks_c)) return 8;
  float* psum = static_cast<float*>(workspace);
  int32_t* pcnt = reinterpret_cast<int32_t*>(psum + g.Kc * 9 * C);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (elem_bytes == 2)
    DMF_LAUNCH(slic_partial_kernel<__half>, blocks_p, SEG_THREADS, static_cast<const __half*>(scene), pitch_pixels, H, W, C, S, g.gh, g.gw, nb,
               items, seg, psum, pcnt);
  else
    DMF_LAUNCH(slic_partial_kernel<float>, blocks_p, SEG_THREADS, static_cast<const float*>(scene), pitch_pixels, H, W, C, S, g.gh, g.gw, nb,
               items, seg, psum, pcnt);
  DMF_LAUNCH(slic_combine_kernel, blocks_c, 256, psum, pcnt, C, S, g.gh, g.gw, total, centres, counts);
  return 0;
}

int32_t dmf_segment_vote(const float* prob, const uint8_t* mask, const int32_t* seg, int32_t H, int32_t W, int32_t K, int32_t S,
                         int32_t mode, float* segprob, int32_t* segcount, int32_t* label_map, float* prob_out, void* stream) {
  if (prob == nullptr || mask == nullptr || seg == nullptr || segprob == nullptr || segcount == nullptr || label_map == nullptr) return 1;
  if (H < 1 || W < 1) return 2;
  if (K < 1 || K > DMF_KMAX) return 3;
  if (S < DMF_SEG_SMIN || S > DMF_SEG_SMAX) return 4;
  if (mode != DMF_VOTE_MEAN && mode != DMF_VOTE_MAJORITY) return 11;
  const SegGrid g = seg_grid(H, W, S);
  const uint64_t pixels = (uint64_t)H * W;
  const void* ins[3] = {prob, mask, seg};
  const uint64_t in_bytes[3] = {pixels * K * sizeof(float), pixels, pixels * sizeof(int32_t)};
  const void* outs[4] = {segprob, segcount, label_map, prob_out};
  const uint64_t out_bytes[4] = {(uint64_t)g.Kc * K * sizeof(float), (uint64_t)g.Kc * sizeof(int32_t), pixels * sizeof(int32_t),
                                 pixels * K * sizeof(float)};
  if (any_overlap(outs, out_bytes, 4, ins, in_bytes, 3)) return 7;
  unsigned blocks_s, blocks_l;
  if (g.Kc > INT32_MAX || !seg_blocks(g.Kc, SEG_WAVES, blocks_s) || !seg_blocks((int64_t)pixels, 256, blocks_l)) return 8;
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (mode == DMF_VOTE_MEAN) {
    DMF_LAUNCH(vote_sum_kernel<0>, blocks_s, SEG_THREADS, prob, mask, seg, H, W, K, S, g.gh, g.gw, segprob, segcount);
    DMF_LAUNCH(vote_label_kernel<0>, blocks_l, 256, prob, mask, seg, W, K, S, g.gh, g.gw, (int64_t)pixels, segprob, label_map, prob_out);
  } else {
    DMF_LAUNCH(vote_sum_kernel<1>, blocks_s, SEG_THREADS, prob, mask, seg, H, W, K, S, g.gh, g.gw, segprob, segcount);
    DMF_LAUNCH(vote_label_kernel<1>, blocks_l, 256, prob, mask, seg, W, K, S, g.gh, g.gw, (int64_t)pixels, segprob, label_map, prob_out);
  }
  return 0;
}

}  // extern "C"
