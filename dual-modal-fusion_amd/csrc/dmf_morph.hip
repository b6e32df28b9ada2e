// dmf_morph.hip — morphological profiles of the reduced bands: openings and closings by reconstruction of the
// first P principal components at a ladder of n radii, stacked as extra bands in front of the network (`band_profile: morph`).
//   morph_rows_kernel / morph_cols_kernel     the 2 P mask planes and the 2 n P marker planes (dmf_morph_markers)
//   morph_round_kernel                        one round of the reconstruction of all planes (dmf_morph_reconstruct)
//   morph_stack_kernel                        the profile [H][W][C] from the planes (dmf_morph_stack)
// All arithmetic is min / max of fp32 values whose zeros are +0 (every value read is canonicalised once as x + 0.0f), so no
// order of execution can change a bit.
//
// Only erosions and reconstructions by dilation are computed.  The closing side works on the negated plane: with g = -f,
// delta_r(f) = -eps_r(g) and R^eps(m | f) = -R^delta(-m | g); negation is exact, and -0 is canonicalised again where a negated
// value is formed.  Side s (0 opening, 1 closing), component p and radius index i give mask plane s P + p and marker plane
// q = (s P + p) n + i; the mask of plane q is plane q / n.
//
// Markers.  eps_r is separable: a row pass (scores -> mask planes and the row minima of every radius) and a column pass.  Either
// stages a line segment with a halo of DMF_MORPH_RMAX in LDS (+inf outside the image: the window is clipped) and forms the
// running minimum by doubling, m_2k[i] = min(m_k[i], m_k[i + k]); m_p with p the largest power of two <= w = 2 r + 1 gives the
// window as min(m_p[i - r], m_p[i + r + 1 - p]): at most 6 levels and 2 taps for 65 taps, and one staging serves every radius.
//
// Reconstruction.  A workgroup owns a tile of 32 x 32 pixels and stages it with a halo of 8 (48 x 48, rows 49 floats apart: a
// thread per row or per column reads 32 distinct banks) together with its mask; outside the image both are -inf, which never
// wins a max and never rises.  It repeats (row sweeps right and left, column sweeps down and up, one full 3 x 3 step) until a
// whole pass changes nothing, and writes the interior.  Every step sets a pixel to min(max(some of its 3 x 3), mask): values only
// rise and never pass the reconstruction, the least fixed point above the marker; and the last pass ends with a full 3 x 3 step
// that changed nothing.  When a whole round changes no tile, every pixel satisfies j = min(delta_1(j), f): the fixed point.
// Round k reads buffer k & 1 and writes the other, so a round is a function of its input alone: result and round count depend on
// (H, W, data) only.
// THE SKIP INVARIANT.  flag[k][tile] = the tile's interior differs between the two buffers after round k.  A tile is skipped in
// round k when neither it nor one of its 8 neighbours changed in round k - 1.  Then (a) its interior is equal in both buffers:
// either it ran in round k - 1 and wrote what it read, or it was skipped and they were equal before (induction; round 0 runs
// every tile); (b) the same holds for its halo, which lies in those neighbours; so (c) round k would read what round k - 1 read,
// or what an earlier round read when it last ran, and write the same values again.  Skipping it leaves both buffers as they
// would be.  When a round counts zero changed tiles, the two buffers are equal everywhere.
// counters[k & 15] counts the tiles that round k changed (int atomicAdd); a launch whose predecessor counted zero returns at once.
// No float atomics, no allocation, no host synchronisation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/dmf.h"

namespace dmf {

constexpr int MORPH_T = DMF_MORPH_TILE;                  // the tile a workgroup owns
constexpr int MORPH_HALO = 8;
constexpr int MORPH_R = MORPH_T + 2 * MORPH_HALO;        // the staged region: 48 x 48
constexpr int MORPH_PITCH = MORPH_R + 1;                 // 49: odd, so a thread per row hits 32 banks
constexpr int MORPH_RMAX = DMF_MORPH_RMAX;
constexpr int MORPH_SLOTS = 2 * DMF_MORPH_BATCH;         // the ring of round counters: this batch's and the one before
constexpr int ROW_SEG = 256, ROW_LEN = ROW_SEG + 2 * MORPH_RMAX;          // a row segment and its halo: 320 floats
constexpr int COL_W = 64, COL_SEG = 64, COL_LEN = COL_SEG + 2 * MORPH_RMAX;   // a column tile: 128 rows of 64 columns, 32 KB
static_assert(MORPH_R * MORPH_R == 9 * 256, "the full step gives every thread 9 pixels");
static_assert(MORPH_T * MORPH_T == 4 * 256, "the write-back gives every thread 4 pixels");

struct MorphRadii { int32_t r[DMF_MORPH_NMAX]; };

__device__ __forceinline__ float morph_canon(float x) { return x + 0.0f; }      // -0 -> +0; everything else as it is

// Row pass.  Block (segment, row y) of mask plane sp = s P + p: stages the canonicalised (s = 1: negated) scores of the
// segment and its halo, writes the segment's part of the mask plane, and at doubling level p2 the row minima of every radius
// with p2 <= 2 r + 1 < 2 p2.
__global__ __launch_bounds__(256) void morph_rows_kernel(const float* __restrict__ scores, int H, int W, int64_t pitch, int P, int n,
                                                         MorphRadii radii, int segs, float* __restrict__ mask,
                                                         float* __restrict__ rows /* [2 P n][H][W] */) {
  __shared__ float m[ROW_LEN];
  const int seg = (int)(blockIdx.x % (unsigned)segs), y = (int)(blockIdx.x / (unsigned)segs);
  const int sp = (int)blockIdx.z, s = sp / P, p = sp - s * P;
  const int x0 = seg * ROW_SEG - MORPH_RMAX;
  const int64_t HW = (int64_t)H * W, line = (int64_t)y * W;
  for (int i = (int)threadIdx.x; i < ROW_LEN; i += 256) {
    const int x = x0 + i;
    float v = INFINITY;                                  // outside the image: never the minimum
    if (x >= 0 && x < W) {
      v = morph_canon(scores[(line + x) * pitch + p]);
      if (s) v = morph_canon(-v);
      if (i >= MORPH_RMAX && i < MORPH_RMAX + ROW_SEG) mask[sp * HW + line + x] = v;
    }
    m[i] = v;
  }
  __syncthreads();
  const int xo = seg * ROW_SEG + (int)threadIdx.x, io = (int)threadIdx.x + MORPH_RMAX;
  for (int k = 1; k <= MORPH_RMAX; k <<= 1) {            // m[i] = the minimum of [i, i + k) -> of [i, i + 2 k), cut at the end
    float v[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = (int)threadIdx.x + 256 * e;
      if (i < ROW_LEN) v[e] = fminf(m[i], i + k < ROW_LEN ? m[i + k] : m[i]);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int i = (int)threadIdx.x + 256 * e;
      if (i < ROW_LEN) m[i] = v[e];
    }
    __syncthreads();
    const int p2 = 2 * k;
    if (xo < W) {
      for (int t = 0; t < n; ++t) {
        const int r = radii.r[t], w = 2 * r + 1;
        if (w >= p2 && w < 2 * p2)                       // [io - r, io + r] = two runs of p2; the last index read covers io + r < ROW_LEN
          rows[(int64_t)(sp * n + t) * HW + line + xo] = fminf(m[io - r], m[io + r + 1 - p2]);
      }
    }
  }
}

// Column pass.  Block (tile of 64 columns x 64 rows) of plane q with radius radii[q % n]: the same doubling down the columns.
__global__ __launch_bounds__(256) void morph_cols_kernel(const float* __restrict__ rows, int H, int W, int n, MorphRadii radii, int tilesX,
                                                         float* __restrict__ markers /* [2 P n][H][W] */) {
  __shared__ float m[COL_LEN * COL_W];
  const int q = (int)blockIdx.z, r = radii.r[q % n], w = 2 * r + 1;
  const int tx = (int)(blockIdx.x % (unsigned)tilesX), ty = (int)(blockIdx.x / (unsigned)tilesX);
  const int c = (int)threadIdx.x & 63, g = (int)threadIdx.x >> 6;
  const int x = tx * COL_W + c, y0 = ty * COL_SEG - MORPH_RMAX;
  const int64_t HW = (int64_t)H * W;
  const float* src = rows + (int64_t)q * HW;
#pragma unroll 4
  for (int e = 0; e < COL_LEN / 4; ++e) {
    const int i = g + 4 * e, y = y0 + i;
    m[i * COL_W + c] = (x < W && y >= 0 && y < H) ? src[(int64_t)y * W + x] : INFINITY;
  }
  __syncthreads();
  int p2 = 1;
  for (int k = 1; 2 * k <= w; k <<= 1) {                 // (uniform) up to the largest power of two <= w
    float v[COL_LEN / 4];
#pragma unroll
    for (int e = 0; e < COL_LEN / 4; ++e) {
      const int i = g + 4 * e;
      v[e] = fminf(m[i * COL_W + c], i + k < COL_LEN ? m[(i + k) * COL_W + c] : m[i * COL_W + c]);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < COL_LEN / 4; ++e) m[(g + 4 * e) * COL_W + c] = v[e];
    __syncthreads();
    p2 = 2 * k;
  }
  float* dst = markers + (int64_t)q * HW;
#pragma unroll 4
  for (int e = 0; e < COL_SEG / 4; ++e) {
    const int i = MORPH_RMAX + g + 4 * e, y = y0 + i;
    if (x < W && y < H) dst[(int64_t)y * W + x] = fminf(m[(i - r) * COL_W + c], m[(i + r + 1 - p2) * COL_W + c]);
  }
}

// One round of the reconstruction by dilation of every plane: blockIdx.x the tile, blockIdx.z the plane (see the head of the file).
__global__ __launch_bounds__(256) void morph_round_kernel(const float* __restrict__ mask, const float* __restrict__ src,
                                                          float* __restrict__ dst, int H, int W, int per_mask, int tilesX, int tilesY,
                                                          int k, const uint8_t* __restrict__ flag_in, uint8_t* __restrict__ flag_out,
                                                          int32_t* __restrict__ counters) {
  __shared__ float J[MORPH_R * MORPH_PITCH], F[MORPH_R * MORPH_PITCH];
  if (k > 0 && counters[(k - 1) & (MORPH_SLOTS - 1)] == 0) return;         // (uniform) the round before changed nothing: done
  const int tid = (int)threadIdx.x, q = (int)blockIdx.z;
  const int tile = (int)blockIdx.x, tx = tile % tilesX, ty = tile / tilesX;
  const int64_t tiles = (int64_t)tilesX * tilesY;
  if (k > 0) {                                           // (uniform) skipped: both buffers already hold this tile (THE SKIP INVARIANT)
    bool active = false;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int ny = ty + dy, nx = tx + dx;
        if (ny >= 0 && ny < tilesY && nx >= 0 && nx < tilesX) active |= flag_in[q * tiles + (int64_t)ny * tilesX + nx] != 0;
      }
    if (!active) {
      if (tid == 0) flag_out[q * tiles + tile] = 0;
      return;
    }
  }
  const int64_t HW = (int64_t)H * W;
  const float* sj = src + (int64_t)q * HW;
  const float* sf = mask + (int64_t)(q / per_mask) * HW;
  const int gy0 = ty * MORPH_T - MORPH_HALO, gx0 = tx * MORPH_T - MORPH_HALO;
#pragma unroll
  for (int e = 0; e < 9; ++e) {
    const int idx = tid + 256 * e, ry = idx / MORPH_R, rx = idx - ry * MORPH_R;
    const int gy = gy0 + ry, gx = gx0 + rx;
    const bool in = gy >= 0 && gy < H && gx >= 0 && gx < W;
    J[ry * MORPH_PITCH + rx] = in ? sj[(int64_t)gy * W + gx] : -INFINITY;
    F[ry * MORPH_PITCH + rx] = in ? sf[(int64_t)gy * W + gx] : -INFINITY;
  }
  __syncthreads();
  // (a value reaches every pixel it can reach in the region within MORPH_R^2 full steps, so the bound below never binds on
  // finite data; it ends the loop on NaN planes, which the callers refuse)
  for (int pass = 0; pass < MORPH_R * MORPH_R + 2; ++pass) {
    bool ch = false;
    if (tid < MORPH_R) {                                 // thread = row: a value runs the whole row right, then left
      float* j = J + tid * MORPH_PITCH;
      const float* f = F + tid * MORPH_PITCH;
      float run = j[0];
      for (int x = 1; x < MORPH_R; ++x) {
        const float v = j[x], nv = fminf(fmaxf(v, run), f[x]);
        if (nv != v) { j[x] = nv; ch = true; }
        run = nv;
      }
      for (int x = MORPH_R - 2; x >= 0; --x) {
        const float v = j[x], nv = fminf(fmaxf(v, run), f[x]);
        if (nv != v) { j[x] = nv; ch = true; }
        run = nv;
      }
    }
    __syncthreads();
    if (tid < MORPH_R) {                                 // thread = column: down, then up
      float* j = J + tid;
      const float* f = F + tid;
      float run = j[0];
      for (int y = 1; y < MORPH_R; ++y) {
        const float v = j[y * MORPH_PITCH], nv = fminf(fmaxf(v, run), f[y * MORPH_PITCH]);
        if (nv != v) { j[y * MORPH_PITCH] = nv; ch = true; }
        run = nv;
      }
      for (int y = MORPH_R - 2; y >= 0; --y) {
        const float v = j[y * MORPH_PITCH], nv = fminf(fmaxf(v, run), f[y * MORPH_PITCH]);
        if (nv != v) { j[y * MORPH_PITCH] = nv; ch = true; }
        run = nv;
      }
    }
    __syncthreads();
    float nv[9];                                         // the elementary step on the whole region, all 8 neighbours
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int idx = tid + 256 * e, ry = idx / MORPH_R, rx = idx - ry * MORPH_R;
      float mx = -INFINITY;
#pragma unroll
      for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
        for (int dx = -1; dx <= 1; ++dx) {
          const int yy = ry + dy, xx = rx + dx;
          if (yy >= 0 && yy < MORPH_R && xx >= 0 && xx < MORPH_R) mx = fmaxf(mx, J[yy * MORPH_PITCH + xx]);
        }
      nv[e] = fminf(mx, F[ry * MORPH_PITCH + rx]);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < 9; ++e) {
      const int idx = tid + 256 * e, ry = idx / MORPH_R, rx = idx - ry * MORPH_R;
      if (nv[e] != J[ry * MORPH_PITCH + rx]) { J[ry * MORPH_PITCH + rx] = nv[e]; ch = true; }
    }
    if (!__syncthreads_or(ch)) break;                    // a whole pass, the full step included, changed nothing
  }
  float* dj = dst + (int64_t)q * HW;
  bool changed = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int idx = tid + 256 * e, iy = idx / MORPH_T, ix = idx - iy * MORPH_T;
    const int gy = ty * MORPH_T + iy, gx = tx * MORPH_T + ix;
    if (gy < H && gx < W) {
      const float v = J[(iy + MORPH_HALO) * MORPH_PITCH + ix + MORPH_HALO];
      changed |= v != sj[(int64_t)gy * W + gx];
      dj[(int64_t)gy * W + gx] = v;
    }
  }
  const int any = __syncthreads_or(changed);
  if (tid == 0) {
    flag_out[q * tiles + tile] = any ? 1 : 0;
    if (any) atomicAdd(&counters[k & (MORPH_SLOTS - 1)], 1);
  }
}

// out[pixel][c], c fastest: per profiled component the closings from the widest radius down, the component, the openings from
// the narrowest up; then the components P .. K - 1 as the scores hold them.
__global__ __launch_bounds__(256) void morph_stack_kernel(const float* __restrict__ scores, int64_t HW, int K, int64_t pitch, int P, int n,
                                                          const float* __restrict__ mask, const float* __restrict__ planes,
                                                          float* __restrict__ out) {
  const int C = K + 2 * n * P, G = 2 * n + 1;
  const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= HW * C) return;
  const int64_t px = idx / C;
  const int c = (int)(idx - px * C);
  float v;
  if (c < P * G) {
    const int p = c / G, b = c - p * G;
    if (b == n) v = mask[(int64_t)p * HW + px];
    else if (b < n) v = morph_canon(-planes[(int64_t)((P + p) * n + (n - 1 - b)) * HW + px]);
    else v = planes[(int64_t)(p * n + (b - n - 1)) * HW + px];
  } else {
    v = scores[px * pitch + P + (c - P * G)];
  }
  out[idx] = v;
}

static inline int64_t morph_tiles(int32_t H, int32_t W) {
  return (int64_t)((H + MORPH_T - 1) / MORPH_T) * ((W + MORPH_T - 1) / MORPH_T);
}

static inline bool morph_extent_ok(int32_t H, int32_t W) { return H >= 1 && W >= 1 && (int64_t)H * W < DMF_MORPH_PIXELS_MAX; }

static inline bool morph_radii_ok(const int32_t* radii, int32_t n) {
  if (n < 1 || n > DMF_MORPH_NMAX) return false;
  for (int i = 0; i < n; ++i)
    if (radii[i] < 1 || radii[i] > DMF_MORPH_RMAX || (i > 0 && radii[i] <= radii[i - 1])) return false;
  return true;
}

static inline bool morph_aligned(const void* p) { return reinterpret_cast<uintptr_t>(p) % 4 == 0; }

}  // namespace dmf

using namespace dmf;

extern "C" {

int64_t dmf_morph_state_bytes(int32_t H, int32_t W, int32_t planes) {
  if (!morph_extent_ok(H, W) || planes < 1 || planes > DMF_MORPH_PLANES_MAX) return -1;
  return (MORPH_SLOTS * (int64_t)sizeof(int32_t) + 2 * planes * morph_tiles(H, W) + 15) / 16 * 16;
}

int64_t dmf_morph_workspace_bytes(int32_t H, int32_t W, int32_t P, int32_t n) {
  if (!morph_extent_ok(H, W) || P < 1 || P > 64 || n < 1 || n > DMF_MORPH_NMAX) return -1;
  return (int64_t)(2 * P + 4 * n * P) * H * W * (int64_t)sizeof(float) + dmf_morph_state_bytes(H, W, 2 * n * P);
}

int32_t dmf_morph_markers(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P, const int32_t* radii, int32_t n,
                          float* mask, float* markers, float* scratch, void* stream) {
  if (scores == nullptr || radii == nullptr || mask == nullptr || markers == nullptr || scratch == nullptr) return 1;
  if (!morph_extent_ok(H, W)) return 2;
  if (K < 1 || K > 64 || P < 1 || P > K) return 3;
  if (!morph_radii_ok(radii, n)) return 4;
  if (pitch < K) return 5;
  if (!morph_aligned(scores) || !morph_aligned(mask) || !morph_aligned(markers) || !morph_aligned(scratch)) return 6;
  if (markers == scratch || mask == markers || mask == scratch) return 7;
  const int64_t segs = (W + ROW_SEG - 1) / ROW_SEG, row_blocks = segs * H;
  const int64_t col_blocks = (int64_t)((W + COL_W - 1) / COL_W) * ((H + COL_SEG - 1) / COL_SEG);
  if (row_blocks > INT32_MAX || col_blocks > INT32_MAX || (int64_t)H * W > INT64_MAX / 4 / pitch) return 8;
  MorphRadii rr = {};
  for (int i = 0; i < n; ++i) rr.r[i] = radii[i];
  hipStream_t st = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(morph_rows_kernel, dim3((unsigned)row_blocks, 1, 2 * P), dim3(256), 0, st, scores, H, W, pitch, P, n, rr, (int)segs, mask,
                     scratch);
  if (hipGetLastError() != hipSuccess) return 9;
  hipLaunchKernelGGL(morph_cols_kernel, dim3((unsigned)col_blocks, 1, 2 * P * n), dim3(256), 0, st, scratch, H, W, n, rr,
                     (W + COL_W - 1) / COL_W, markers);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

int32_t dmf_morph_reconstruct(const float* mask, float* X, float* Y, int32_t H, int32_t W, int32_t planes, int32_t planes_per_mask,
                              int32_t first_round, int32_t rounds, void* state, void* stream) {
  if (mask == nullptr || X == nullptr || Y == nullptr || state == nullptr) return 1;
  if (!morph_extent_ok(H, W)) return 2;
  if (planes < 1 || planes > DMF_MORPH_PLANES_MAX || planes_per_mask < 1 || planes % planes_per_mask) return 3;
  if (!morph_aligned(mask) || !morph_aligned(X) || !morph_aligned(Y) || !morph_aligned(state)) return 6;
  if (X == Y || mask == X || mask == Y) return 7;
  const int64_t tiles = morph_tiles(H, W);
  if (tiles > INT32_MAX) return 8;
  if (first_round < 0 || first_round % DMF_MORPH_BATCH || rounds < 1 || rounds > DMF_MORPH_BATCH) return 10;
  hipStream_t st = static_cast<hipStream_t>(stream);
  int32_t* counters = static_cast<int32_t*>(state);
  uint8_t* flags = reinterpret_cast<uint8_t*>(counters + MORPH_SLOTS);
  // this batch's half of the ring is cleared; the other half holds the batch before, whose last count round first_round reads
  if (hipMemsetAsync(counters + (first_round & (MORPH_SLOTS - 1)), 0, DMF_MORPH_BATCH * sizeof(int32_t), st) != hipSuccess) return 9;
  const int tilesX = (W + MORPH_T - 1) / MORPH_T, tilesY = (H + MORPH_T - 1) / MORPH_T;
  for (int k = first_round; k < first_round + rounds; ++k) {
    const uint8_t* fin = flags + (int64_t)((k + 1) & 1) * planes * tiles;       // what round k - 1 wrote
    uint8_t* fout = flags + (int64_t)(k & 1) * planes * tiles;
    hipLaunchKernelGGL(morph_round_kernel, dim3((unsigned)tiles, 1, planes), dim3(256), 0, st, mask, k & 1 ? Y : X, k & 1 ? X : Y, H, W,
                       planes_per_mask, tilesX, tilesY, k, fin, fout, counters);
    if (hipGetLastError() != hipSuccess) return 9;
  }
  return 0;
}

int32_t dmf_morph_stack(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P, int32_t n, const float* mask,
                        const float* planes, float* out, void* stream) {
  if (scores == nullptr || mask == nullptr || planes == nullptr || out == nullptr) return 1;
  if (!morph_extent_ok(H, W)) return 2;
  if (K < 1 || K > 64 || P < 1 || P > K) return 3;
  if (n < 1 || n > DMF_MORPH_NMAX) return 4;
  if (pitch < K) return 5;
  if (!morph_aligned(scores) || !morph_aligned(mask) || !morph_aligned(planes) || !morph_aligned(out)) return 6;
  if (out == scores || out == mask || out == planes) return 7;
  const int64_t total = (int64_t)H * W * (K + 2 * n * P), blocks = (total + 255) / 256;
  if (blocks > INT32_MAX || (int64_t)H * W > INT64_MAX / 4 / pitch) return 8;
  hipLaunchKernelGGL(morph_stack_kernel, dim3((unsigned)blocks), dim3(256), 0, static_cast<hipStream_t>(stream), scores, (int64_t)H * W, K,
                     pitch, P, n, mask, planes, out);
  return hipGetLastError() == hipSuccess ? 0 : 9;
}

}  // extern "C"
