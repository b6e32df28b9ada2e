// dmf_calib.hip — calibrated confidence on the evaluation side: what can be said about a row of logits
// beyond its argmax.
//   softmax_stats_kernel        argmax, confidence, margin and entropy of every row, optionally scattered into [H, W] maps
//   calib_accum_kernel          the reliability histogram (count, hits, confidence sum as a 2^-32 fixed-point integer)
//   temperature_init_kernel / temperature_rows_kernel / temperature_final_kernel
//                               temperature scaling (Guo et al. 2017): NLL, gradient and curvature in beta = 1 / T over a split,
//                               in double, and the safeguarded Newton step on the device
// Plain HIP C++; every result is the same bits on every run (integer atomics, fixed summation orders).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dmf_kargs.h"
#include "dmf_rows.h"

namespace dmf {

// ------------------------------------------------------------------------------ softmax statistics
// One row per group of L lanes (dmf_rows.h).  Beyond the softmax terms: S = sum e t for the entropy ln Z - S / Z, and e2, the
// largest e over c != pred, for the margin (1 - e2) / Z.
template <int L>
__global__ __launch_bounds__(256) void softmax_stats_kernel(const float* __restrict__ logits, int B, int K,
                                                            const float* __restrict__ inv_temp, const int32_t* __restrict__ xy, int W,
                                                            int32_t* __restrict__ pred, float* __restrict__ conf,
                                                            float* __restrict__ margin, float* __restrict__ entropy) {
  const int c = row_column<L>();
  const int64_t r = row_index<L>();
  const bool row = r < B;
  const float beta = inv_temp != nullptr ? inv_temp[0] : 1.f;
  const RowSoftmax s = row_softmax<L>(row && c < K ? logits[(size_t)r * K + c] : -INFINITY, c, beta);
  float Z = s.e;
  float S = s.e == 0.f ? 0.f : s.e * s.t;                        // (a term with e == 0 counts as 0: 0 * -inf is not a number)
  float e2 = c == s.first ? 0.f : s.e;                           // K == 1: 0
  row_butterfly<L>([&](auto other) {
    Z += other(Z);
    S += other(S);
    e2 = fmaxf(e2, other(e2));
  });
  if (!row || c != 0) return;
  const size_t o = xy != nullptr ? (size_t)xy[2 * r] * W + xy[2 * r + 1] : (size_t)r;     // labelmap_kernel's addressing
  if (pred != nullptr) pred[o] = s.first;
  if (conf != nullptr) conf[o] = 1.f / Z;
  if (margin != nullptr) margin[o] = (1.f - e2) / Z;
  if (entropy != nullptr) entropy[o] = fmaxf(0.f, logf(Z) - S / Z);
}

hipError_t launch_softmax_stats(const SoftmaxStatsArgs& a, hipStream_t st) {
  return for_row_lanes(a.K, [&](auto L) {
    hipLaunchKernelGGL(softmax_stats_kernel<decltype(L)::value>, row_blocks<decltype(L)::value>(a.B), dim3(256), 0, st, a.logits, a.B,
                       a.K, a.inv_temp, a.xy, a.W, a.pred, a.conf, a.margin, a.entropy);
    return hipGetLastError();
  });
}

// ------------------------------------------------------------------------------ reliability histogram
// hist [nbins][3]: rows, hits, sum of conf * 2^32 as an integer — exact and independent of the order (a conf >= 1/64 has no
// bits below 2^-30).  Every workgroup counts in LDS and adds its non-empty cells to the global histogram: integer atomics on
// unsigned long long, as confusion_kernel's.
constexpr int CALIB_MAX_BINS = 1024;

__global__ __launch_bounds__(256) void calib_accum_kernel(const float* __restrict__ conf, const int32_t* __restrict__ pred,
                                                          const int32_t* __restrict__ target, int B, int K, int nbins,
                                                          unsigned long long* hist) {
  __shared__ unsigned long long cell[3 * CALIB_MAX_BINS];
  for (int i = threadIdx.x; i < 3 * nbins; i += 256) cell[i] = 0ull;
  __syncthreads();
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < B) {
    const int t = target[i];
    if (t >= 0 && t < K) {
      const float cf = conf[i];
      const float fb = cf * (float)nbins;
      const int b = fb >= (float)nbins ? nbins - 1 : (fb > 0.f ? (int)fb : 0);      // min(nbins - 1, (int)(conf * nbins)), kept in range
      atomicAdd(&cell[3 * b], 1ull);
      if (pred[i] == t) atomicAdd(&cell[3 * b + 1], 1ull);
      atomicAdd(&cell[3 * b + 2], (unsigned long long)llrint((double)cf * 4294967296.0));
    }
  }
  __syncthreads();
  for (int j = threadIdx.x; j < 3 * nbins; j += 256)
    if (cell[j] != 0ull) atomicAdd(&hist[j], cell[j]);
}

hipError_t launch_calib_accum(const float* conf, const int32_t* pred, const int32_t* target, int B, int K, int nbins,
                              unsigned long long* hist, hipStream_t st) {
  hipLaunchKernelGGL(calib_accum_kernel, dim3((B + 255) / 256), dim3(256), 0, st, conf, pred, target, B, K, nbins, hist);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ temperature scaling
// state [DMF_TEMP_DOUBLES]: beta, nll, g, h, lo, hi, steps taken, reserved.
__global__ void temperature_init_kernel(double* state) {
  const double init[DMF_TEMP_DOUBLES] = {1.0, 0.0, 0.0, 0.0, 0.015625, 64.0, 0.0, 0.0};    // beta = 1 in the bracket [2^-6, 2^6]
  if (threadIdx.x < DMF_TEMP_DOUBLES) state[threadIdx.x] = init[threadIdx.x];
}

hipError_t launch_temperature_init(double* state, hipStream_t st) {
  hipLaunchKernelGGL(temperature_init_kernel, dim3(1), dim3(64), 0, st, state);
  return hipGetLastError();
}

// the 256 lanes' three values -> their sums in pn[0], pg[0], ph[0], by the fixed tree of valid_accum_kernel
__device__ __forceinline__ void tree_sum3(double* pn, double* pg, double* ph, int t) {
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) { pn[t] += pn[t + w]; pg[t] += pg[t + w]; ph[t] += ph[t + w]; }
    __syncthreads();
  }
}

// Launch (a): one row per lane, in double.  With d_c = l_c - m, Z = sum exp(beta d_c), p_c = exp(beta d_c) / Z:
//   nll_i = ln Z - beta d_y        g_i = sum p_c d_c - d_y        h_i = sum p_c d_c^2 - (sum p_c d_c)^2
// A row whose label lies outside [0, K) adds nothing and indexes nothing.  partial [grid][3] <- the workgroup's three sums.
__global__ __launch_bounds__(256) void temperature_rows_kernel(const float* __restrict__ logits, const int32_t* __restrict__ labels,
                                                               int N, int K, const double* __restrict__ state,
                                                               double* __restrict__ partial) {
  __shared__ double pn[256], pg[256], ph[256];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * 256 + t;
  const double beta = state[0];
  double nll = 0.0, g = 0.0, h = 0.0;
  const int y = i < N ? labels[i] : -1;
  if (y >= 0 && y < K) {
    const float* row = logits + (size_t)i * K;
    float m = row[0];
    for (int c = 1; c < K; ++c) m = fmaxf(m, row[c]);
    double Z = 0.0, A = 0.0, Q = 0.0;
    for (int c = 0; c < K; ++c) {
      const double d = (double)row[c] - (double)m;
      const double e = exp(beta * d);
      Z += e; A += e * d; Q += e * d * d;
    }
    const double dy = (double)row[y] - (double)m;
    const double mean = A / Z;
    nll = log(Z) - beta * dy;
    g = mean - dy;
    h = Q / Z - mean * mean;
  }
  pn[t] = nll; pg[t] = g; ph[t] = h;
  tree_sum3(pn, pg, ph, t);
  if (t == 0) {
    partial[3 * (size_t)blockIdx.x] = pn[0];
    partial[3 * (size_t)blockIdx.x + 1] = pg[0];
    partial[3 * (size_t)blockIdx.x + 2] = ph[0];
  }
}

// Launch (b), ONE workgroup: lane t adds partials t, t + 256, ... in index order, then the tree (valid_accum_kernel's order);
// lane 0 stores nll, g, h and, with `update`, takes the safeguarded Newton step: the sign of g moves one end of the bracket
// to beta; the Newton candidate beta - g / h is taken if h > 0 and it is finite and strictly inside (lo, hi), else
// sqrt(lo hi).  The NLL is convex in beta, so the bracket always holds the minimiser (or the end it was started with).
__global__ __launch_bounds__(256) void temperature_final_kernel(const double* __restrict__ partial, int nblk, double* state, int update) {
  __shared__ double pn[256], pg[256], ph[256];
  const int t = threadIdx.x;
  double nll = 0.0, g = 0.0, h = 0.0;
  for (int b = t; b < nblk; b += 256) {
    nll += partial[3 * (size_t)b]; g += partial[3 * (size_t)b + 1]; h += partial[3 * (size_t)b + 2];
  }
  pn[t] = nll; pg[t] = g; ph[t] = h;
  tree_sum3(pn, pg, ph, t);
  if (t != 0) return;
  nll = pn[0]; g = pg[0]; h = ph[0];
  state[1] = nll; state[2] = g; state[3] = h;
  if (!update) return;
  const double beta = state[0];
  double lo = state[4], hi = state[5];
  if (g > 0.0) hi = beta; else lo = beta;
  double cand = beta - g / h;
  if (!(h > 0.0) || !isfinite(cand) || !(cand > lo && cand < hi)) cand = sqrt(lo * hi);
  state[0] = cand; state[4] = lo; state[5] = hi; state[6] += 1.0;
}

hipError_t launch_temperature_step(const float* logits, const int32_t* labels, int N, int K, double* state, double* partial,
                                   int update, hipStream_t st) {
  const int nblk = (N + 255) / 256;
  if (nblk > 0) {
    hipLaunchKernelGGL(temperature_rows_kernel, dim3(nblk), dim3(256), 0, st, logits, labels, N, K, state, partial);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL(temperature_final_kernel, dim3(1), dim3(256), 0, st, partial, nblk, state, update);
  return hipGetLastError();
}

}  // namespace dmf
