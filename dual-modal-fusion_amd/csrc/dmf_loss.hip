// dmf_loss.hip — per-sample classification losses on the logits [bs_r, K] of the unit-gradient step:
//   kind 0  cross-entropy with class weights w and label smoothing eps — torch.nn.functional.cross_entropy(weight=, label_smoothing=,
//           reduction='mean'):  t_i = (1 - eps) w[y] (-log p_y) + (eps / K) sum_c w[c] (-log p_c)
//   kind 1  focal loss with class weights:  t_i = w[y] (1 - p_y)^gamma (-log p_y)
// batch loss = sum_i t_i / D with D = sum_j w[y_j] over the GLOBAL batch (all ranks); loss[i] = N t_i / D (N = global batch), so
// that the mean over a rank's rows, averaged over the ranks, is the batch loss; dlogits = grad_scale * scale / D * dt_i/dz.
//
// Element-parallel like qua_e*_kernel (dmf_qua.hip): lane k of a group holds class k of one sample — a 16-lane DPP row when
// K <= 16 (16 samples per 256-thread workgroup), a whole wave otherwise (4 samples) — and row max, sum exp and the weighted sums
// are lane reductions whose result is the same bits in every lane.  ONE launch: the denominator depends on the labels only, so
// every workgroup sums w[label] of the whole global batch itself, in an order (thread t takes j = t, t + 256, ...; then a fixed
// LDS tree) that depends on nothing but the global batch — every workgroup of every rank holds the same bits, and a rank's rows
// are bit for bit the rows the same samples get in a one-rank call on the whole batch.  No atomics, plain vector stores.
// The gradient is float32 arithmetic; the per-sample VALUE and D are formed in double and rounded once at the store (see there).
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dmf_kargs.h"
#include "dmf_lanes.h"

namespace dmf {

#define DMF_DPP_MAX(v, CTRL) \
  fmaxf((v), __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, (v)), __builtin_bit_cast(int, (v)), (CTRL), 0xF, 0xF, false)))
__device__ __forceinline__ float max16(float v) {         // over the 16 lanes sharing lane>>4 (the butterfly of sum16)
  v = DMF_DPP_MAX(v, 0xB1); v = DMF_DPP_MAX(v, 0x4E); v = DMF_DPP_MAX(v, 0x141); v = DMF_DPP_MAX(v, 0x140);
  return v;
}
#undef DMF_DPP_MAX
__device__ __forceinline__ float wave_max_dpp(float v) {  // all 64 lanes (the row / half swaps of wave_sum_dpp)
  v = max16(v);
  unsigned u = __builtin_bit_cast(unsigned, v);
  auto r = __builtin_amdgcn_permlane16_swap(u, u, false, false);
  v = fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
  u = __builtin_bit_cast(unsigned, v);
  r = __builtin_amdgcn_permlane32_swap(u, u, false, false);
  return fmaxf(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}
template <int L> __device__ __forceinline__ float grp_sum(float v) { return L == 16 ? sum16(v) : wave_sum_dpp(v); }
template <int L> __device__ __forceinline__ double grp_sum_d(double v) {   // the same bits in every lane of the group
#pragma unroll
  for (int o = L / 2; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
template <int L> __device__ __forceinline__ float grp_max(float v) { return L == 16 ? max16(v) : wave_max_dpp(v); }

// the callers have checked the labels (_check_labels); a bad one must still not index class_w out of bounds (as dmf_forward_ce)
__device__ __forceinline__ int clamp_label(int y, int K) { return y < 0 ? 0 : (y >= K ? K - 1 : y); }

// L lanes per sample (16 or 64); every thread stays alive to the end (the lane reductions read all lanes of a group): samples
// beyond bs_r recompute the last row and store nothing.
template <int L>
__global__ __launch_bounds__(256) void ce_loss_kernel(const CeArgs a) {
  __shared__ double red[256];
  const int tid = threadIdx.x, K = a.K, N = a.ranks * a.bs_r;
  const int cur = a.cursor != nullptr ? *a.cursor : 0;
  const int32_t* lab = a.labels + (size_t)cur * N;

  // D = sum_j w[y_j] over the global batch: strided pass, then the fixed tree (the same bits in every workgroup of every rank).
  // In double: the value is divided by it, and a float32 sum of weights spanning 0.01 ... 50 is already 1e-7 off.
  double s = 0.0;
  for (int j = tid; j < N; j += 256) s += a.class_w != nullptr ? (double)a.class_w[clamp_label(lab[j], K)] : 1.0;
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  const double Dd = red[0];
  const float D = (float)Dd;

  const int i = blockIdx.x * (256 / L) + tid / L, k = tid % L;
  const bool row = i < a.bs_r, on = row && k < K;
  const int ic = row ? i : a.bs_r - 1;
  const int y = clamp_label(lab[(size_t)a.rank * a.bs_r + ic], K);
  const float z = k < K ? a.logits[(size_t)ic * K + k] : -INFINITY;
  const float wk = k < K ? (a.class_w != nullptr ? a.class_w[k] : 1.f) : 0.f;
  const bool hit = k == y;
  const float mx = grp_max<L>(z);
  const float zm = z - mx;
  const float e = k < K ? expf(zm) : 0.f;
  // the label's own lane carries z_y, e_y, w_y to the group (sums with one non-zero term: exact); 1 - p_y is formed as
  // sum_{c != y} p_c = R / S, which stays accurate when p_y -> 1
  const float R = grp_sum<L>(hit ? 0.f : e);
  const float ey = grp_sum<L>(hit ? e : 0.f);
  const float zy = grp_sum<L>(hit ? zm : 0.f);
  const float wy = grp_sum<L>(hit ? wk : 0.f);
  const float S = ey + R;
  const float logS = logf(S);
  const float p = e / S, q = R / S;
  // -log p_y; where the label holds the row maximum (e_y = 1, S = 1 + R) log(1 + R) keeps the digits that S has rounded away
  const float nlpy = zy == 0.f ? log1pf(R) : logS - zy;
  const float d = hit ? -q : p;                           // p_c - [c == y]
  float g;                                                // dt_i / dz_k
  if (a.kind == 0) {
    const float c1 = (1.f - a.eps) * wy;
    g = c1 * d;
    if (a.eps != 0.f) {                                   // gradient of (eps / K) sum_c w_c (-log p_c): (eps / K) (p_k sum_c w_c - w_k)
      const float wsum = grp_sum<L>(wk);
      g += (a.eps / (float)K) * (wsum * p - wk);
    }
  } else {
    // dt/dz_c = w_y [gamma p_y q^(gamma - 1) log p_y - q^gamma] ([c == y] - p_c) = w_y A (p_c - [c == y]),
    // A = q^gamma + gamma p_y q^(gamma - 1) (-log p_y); gamma = 0: A = 1, kind 0 with eps = 0 bit for bit
    const float gm = a.gamma, py = ey / S;
    float pw = 1.f, pw1 = 0.f;                            // q^gamma, q^(gamma - 1) (gamma = 0: the second term is absent)
    if (gm == 1.f) { pw = q; pw1 = 1.f; }
    else if (gm == 2.f) { pw = q * q; pw1 = q; }
    else if (gm != 0.f) { pw = powf(q, gm); pw1 = powf(q, gm - 1.f); }
    const float A = pw + gm * py * pw1 * nlpy;
    g = (wy * A) * d;
  }
  if (a.dlogits != nullptr && on) {
    const float gs = a.grad_scale * (a.scaler != nullptr ? a.scaler[0] : 1.f);
    a.dlogits[(size_t)i * K + k] = g * (gs / D);
  }
  if (a.loss == nullptr) return;                          // (uniform)

  // The value.  loss[i] is one float32 per sample and the batch loss is their mean, so every rounding made on the way to
  // loss[i] shows in it undiminished; the gradient above is compared element by element and float32 arithmetic serves it.  The
  // per-sample term is therefore formed in double from the float32 logits and weights (a dozen fp64 operations per lane in a
  // launch whose time is its latency) and rounded ONCE, when it is stored.
  const double zmd = (double)z - (double)mx;
  const double ed = k < K ? exp(zmd) : 0.0;
  const double Rd = grp_sum_d<L>(hit ? 0.0 : ed), eyd = grp_sum_d<L>(hit ? ed : 0.0);
  const double zyd = grp_sum_d<L>(hit ? zmd : 0.0);
  const double Sd = eyd + Rd, logSd = log(Sd);
  const double nlpyd = zyd == 0.0 ? log1p(Rd) : logSd - zyd;
  double td;
  if (a.kind == 0) {
    td = ((1.0 - (double)a.eps) * (double)wy) * nlpyd;
    if (a.eps != 0.f) td += ((double)a.eps / (double)K) * grp_sum_d<L>(k < K ? (double)wk * (logSd - zmd) : 0.0);
  } else {
    const double qd = Rd / Sd, gmd = (double)a.gamma;
    const double pwd = a.gamma == 0.f ? 1.0 : (a.gamma == 1.f ? qd : (a.gamma == 2.f ? qd * qd : pow(qd, gmd)));
    td = ((double)wy * pwd) * nlpyd;                      // gamma = 0: kind 0 with eps = 0 bit for bit
  }
  if (row && k == 0) a.loss[i] = (float)((double)N * td / Dd);
}

hipError_t launch_ce_loss(const CeArgs& a, hipStream_t st) {
  if (a.K <= 16) hipLaunchKernelGGL(ce_loss_kernel<16>, dim3((a.bs_r + 15) / 16), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ce_loss_kernel<64>, dim3((a.bs_r + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmf
