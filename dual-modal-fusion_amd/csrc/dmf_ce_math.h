// The arithmetic of the classification criterion (class weights, label smoothing, focal term), stated ONCE for
// the two kernels that evaluate it: ce_loss_kernel (dmf_loss.hip, on the logits of the unit-gradient step) and the criterion
// instance of the attention training kernel (dmf_attention.hip, on the logits of the patch it has just formed).  Both call the
// functions below, so a sample's gradient and value are the same bits on either route.
//
// Lane k of a group of L lanes (16 or 64) holds class k of one sample; lanes k >= K hold z = -inf and w = 0.  Group reductions
// leave the same bits in every lane.  L = 64 reproduces the bits of L = 16 when K <= 16: the 64-lane reductions are the 16-lane
// butterfly followed by steps that add the other rows, whose lanes contribute +0 (or -inf to the maximum) — exact.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

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

// D = sum_j w[y_j] over the N labels `lab` of one global batch, by a 256-thread workgroup (tid = its thread, red = 256 doubles
// of its LDS): strided pass (thread t takes j = t, t + 256, ...), then the fixed tree — an order that depends on nothing but
// the batch, so every workgroup of every launch that sums the same labels holds the same bits.  In double: the value is
// divided by it, and a float32 sum of weights spanning 0.01 ... 50 is already 1e-7 off.  Returned to every thread.
__device__ __forceinline__ double ce_denominator(const int32_t* __restrict__ lab, int N, int K, const float* __restrict__ class_w,
                                                 double* red, int tid) {
  double s = 0.0;
  for (int j = tid; j < N; j += 256) s += class_w != nullptr ? (double)class_w[clamp_label(lab[j], K)] : 1.0;
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int w = 128; w > 0; w >>= 1) {
    if (tid < w) red[tid] += red[tid + w];
    __syncthreads();
  }
  return red[0];
}

// what the value of a sample needs of the quantities its gradient has formed
struct CeTerm {
  float z, mx, wk, wy;
  bool hit, in;
};

// dt_i / dz_k of lane k's class for the sample with label y (clamped): z the lane's logit (-inf for k >= K), wk its class
// weight (0 for k >= K), wsum the group sum of wk (read when kind == 0 and eps != 0).  kind, eps, gamma: dmf_ce_params, uniform.
template <int L>
__device__ __forceinline__ float ce_grad(float z, float wk, float wsum, int k, int y, int K, int kind, float eps, float gamma,
                                         CeTerm& t) {
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
  if (kind == 0) {
    const float c1 = (1.f - eps) * wy;
    g = c1 * d;
    if (eps != 0.f)                                       // gradient of (eps / K) sum_c w_c (-log p_c): (eps / K) (p_k sum_c w_c - w_k)
      g += (eps / (float)K) * (wsum * p - wk);
  } else {
    // dt/dz_c = w_y [gamma p_y q^(gamma - 1) log p_y - q^gamma] ([c == y] - p_c) = w_y A (p_c - [c == y]),
    // A = q^gamma + gamma p_y q^(gamma - 1) (-log p_y); gamma = 0: A = 1, kind 0 with eps = 0 bit for bit
    const float gm = gamma, py = ey / S;
    float pw = 1.f, pw1 = 0.f;                            // q^gamma, q^(gamma - 1) (gamma = 0: the second term is absent)
    if (gm == 1.f) { pw = q; pw1 = 1.f; }
    else if (gm == 2.f) { pw = q * q; pw1 = q; }
    else if (gm != 0.f) { pw = powf(q, gm); pw1 = powf(q, gm - 1.f); }
    const float A = pw + gm * py * pw1 * nlpy;
    g = (wy * A) * d;
  }
  t.z = z; t.mx = mx; t.wk = wk; t.wy = wy; t.hit = hit; t.in = k < K;
  return g;
}

// The value t_i of the same sample, the same bits in every lane of the group.  loss[i] is one float32 per sample and the batch
// loss is their mean, so every rounding made on the way to loss[i] shows in it undiminished; the gradient is compared element by
// element and float32 arithmetic serves it.  The per-sample term is therefore formed in double from the float32 logits and
// weights (a dozen fp64 operations per lane in a section whose time is its latency) and rounded ONCE, when the caller stores
// (float)((double)N * t_i / D).
template <int L>
__device__ __forceinline__ double ce_value(const CeTerm& t, int K, int kind, float eps, float gamma) {
  const double zmd = (double)t.z - (double)t.mx;
  const double ed = t.in ? exp(zmd) : 0.0;
  const double Rd = grp_sum_d<L>(t.hit ? 0.0 : ed), eyd = grp_sum_d<L>(t.hit ? ed : 0.0);
  const double zyd = grp_sum_d<L>(t.hit ? zmd : 0.0);
  const double Sd = eyd + Rd, logSd = log(Sd);
  const double nlpyd = zyd == 0.0 ? log1p(Rd) : logSd - zyd;
  double td;
  if (kind == 0) {
    td = ((1.0 - (double)eps) * (double)t.wy) * nlpyd;
    if (eps != 0.f) td += ((double)eps / (double)K) * grp_sum_d<L>(t.in ? (double)t.wk * (logSd - zmd) : 0.0);
  } else {
    const double qd = Rd / Sd, gmd = (double)gamma;
    const double pwd = gamma == 0.f ? 1.0 : (gamma == 1.f ? qd : (gamma == 2.f ? qd * qd : pow(qd, gmd)));
    td = ((double)t.wy * pwd) * nlpyd;                    // gamma = 0: kind 0 with eps = 0 bit for bit
  }
  return td;
}

}  // namespace dmf
