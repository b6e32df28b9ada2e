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

#include "dmf_ce_math.h"
#include "dmf_kargs.h"

namespace dmf {

// (the lane reductions, the denominator and the per-sample arithmetic: dmf_ce_math.h, shared with the attention training kernel)

// L lanes per sample (16 or 64); every thread stays alive to the end (the lane reductions read all lanes of a group): samples
// beyond bs_r recompute the last row and store nothing.
template <int L>
__global__ __launch_bounds__(256) void ce_loss_kernel(const CeArgs a) {
  __shared__ double red[256];
  const int tid = threadIdx.x, K = a.K, N = a.ranks * a.bs_r;
  const int cur = a.cursor != nullptr ? *a.cursor : 0;
  const int32_t* lab = a.labels + (size_t)cur * N;

  // D = sum_j w[y_j] over the global batch (the same bits in every workgroup of every rank)
  const double Dd = ce_denominator(lab, N, K, a.class_w, red, tid);
  const float D = (float)Dd;

  const int i = blockIdx.x * (256 / L) + tid / L, k = tid % L;
  const bool row = i < a.bs_r, on = row && k < K;
  const int ic = row ? i : a.bs_r - 1;
  const int y = clamp_label(lab[(size_t)a.rank * a.bs_r + ic], K);
  const float z = k < K ? a.logits[(size_t)ic * K + k] : -INFINITY;
  const float wk = k < K ? (a.class_w != nullptr ? a.class_w[k] : 1.f) : 0.f;
  const float wsum = a.kind == 0 && a.eps != 0.f ? grp_sum<L>(wk) : 0.f;   // (uniform)
  CeTerm t;
  const float g = ce_grad<L>(z, wk, wsum, k, y, K, a.kind, a.eps, a.gamma, t);
  if (a.dlogits != nullptr && on) {
    const float gs = a.grad_scale * (a.scaler != nullptr ? a.scaler[0] : 1.f);
    a.dlogits[(size_t)i * K + k] = g * (gs / D);
  }
  if (a.loss == nullptr) return;                          // (uniform)
  const double td = ce_value<L>(t, K, a.kind, a.eps, a.gamma);   // in double, rounded once at the store (ce_value)
  if (row && k == 0) a.loss[i] = (float)((double)N * td / Dd);
}

// denom[r] = the D of plan row r (N labels each), in ce_loss_kernel's own order: one workgroup per row
__global__ __launch_bounds__(256) void ce_denominators_kernel(const int32_t* __restrict__ labels, int N, int K,
                                                              const float* __restrict__ class_w, double* __restrict__ denom) {
  __shared__ double red[256];
  const double Dd = ce_denominator(labels + (size_t)blockIdx.x * N, N, K, class_w, red, threadIdx.x);
  if (threadIdx.x == 0) denom[blockIdx.x] = Dd;
}

hipError_t launch_ce_denominators(const int32_t* labels, int N, int rows, int K, const float* class_w, double* denom, hipStream_t st) {
  hipLaunchKernelGGL(ce_denominators_kernel, dim3(rows), dim3(256), 0, st, labels, N, K, class_w, denom);
  return hipGetLastError();
}

hipError_t launch_ce_loss(const CeArgs& a, hipStream_t st) {
  if (a.K <= 16) hipLaunchKernelGGL(ce_loss_kernel<16>, dim3((a.bs_r + 15) / 16), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(ce_loss_kernel<64>, dim3((a.bs_r + 3) / 4), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dmf
