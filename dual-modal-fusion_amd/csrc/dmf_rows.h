// dmf_rows.h — the row group: what softmax_stats_kernel, prob_scatter_kernel and logits_mean_kernel share.
// A group of L = next power of two >= K lanes holds one row of logits [B, K] (rows are not 16-byte aligned when K % 4 != 0: one
// 4-byte load per lane, and a wave of 64 / L consecutive rows still reads one contiguous span); a workgroup of 256 threads
// holds 256 / L rows.  Lanes c >= K and the lanes of rows >= B hold -inf; they take part in every shuffle and store nothing.
// All cross-lane steps are xor butterflies inside the group: both partners of a step form the same bits (a + b == b + a; the
// (value, index) order is total), so every lane of a group ends with the group's result, in an order that depends on L alone.
// The kernels form the softmax terms through row_softmax and nothing else: that is what makes prob[pred] the bits of conf.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

namespace dmf {

// this lane's column, and its row (past B in the last workgroup's tail)
template <int L> __device__ __forceinline__ int row_column() { return threadIdx.x % L; }
template <int L> __device__ __forceinline__ int64_t row_index() { return (int64_t)blockIdx.x * (256 / L) + threadIdx.x / L; }

// One pass of the butterfly, off = L / 2 ... 1: step(other), where other(v) is the partner lane's v.  A step that combines
// several values keeps them in one pass (softmax_stats_kernel's three).
template <int L, typename F> __device__ __forceinline__ void row_butterfly(F&& step) {
#pragma unroll
  for (int off = L / 2; off > 0; off >>= 1) step([off](auto v) { return __shfl_xor(v, off, 64); });
}

// (m, first) <- the row maximum with its FIRST index: the value decides, then the lower index (dmf_forward's rule)
template <int L> __device__ __forceinline__ void row_argmax_first(float& m, int& first) {
  row_butterfly<L>([&](auto other) {
    const float om = other(m);
    const int oi = other(first);
    if (om > m || (om == m && oi < first)) { m = om; first = oi; }
  });
}

template <int L> __device__ __forceinline__ float row_sum(float v) {
  row_butterfly<L>([&](auto other) { v += other(v); });
  return v;
}

// The softmax terms at beta of the row whose column c holds the logit l: t = (l - m) beta <= 0 (-inf on the lanes past K) and
// e = exp(t).  With Z = the row's sum of e, p_c = e / Z and the confidence p[first] is 1 / Z.
struct RowSoftmax { float m; int first; float t, e; };

template <int L> __device__ __forceinline__ RowSoftmax row_softmax(float l, int c, float beta) {
  RowSoftmax s{l, c, 0.f, 0.f};
  row_argmax_first<L>(s.m, s.first);
  s.t = (l - s.m) * beta;
  s.e = expf(s.t);
  return s;
}

// workgroups that hold B rows in groups of L lanes
template <int L> inline dim3 row_blocks(int B) { return dim3((unsigned)(((int64_t)B + 256 / L - 1) / (256 / L))); }

// f(std::integral_constant<int, L>{}) at the L of K classes: the one ladder of the three launches
template <typename F> auto for_row_lanes(int K, F&& f) {
  if (K <= 1) return f(std::integral_constant<int, 1>{});
  if (K <= 2) return f(std::integral_constant<int, 2>{});
  if (K <= 4) return f(std::integral_constant<int, 4>{});
  if (K <= 8) return f(std::integral_constant<int, 8>{});
  if (K <= 16) return f(std::integral_constant<int, 16>{});
  if (K <= 32) return f(std::integral_constant<int, 32>{});
  return f(std::integral_constant<int, 64>{});
}

}  // namespace dmf
