// dmf_scene.hip — scene preparation on the device: what `function.data_padding` (`to_tensor` + np.pad 'reflect') and the
// float32 / float16 conversions of dmf.engine.Scene do on the host, for a raw scene uploaded in its own dtype:
//   minmax_part_kernel / minmax_final_kernel : global {min, max} of the raw scene, two stages, NaN kept as np.min / np.max keep it
//   scene_prepare_kernel                     : one streaming pass, out[i, j, c] = normalise(raw[ri(i), rj(j), c]) with
//                                              ri(i) = i < H ? i : 2 (H - 1) - i  (numpy 'reflect' / BORDER_REFLECT_101)
// The arithmetic is numpy's for each dtype (function.to_tensor under numpy 2): integer types subtract in the raw integer
// type and divide the two values as float64, float32 stays float32, float64 stays float64; then ONE rounding to fp32 and,
// for an fp16 scene, a second one from fp32 to fp16 — the host path's double rounding, kept on purpose.
// pan2ms_kernel (image_convert/IHS.py) lives here too.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

#include <type_traits>

#include "dmf_kargs.h"

namespace dmf {

constexpr int MM_T = 256;        // threads of a reduction block
constexpr int MM_MAXB = 2048;    // blocks of the first stage at most (grid-stride beyond)

// first-stage partials {min, max} per block, in 8-byte slots that hold any accumulator type.  Library-owned (the entry point
// takes no workspace): two dmf_scene_minmax calls must not run at the same time on different streams.
__device__ double g_mm_part[2 * MM_MAXB];

// the accumulator of a raw type: every integer code fits int32
template <typename T> using mm_acc = typename std::conditional<std::is_integral<T>::value, int32_t, T>::type;

// comparisons that KEEP a NaN (fmin / fmax would drop it): once m is NaN neither test is true again
template <typename A> __device__ __forceinline__ A keep_min(A m, A x) {
  if constexpr (std::is_floating_point<A>::value) return (x < m || x != x) ? x : m;
  else return x < m ? x : m;
}
template <typename A> __device__ __forceinline__ A keep_max(A m, A x) {
  if constexpr (std::is_floating_point<A>::value) return (x > m || x != x) ? x : m;
  else return x > m ? x : m;
}

// {mn, mx} of the block into thread 0: butterfly inside each wavefront, then the four wave results through LDS
template <typename A> __device__ __forceinline__ void block_minmax(A& mn, A& mx) {
  __shared__ A red[2 * (MM_T / 64)];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    mn = keep_min(mn, (A)__shfl_xor(mn, o));
    mx = keep_max(mx, (A)__shfl_xor(mx, o));
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[2 * wave] = mn; red[2 * wave + 1] = mx; }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < MM_T / 64; ++w) { mn = keep_min(mn, red[2 * w]); mx = keep_max(mx, red[2 * w + 1]); }
  }
}

// x[0, n): `head` scalar elements up to the first 16-byte boundary, nvec 16-byte vectors, then the scalar rest
template <typename T>
__global__ __launch_bounds__(MM_T) void minmax_part_kernel(const T* __restrict__ x, int64_t n, int64_t head, int64_t nvec) {
  using A = mm_acc<T>;
  constexpr int V = 16 / (int)sizeof(T);
  const int64_t g = (int64_t)blockIdx.x * MM_T + threadIdx.x, stride = (int64_t)gridDim.x * MM_T;
  A mn = (A)x[0], mx = mn;
  const uint4* xv = reinterpret_cast<const uint4*>(x + head);
  for (int64_t v = g; v < nvec; v += stride) {
    const uint4 q = xv[v];
    T e[V];
    memcpy(e, &q, 16);
#pragma unroll
    for (int k = 0; k < V; ++k) { mn = keep_min(mn, (A)e[k]); mx = keep_max(mx, (A)e[k]); }
  }
  const int64_t body_end = head + nvec * V, loose = head + (n - body_end);      // (fewer than 2 V elements)
  for (int64_t k = g; k < loose; k += stride) {
    const A e = (A)x[k < head ? k : body_end + (k - head)];
    mn = keep_min(mn, e); mx = keep_max(mx, e);
  }
  block_minmax(mn, mx);
  if (threadIdx.x == 0) {
    A* part = reinterpret_cast<A*>(g_mm_part);
    part[2 * blockIdx.x] = mn; part[2 * blockIdx.x + 1] = mx;
  }
}

template <typename T>
__global__ __launch_bounds__(MM_T) void minmax_final_kernel(int nblk, T* __restrict__ out) {
  using A = mm_acc<T>;
  const A* part = reinterpret_cast<const A*>(g_mm_part);
  A mn = part[0], mx = part[1];
  for (int b = threadIdx.x; b < nblk; b += MM_T) { mn = keep_min(mn, part[2 * b]); mx = keep_max(mx, part[2 * b + 1]); }
  block_minmax(mn, mx);
  if (threadIdx.x == 0) { out[0] = (T)mn; out[1] = (T)mx; }
}

template <typename T>
static hipError_t minmax_typed(const void* raw, int64_t n, void* minmax, hipStream_t st) {
  constexpr int V = 16 / (int)sizeof(T);
  const T* x = static_cast<const T*>(raw);
  int64_t head = (int64_t)(((16 - (reinterpret_cast<uintptr_t>(raw) & 15)) & 15) / sizeof(T));
  if (head > n) head = n;
  const int64_t nvec = (n - head) / V;
  int64_t nblk = (nvec + MM_T - 1) / MM_T;
  nblk = nblk < 1 ? 1 : (nblk > MM_MAXB ? MM_MAXB : nblk);
  hipLaunchKernelGGL(minmax_part_kernel<T>, dim3((unsigned)nblk), dim3(MM_T), 0, st, x, n, head, nvec);
  hipLaunchKernelGGL(minmax_final_kernel<T>, dim3(1), dim3(MM_T), 0, st, (int)nblk, static_cast<T*>(minmax));
  return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------ normalise + pad + convert
// numpy's `(image - min_i) / (max_i - min_i)` for the raw type, rounded once to fp32
template <typename T> struct Norm {
  T mn; double den;
  __device__ Norm(T mn_, T mx_) : mn(mn_) {
    using U = typename std::make_unsigned<T>::type;
    den = (double)(T)((U)mx_ - (U)mn_);                      // in the raw integer type (the caller has ruled a wrap out)
  }
  __device__ __forceinline__ float operator()(T x) const {
    using U = typename std::make_unsigned<T>::type;
    return (float)((double)(T)((U)x - (U)mn) / den);
  }
};
template <> struct Norm<float> {
  float mn, den;
  __device__ Norm(float mn_, float mx_) : mn(mn_), den(mx_ - mn_) {}
  __device__ __forceinline__ float operator()(float x) const { return (x - mn) / den; }
};
template <> struct Norm<double> {
  double mn, den;
  __device__ Norm(double mn_, double mx_) : mn(mn_), den(mx_ - mn_) {}
  __device__ __forceinline__ float operator()(double x) const { return (float)((x - mn) / den); }
};

typedef _Float16 half8 __attribute__((ext_vector_type(8)));

// Thread t makes the 16 bytes of output at the 16-byte-aligned address (out - shift) + t * EPT elements: 4 fp32 or 8 fp16,
// flat over [H + pad, W + pad, C], so a piece may straddle pixels and rows.  `shift` (elements) is how far `out` lies past a
// 16-byte boundary (a stream of the stage-2 tall scene starts wherever the one above it ends); the first and the last piece
// may be partial and are stored element by element.  A piece inside the unpadded columns of one row reads EPT consecutive raw
// elements with one load; the others (right padding, row ends) gather element by element.  All offsets are 64-bit.
template <typename T, bool HALF>
__global__ __launch_bounds__(256) void scene_prepare_kernel(ScenePrepArgs a) {
  constexpr int EPT = HALF ? 8 : 4;
  using O = typename std::conditional<HALF, _Float16, float>::type;
  const int64_t e0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * EPT - a.shift;
  const int k0 = e0 < 0 ? (int)-e0 : 0;
  const int k1 = a.n_out - e0 < EPT ? (int)(a.n_out - e0) : EPT;
  if (k1 <= k0) return;
  const T* raw = static_cast<const T*>(a.raw);
  const T* mm = static_cast<const T*>(a.minmax);
  const Norm<T> norm(mm[0], mm[1]);
  // row i and offset r inside the padded row of the first element: one multiply by 1 / row and a correction instead of a
  // 64-bit division (the quotient is below 2^31 and the product exact to far less than one row: off by one at most)
  const int64_t eb = e0 + k0;
  int64_t i = (int64_t)((double)eb * a.inv_row);
  int64_t r = eb - i * a.row;
  while (r < 0) { --i; r += a.row; }
  while (r >= a.row) { ++i; r -= a.row; }
  const int WC = a.W * a.C;
  float v[EPT];
  if (k0 == 0 && k1 == EPT && r + EPT <= WC) {
    const int64_t ri = i < a.H ? i : 2 * (int64_t)(a.H - 1) - i;
    T x[EPT];
    memcpy(x, raw + ri * WC + r, sizeof(x));
#pragma unroll
    for (int k = 0; k < EPT; ++k) v[k] = norm(x[k]);
  } else {
    int j = (int)r / a.C, c = (int)r - j * a.C;
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
      v[k] = 0.f;
      if (k >= k0 && k < k1) {
        const int64_t ri = i < a.H ? i : 2 * (int64_t)(a.H - 1) - i;
        const int64_t rj = j < a.W ? j : 2 * (int64_t)(a.W - 1) - j;
        v[k] = norm(raw[(ri * a.W + rj) * a.C + c]);
        if (++c == a.C) { c = 0; if (++j == a.W + a.pad) { j = 0; ++i; } }
      }
    }
  }
  O* out = static_cast<O*>(a.out) + e0;
  if (k0 == 0 && k1 == EPT) {
    if constexpr (HALF) {
      half8 h;
#pragma unroll
      for (int k = 0; k < 8; ++k) h[k] = (_Float16)v[k];              // round to nearest even, as numpy's astype(float16)
      *reinterpret_cast<half8*>(out) = h;
    } else {
      *reinterpret_cast<float4*>(out) = make_float4(v[0], v[1], v[2], v[3]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < EPT; ++k)
      if (k >= k0 && k < k1) out[k] = (O)v[k];
  }
}

template <typename T>
static hipError_t prepare_typed(const ScenePrepArgs& a, int half, hipStream_t st) {
  const int ept = half ? 8 : 4;
  const int64_t pieces = (a.n_out + a.shift + ept - 1) / ept;
  const dim3 grid((unsigned)((pieces + 255) / 256));
  if (half) hipLaunchKernelGGL((scene_prepare_kernel<T, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((scene_prepare_kernel<T, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

int scene_raw_bytes(int dtype) {
  switch (dtype) {
    case 0: return 1;
    case 1: case 2: return 2;
    case 3: case 4: return 4;
    case 5: return 8;
    default: return 0;
  }
}

hipError_t launch_scene_minmax(const void* raw, int dtype, int64_t n, void* minmax, hipStream_t st) {
  switch (dtype) {
    case 0: return minmax_typed<uint8_t>(raw, n, minmax, st);
    case 1: return minmax_typed<uint16_t>(raw, n, minmax, st);
    case 2: return minmax_typed<int16_t>(raw, n, minmax, st);
    case 3: return minmax_typed<int32_t>(raw, n, minmax, st);
    case 4: return minmax_typed<float>(raw, n, minmax, st);
    case 5: return minmax_typed<double>(raw, n, minmax, st);
    default: return hipErrorInvalidValue;
  }
}

hipError_t launch_scene_prepare(const ScenePrepArgs& a, int dtype, int half, hipStream_t st) {
  switch (dtype) {
    case 0: return prepare_typed<uint8_t>(a, half, st);
    case 1: return prepare_typed<uint16_t>(a, half, st);
    case 2: return prepare_typed<int16_t>(a, half, st);
    case 3: return prepare_typed<int32_t>(a, half, st);
    case 4: return prepare_typed<float>(a, half, st);
    case 5: return prepare_typed<double>(a, half, st);
    default: return hipErrorInvalidValue;
  }
}

// pan2ms (image_convert/IHS.py:14-19): p = 2x2 mean pool of pan; out[:, :, i] = p[i%2::2, i//2::2]
//   => out[h, w, i] = mean(pan[4h + 2(i%2) + {0,1}, 4w + 2(i//2) + {0,1}])
__global__ __launch_bounds__(256) void pan2ms_kernel(const double* pan, int pitch, int H, int W, double* out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)H * W * 4) return;
  const int i = (int)(e & 3);
  const int64_t hw = e >> 2;
  const int h = (int)(hw / W), w = (int)(hw - (int64_t)h * W);
  const int r = 4 * h + 2 * (i % 2), c = 4 * w + 2 * (i / 2);
  const double* p0 = pan + (size_t)r * pitch + c;
  // numpy.mean over a 2x2 block: running sum in row-major order, then / 4
  out[e] = (((p0[0] + p0[1]) + p0[pitch]) + p0[pitch + 1]) / 4.0;
}

hipError_t launch_pan2ms(const double* pan, int pitch, int H, int W, double* out, hipStream_t st) {
  const int64_t n = (int64_t)H * W * 4;
  hipLaunchKernelGGL(pan2ms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, pan, pitch, H, W, out);
  return hipGetLastError();
}

}  // namespace dmf
