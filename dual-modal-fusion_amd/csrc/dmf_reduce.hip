// dmf_reduce.hip — the batch-level launches behind the patch and attention kernels: the slab / outer-product gradient
// reduction with its fused Adam (grad_reduce_kernel), the ONE optimiser kernel on a flat gradient (optim_step_kernel: Adam, AdamW,
// SGD, RMSprop, with or without weight decay, gradient-norm clipping and the loss scaler's step end; every dmf_*_step entry
// point and dmf_unscale_adam launch it), the loss scaler's unscale + check (unscale_check_kernel) and the small xgmi
// all-reduce.  dmf_capi.hip validates and calls the launch_* functions at the end of this file.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "dmf_kargs.h"
#include "dmf_lanes.h"
#include "dmf_xgmi.h"

namespace dmf {

// bias corrections from a device-resident step count, in double like torch's host-side scalars
__device__ __forceinline__ void bias_corrections(int step, float b1, float b2, float& bc1, float& bc2_sqrt) {
  bc1 = (float)(1.0 - pow((double)b1, (double)step));
  bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
}

__device__ __forceinline__ void adam_update(float* theta, float* m, float* v, int64_t p, float g,
                                            float lr, float b1, float b2, float eps, float bc1, float bc2_sqrt) {
  // torch.optim.Adam single-tensor path: exp_avg.lerp_(grad, 1-b1); exp_avg_sq.mul_(b2).addcmul_(g, g, 1-b2);
  // denom = sqrt(v)/sqrt(bc2) + eps; p -= (lr/bc1) * m / denom
  const float mo = m[p], vo = v[p];
  const float mn = mo + (g - mo) * (1.f - b1);
  const float vn = vo * b2 + (1.f - b2) * g * g;
  m[p] = mn;
  v[p] = vn;
  const float denom = sqrtf(vn) / bc2_sqrt + eps;
  theta[p] -= (lr / bc1) * (mn / denom);
}

// ------------------------------------------------------------------------------ the reference's other two optimisers
// torch.optim.SGD(lr, momentum) (dampening 0, no Nesterov): buf = g on the first step, else m buf + g; p -= lr buf.
// torch.optim.RMSprop(lr, alpha) (eps 1e-8, momentum 0, not centred): sq = alpha sq + (1 - alpha) g g;
// p -= lr g / (sqrt(sq) + eps).   (utils/utils.py:13-16)
__device__ __forceinline__ void sgd_update(float* theta, float* buf, int64_t p, float g, float lr, float momentum, int st) {
  float b = g;
  if (momentum != 0.f) { b = st <= 1 ? g : momentum * buf[p] + g; buf[p] = b; }
  theta[p] -= lr * b;
}

__device__ __forceinline__ void rmsprop_update(float* theta, float* sq, int64_t p, float g, float lr, float alpha, float eps) {
  const float s = alpha * sq[p] + (1.f - alpha) * g * g;
  sq[p] = s;
  theta[p] -= lr * (g / (sqrtf(s) + eps));
}

// ------------------------------------------------------------------------------ the averaged copy of the weights
// torch.optim.swa_utils.AveragedModel on the flat vector: st = the 1-based count of the optimiser step just taken;
// st <= start copies theta through (st == start is AveragedModel's first update_parameters), later steps lerp towards it
// with w = 1 - decay (DMF_AVG_EMA, formed by the host) or 1 / (n + 1), n = st - start (DMF_AVG_MEAN: torch's
// 1 / (num_averaged + 1)).  lerp is torch's, its fused steps written out (contraction off) as adam_apply's are.
__device__ __forceinline__ float avg_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
  const float d = b - a;
  return fabsf(w) < 0.5f ? fmaf(w, d, a) : fmaf(-(1.f - w), d, b);
}

__device__ __forceinline__ float avg_rule(int kind, float w_ema, int start, int st, float avg_old, float th_new) {
  if (st <= start) return th_new;
  const float w = kind == DMF_AVG_MEAN ? 1.f / (float)(st - start + 1) : w_ema;
  return avg_lerp(avg_old, th_new, w);
}

// The stand-alone form (dmf_weight_average): the routes without a fused form, and what the fused forms are compared against.
__global__ __launch_bounds__(256) void weight_average_kernel(const AvgArgs av, const float* __restrict__ theta, int64_t n, int step,
                                                             const int32_t* step_dev) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int st = step_dev != nullptr ? *step_dev : step;
  if (p >= n) return;
  av.avg[p] = avg_rule(av.kind, av.w, av.start, st, av.avg[p], theta[p]);
}

// ---- the reduce launch.  What bounds it (tools/reduce_phase_profile.py, stamps of round 3): ONE CU takes in only ~15 bytes
// per clock from the Infinity Cache (about 64 lines in flight x ~550 cycles), and the 2.2 MB the patch kernel left behind are
// nowhere else.  The first forms (16 or 64 parameters per block, 64-byte pieces of 7-KB rows, 64 KB fetched per block) spent
// 4.5 K of their 6.8 K cycles waiting for that; so the producers now lay their results out for THIS kernel (dmf_shapes.h):
//   * conv slabs piece-major: one block per 16 parameters reads rows x 64 contiguous bytes (16 KB at batch 256) — a lane
//     holds one 16-byte piece of up to 4 rows, rows are summed per lane, then over the 16 row lanes by DPP and the row /
//     half swaps, then over the 4 waves through LDS: a fixed order;
//   * fc1.weight / fc2.weight = dh^T z / dl^T h: one 8x8 output tile per block — 2 x 8 KB of contiguous strip-major head
//     vectors at batch 256 (a 16x16 tile needs 2 x 16 KB: twice the wait).  It still runs on the fp32 matrix cores
//     (v_mfma_f32_16x16x4_f32: bit for bit a k-ordered fmaf chain) with the two HALVES of the batch packed into one
//     instruction: rows 0-7 / columns 0-7 carry the first half, rows 8-15 / columns 8-15 the second, the two diagonal 8x8
//     blocks of the result are the two partial tiles (the off-diagonal blocks are discarded); wave w carries a quarter of each
//     half in two accumulators.  The tiles of the first column also sum their dh / dl strip: fc1.bias / fc2.bias;
//   * attention slabs keep the row-major form (64 parameters per block): 15.7 MB per step, bound by the chip, not the CU;
//   * ADAM's bias corrections: b^step by repeated squaring in double on two lanes of a fifth wave (beta1 / beta2 side by
//     side) beside the gradient loads, instead of two calls of the general pow() on one lane in front of the barrier.
// Block order: fc tiles first (the longest chains), then slabs, the bookkeeping block last.
typedef float f32x4_t __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double powi_double(double b, int n) {   // b^n, n >= 0, by squaring (relative error ~ 2 log2(n) ulp)
  double r = 1.0;
  while (n > 0) {
    if (n & 1) r *= b;
    b *= b;
    n >>= 1;
  }
  return r;
}

// the fixed combine of 16 chunk partials ((0+8)+(4+12)) + ... (attention slabs)
__device__ __forceinline__ float tree16(float (&t)[16]) {
#pragma unroll
  for (int w = 8; w > 0; w >>= 1)
#pragma unroll
    for (int i = 0; i < w; ++i) t[i] += t[i + w];
  return t[0];
}

// One 8 x 8 tile of out[m][n] = sum_b U[b][m0 + m] * W[b][n0 + n] (U, W strip-major: hv_index; m0, n0 multiples of 8).
// MFMA row / column q < 8 works on the patches [0, Bh), q >= 8 on [Bh, B); wave w takes a quarter of each half's k-steps (4
// patches each), 8 steps per batch.  issue(): the 16 loads of one batch; consume(): its 8 MFMAs (two accumulators) and the
// running sum of the U operand (the bias gradient).  Rows >= mlim read as zero.  Threads 0..255.
struct FcTile {
  const float* up; const float* wp;
  int bbase, blim, kk, s1, sb_;
  bool mok;
  f32x4_t acc0, acc1;
  float bs;
  float av[8], bv[8];
  __device__ __forceinline__ int init(const float* U, int m0, int mlim, const float* W, int n0, int B) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q8 = lane & 7, half = (lane >> 3) & 1;
    kk = lane >> 4;
    mok = m0 + q8 < mlim;
    const int Bh = (((B + 1) >> 1) + 3) & ~3;                 // first half: a multiple of 4 patches
    bbase = half ? Bh : 0; blim = half ? B : min(Bh, B);
    up = U + (size_t)(m0 >> 3) * B * 8 + q8;                  // strip m0 / 8: element (b, m) at b * 8 + m
    wp = W + (size_t)(n0 >> 3) * B * 8 + q8;
    const int nk = Bh / 4, nkw = (nk + 3) / 4;                // k-steps per half: all, per wave
    const int s0 = w * nkw;
    s1 = min(nk, s0 + nkw);
    acc0 = (f32x4_t){0.f, 0.f, 0.f, 0.f}; acc1 = acc0; bs = 0.f;
    return s0;
  }
  // (loads are UNCONDITIONAL, from a clamped patch index, and masked in consume(): a load under a lane condition becomes a
  // branch around it, and the compiler then waits for the loads of one branch before it enters the next)
  __device__ __forceinline__ void issue(int sb) {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int b = min(bbase + 4 * (sb + q) + kk, blim - 1);
      av[q] = up[(size_t)(b < 0 ? 0 : b) * 8];
      bv[q] = wp[(size_t)(b < 0 ? 0 : b) * 8];
    }
    sb_ = sb;
  }
  __device__ __forceinline__ void consume() {
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const bool in = sb_ + q < s1 && bbase + 4 * (sb_ + q) + kk < blim;
      av[q] = (in && mok) ? av[q] : 0.f;
      bv[q] = in ? bv[q] : 0.f;
    }
#pragma unroll
    for (int q = 0; q < 8; q += 2) {
      acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q], bv[q], acc0, 0, 0, 0);
      acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(av[q + 1], bv[q + 1], acc1, 0, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < 8; ++q) bs += av[q];
  }
};

// (adam_update's arithmetic, stated again on purpose: through a shared helper the reduce kernel gets another register
// allocation and six more instructions)
struct ReduceTail { float* scaler; float* grad; float lr, b1, b2, eps; };   // the scalars of the tail, fetched at kernel entry
// Returns the theta it stored (th0 without one): the averaging instances go on from it without reading it back.
__device__ __forceinline__ float adam_apply(const ReduceTail& a, float* theta, float* m, float* v, int64_t p, float g, float th0,
                                            float m_0, float v_0, const float* bcs) {
  if (a.scaler != nullptr) {                         // unscale_ + the found_inf check of GradScaler, in the reduce
    g *= 1.f / a.scaler[0];
    if (!isfinite(g)) a.scaler[2] = 1.f;             // (every writer stores the same value)
  }
  if (a.grad != nullptr) a.grad[p] = g;
  if (theta != nullptr) {
    // The fused and unfused steps are WRITTEN OUT (and contraction is off): left to the compiler, which products it fuses into
    // the following addition changes with the code around this function — m's update came out as multiply + add once the
    // constants were fetched early, one ulp away from every earlier build.  These are the forms the kernel has always had.
#pragma clang fp contract(off)
    const float mn = fmaf(g - m_0, 1.f - a.b1, m_0);
    const float vn = v_0 * a.b2 + ((1.f - a.b2) * g) * g;
    m[p] = mn;
    v[p] = vn;
    th0 = fmaf(-(a.lr / bcs[0]), mn / (sqrtf(vn) / bcs[1] + a.eps), th0);
    theta[p] = th0;
  }
  return th0;
}

// Diagnostic build only (-DDMF_STAMPS, tools/reduce_phase_profile.py): clock stamps of every wave of the reduce launch in
// scalar registers, dumped by lane 0 right before the wave ends.  [block][5 waves][8]: 0 entry, 2 kernel arguments in registers, 1 role known, 3 partials
// written (loads landed), 4 behind the barrier, 5 stores issued, 6 end; 7 s_memrealtime at entry.
#ifdef DMF_STAMPS
__device__ unsigned long long* g_rstamps = nullptr;
#define RSTAMP_DECL unsigned long long rst_[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull}
#define RSTAMP(i) do { __builtin_amdgcn_sched_barrier(0); asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rst_[i]) :: "memory"); __builtin_amdgcn_sched_barrier(0); } while (0)
#define RSTAMP_RT(i) do { asm volatile("s_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(rst_[i])); } while (0)
#define RSTAMP_DUMP() do { asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); RSTAMP(6); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); \
    if ((threadIdx.x & 63) == 0 && g_rstamps != nullptr) { _Pragma("unroll") for (int i_ = 0; i_ < 8; ++i_) \
      g_rstamps[((size_t)blockIdx.x * 5 + (threadIdx.x >> 6)) * 8 + i_] = rst_[i_]; } } while (0)
#else
#define RSTAMP_DECL do { } while (0)
#define RSTAMP(i) do { } while (0)
#define RSTAMP_RT(i) do { } while (0)
#define RSTAMP_DUMP() do { } while (0)
#endif

typedef const int32_t __attribute__((address_space(4)))* const_i32;   // memory that no launch writes while it is read
typedef const float __attribute__((address_space(4)))* const_f32;

// 320 threads: waves 0-3 reduce, wave 4 only forms ADAM's bias corrections (beside the other waves' gradient loads).
// The first ten arguments (14 dwords) are everything a block needs to find its role, ISSUE its gradient loads and ISSUE the
// loads of the ADAM state of the parameters it owns; they are plain scalars in front of the argument struct so that the
// compiler's kernarg preload (-mllvm -amdgpu-kernarg-preload-count, build.py) puts them into scalar registers at wave launch:
// a kernel argument fetched by the wave itself arrives ~1.0 K cycles after wave entry (stamps), and a load that waits for it
// starts its own cold round trip only then.  The slab rows and head vectors are addressed from the ONE workspace pointer
// (their offsets follow from w3, w4 and B: reduce_words_unpack, dmf_shapes.h), which leaves room for theta / m / v.
// w0 = nFc1 | t1n << 16, w1 = nFc2 | t2n << 16, w2 = nConv | nAttn << 16 (blocks per kind, tiles per row).
// SCHED (the second instance): lr, beta1 and beta2 come from the row of a.hp that belongs to this step instead of
// the launch arguments; the row index and the 16-byte row are fetched where the tail's other scalars are, and wave 4 forms
// b^step from the row's betas.  Nothing else differs, and the default instance takes the arguments it has always taken.
// AVG (the third and fourth instances): every lane that owns a parameter also keeps its element of a.av.avg by
// avg_rule, from the theta it has just written.  The avg pointer and words are fetched where the tail's scalars are, the element
// is requested right behind them (unconditional, clamped index, like the state loads), and the step count is the one the
// SCHED instance reads.  AVG takes ReduceAvgArgs with or without SCHED; there is no AVG form of the xgmi exchange.
template <bool SCHED, bool AVG>
__global__ __launch_bounds__(320) void grad_reduce_kernel(const float* __restrict__ ws, float* theta, float* m, float* v, int w0, int w1,
                                                          int w2, int w3, int w4, int B,
                                                          const std::conditional_t<AVG, ReduceAvgArgs, std::conditional_t<SCHED, ReduceSchedArgs, ReduceArgs>> a) {
  __shared__ float vbuf[4][256];        // tile partials of the four waves / [16 chunks][64] attention-slab partials / [4][16] piece partials
  __shared__ float bbuf[4][16];         // bias partials of the four waves
  __shared__ float bcs[2];
  const int tid = threadIdx.x;
  int blk = blockIdx.x;
  RSTAMP_DECL;
  RSTAMP_RT(7);
  RSTAMP(0);
  const int nFc1 = w0 & 0xffff, t1n = w0 >> 16, nFc2 = w1 & 0xffff, t2n = w1 >> 16, nConv = w2 & 0xffff, nAttn = w2 >> 16;
  const int nTotal = nFc1 + nFc2 + nConv + nAttn + 1;
  const int nblk = B < MAX_BLOCKS ? B : MAX_BLOCKS;  // slab rows: the patch kernel's grid
  const ReduceGeom G = reduce_words_unpack(w3, w4, B);
  const float* __restrict__ slab = ws;
  const float* __restrict__ z = ws + G.z;
  const float* __restrict__ h = ws + G.h;
  const float* __restrict__ dh = ws + G.dh;
  const float* __restrict__ dl = ws + G.dl;
  if (blk == nTotal - 1) {                           // bookkeeping block
    const int cur = a.cursor_dev != nullptr ? *a.cursor_dev : 0;
    if (a.loss != nullptr && a.loss_hist != nullptr) {
      float s = 0.f;
      float* red = &vbuf[0][0];
      if (tid < 256) {
        for (int b = tid; b < a.B; b += 256) s += a.loss[b];
        red[tid] = s;
      }
      __syncthreads();
      for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
      }
      if (tid == 0) a.loss_hist[cur] = red[0] / (float)a.B;
    }
    if (tid == 0 && a.cursor_dev != nullptr) *a.cursor_dev = cur + 1;
    return;
  }
  int kind, sub;                                     // 0 fc1.weight tile, 1 fc2.weight tile, 2 conv slab piece, 3 attention slab
  if (blk < nFc1) { kind = 0; sub = blk; }
  else if ((blk -= nFc1) < nFc2) { kind = 1; sub = blk; }
  else if ((blk -= nFc2) < nConv) { kind = 2; sub = blk; }
  else { kind = 3; sub = blk - nConv; }
  // ---- the first batch of gradient loads goes out before anything else is looked at
  int m0 = 0, n0 = 0;
  FcTile ft;
  int sb = 0;
  float4 cv[4];
  const int lane = tid & 63, wv = tid >> 6, c4 = lane & 3, r16 = lane >> 2;
  const float* csrc = slab + (size_t)sub * nblk * 16 + 4 * c4;       // conv piece `sub` of every row: rows x 16 floats, contiguous
  if (kind < 2) {
    const int tn = kind == 0 ? t1n : t2n;
    const int mt = (int)((float)sub / (float)tn + 0.01f);            // (exact for the few hundred tiles there are)
    m0 = 8 * mt; n0 = 8 * (sub - mt * tn);
    if (tid < 256) {
      sb = kind == 0 ? ft.init(dh, m0, G.H, z, n0, B) : ft.init(dl, m0, G.K, h, n0, B);
      ft.issue(sb);
    }
  } else if (kind == 2 && tid < 256) {
    // lane = (16-byte quarter c4, row lane r16); wave wv, load i: rows (4 i + wv) * 16 + r16 — every wave-level load is 1 KiB
    // of contiguous bytes
#pragma unroll
    for (int i = 0; i < 4; ++i)                          // (unconditional, clamped row; masked where they are summed)
      cv[i] = *reinterpret_cast<const float4*>(csrc + (size_t)min((4 * i + wv) * 16 + r16, nblk - 1) * 16);
  }
  // ---- which parameter(s) this thread finishes (p, own; p2, own2: the bias of a first-column tile) — from the preloaded words
  // alone — and their ADAM state, requested in the same batch as the gradients: UNCONDITIONAL loads from a clamped index
  // (element 0 for a lane that owns nothing; the workspace stands in for a missing theta), masked where they are used
  int64_t p = 0, p2 = 0;
  bool own = false, own2 = false;
  if (kind == 0) {
    const int j = m0 + ((tid >> 3) & 7), i = n0 + (tid & 7);
    own = tid < 64 && j < G.H && i < G.F2;
    p = G.oFc1w + (int64_t)j * G.F2 + i;
    own2 = n0 == 0 && tid < 8 && m0 + tid < G.H;
    p2 = G.oFc1b + m0 + tid;
  } else if (kind == 1) {
    const int k = m0 + ((tid >> 3) & 7), j = n0 + (tid & 7);
    own = tid < 64 && k < G.K && j < G.H;
    p = G.oFc2w + (int64_t)k * G.H + j;
    own2 = n0 == 0 && tid < 8 && m0 + tid < G.K;
    p2 = G.oFc2b + m0 + tid;
  } else if (kind == 2) {
    p = (int64_t)16 * sub + tid;
    own = tid < 16 && p < G.NCONV;
  }
  RSTAMP(1);
  float th0, m_0, v_0, th2 = 0.f, m_2 = 0.f, v_2 = 0.f;
  {
    const bool adam = theta != nullptr;
    const float* tb = adam ? theta : ws;
    const float* mb = adam ? m : ws;
    const float* vb = adam ? v : ws;
    const int64_t q = (adam && own && kind < 3) ? p : 0;
    th0 = tb[q]; m_0 = mb[q]; v_0 = vb[q];
    if (kind < 2) {                                  // (scalar condition)
      const int64_t q2 = (adam && own2) ? p2 : 0;
      th2 = tb[q2]; m_2 = mb[q2]; v_2 = vb[q2];
    }
  }
  __builtin_amdgcn_sched_barrier(0);                 // (nothing that waits for these loads may move up here)
  RSTAMP(2);
  // the tail's scalars (exchange on / off, scaler, gradient pointer, ADAM's constants) live in the argument struct: read where
  // they are used they are four DEPENDENT kernarg fetches behind the barrier; fetched here they arrive under the gradient loads
  const int world = a.x.world;
  ReduceTail tl = {a.scaler, a.grad, a.lr, a.b1, a.b2, a.eps};
  int hp_st = 0;
  // the averaged copy: its pointer and words in the same fetch (a second one behind it is a second wait for the argument struct)
  float* avp = nullptr;
  int av_kind = 0, av_start = 0;
  float av_w = 0.f, av0 = 0.f, av2 = 0.f;
  if constexpr (AVG) {
    avp = a.av.avg; av_kind = a.av.kind; av_w = a.av.w; av_start = a.av.start;
    asm volatile("" ::"s"(avp), "s"(av_kind), "s"(av_w), "s"(av_start), "s"(world), "s"(tl.scaler), "s"(tl.grad), "s"(tl.eps));
  }
  if (!SCHED) asm volatile("" ::"s"(world), "s"(tl.scaler), "s"(tl.grad), "s"(tl.lr), "s"(tl.b1), "s"(tl.b2), "s"(tl.eps));
  if constexpr (AVG) {                               // ... and the owned elements requested at once
    const bool adam = theta != nullptr;
    av0 = avp[(adam && own && kind < 3) ? p : 0];
    if (kind < 2) av2 = avp[(adam && own2) ? p2 : 0];
  }
  if constexpr (SCHED) {
    // the step's row (uniform addresses: step count and row index -> 16 bytes of the table), requested here, behind the first
    // batch of gradient and state loads; wave 4 and the tail wait for it where they use it
    const int32_t* sd = a.step_dev;
    const int32_t* rd = a.hp.row_dev;
    const float* tb = a.hp.table;
    const int rows = a.hp.rows;
    asm volatile("" ::"s"(world), "s"(tl.scaler), "s"(tl.grad), "s"(tl.eps), "s"(sd), "s"(rd), "s"(tb), "s"(rows));
    // (this launch writes none of the three: read through the constant address space they are scalar loads, which do not
    // queue behind the gradient loads as vector loads would)
    hp_st = sd != nullptr ? *(const_i32)sd : a.step;
    int row = rd != nullptr ? *(const_i32)rd : hp_st - 1;
    row = row < 0 ? 0 : (row > rows - 1 ? rows - 1 : row);
    const const_f32 hr = (const_f32)tb + (size_t)row * 4;
    tl.lr = hr[0]; tl.b1 = hr[1]; tl.b2 = hr[2];
  }
  if (kind == 3) {                                   // attention slabs: the block's role needs the argument struct
    p = a.oAttn + (int64_t)64 * sub + tid;
    own = tid < 64 && 64 * sub + tid < a.ASLAB;
    if (theta != nullptr && own) {
      th0 = theta[p]; m_0 = m[p]; v_0 = v[p];
      if constexpr (AVG) av0 = avp[p];
    }
  }
  if constexpr (AVG && !SCHED) {
    // the step count (the schedule instance has it): requested behind the attention block's words — a scalar wait cannot tell
    // loads apart, and in front of them every wave waited there for this dependent fetch — and used in the tail
    const int32_t* sd = a.step_dev;
    hp_st = sd != nullptr ? *(const_i32)sd : a.step;
  }
  float* part = &vbuf[0][0];
  if (tid >= 256) {
    // bias corrections (lanes 0 / 1 of wave 4: beta1 / beta2 side by side), b^step by repeated squaring in double
    if (theta != nullptr && tid < 258) {
      float bc = tid == 256 ? a.bc1 : a.bc2_sqrt;
      if (SCHED) {                                     // (the host does not know the row's betas: always formed here)
        const double pw = powi_double((double)(tid == 256 ? tl.b1 : tl.b2), hp_st);
        bc = tid == 256 ? (float)(1.0 - pw) : (float)sqrt(1.0 - pw);
      } else if (a.step_dev != nullptr) {
        const double pw = powi_double((double)(tid == 256 ? a.b1 : a.b2), *a.step_dev);
        bc = tid == 256 ? (float)(1.0 - pw) : (float)sqrt(1.0 - pw);
      }
      bcs[tid - 256] = bc;
    }
  } else if (kind < 2) {
    ft.consume();
    for (sb += 8; sb < ft.s1; sb += 8) { ft.issue(sb); ft.consume(); }
    const f32x4_t v = ft.acc0 + ft.acc1;
#pragma unroll
    for (int r = 0; r < 4; ++r) vbuf[wv][(4 * ft.kk + r) * 16 + (lane & 15)] = v[r];   // C layout: row 4 (lane >> 4) + r, column lane & 15
    const float bias = swap_add32(swap_add16(ft.bs));                                  // over the four k lanes of a row
    if (lane < 16) bbuf[wv][lane] = bias;                                              // [wave][half * 8 + row]
  } else if (kind == 2) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int i0 = 0;;) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool in = (4 * (i0 + i) + wv) * 16 + r16 < nblk;
        acc.x += in ? cv[i].x : 0.f; acc.y += in ? cv[i].y : 0.f; acc.z += in ? cv[i].z : 0.f; acc.w += in ? cv[i].w : 0.f;
      }
      i0 += 4;
      if ((4 * i0 + wv) * 16 >= nblk) break;                           // (more than 256 rows: not with today's MAX_BLOCKS)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        cv[i] = *reinterpret_cast<const float4*>(csrc + (size_t)min((4 * (i0 + i) + wv) * 16 + r16, nblk - 1) * 16);
    }
    // over the 16 row lanes (lane bits 2..5): xor 4 / xor 8 inside a 16-lane row by row rotations, then the row / half swaps
    float e[4] = {acc.x, acc.y, acc.z, acc.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float x = e[k];
      x = DMF_DPP_ADD(x, 0x124);     // row_ror:4
      x = DMF_DPP_ADD(x, 0x128);     // row_ror:8
      e[k] = swap_add32(swap_add16(x));
    }
    if (lane < 4) *reinterpret_cast<float4*>(part + wv * 16 + 4 * c4) = make_float4(e[0], e[1], e[2], e[3]);
  } else {
    const int pitch = a.ASLAB, nb = a.nablk;
    const int q4 = tid & 15, ch = tid >> 4;
    const bool in_row = 64 * sub + 4 * q4 < pitch;
    const float* sl = a.aslab + 64 * sub + 4 * q4;
    const int per = (nb + 15) / 16;
    const int lo = ch * per, hi = min(nb, lo + per);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int b0 = lo; b0 < hi; b0 += 16) {
      float4 v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i)
        v[i] = (in_row && b0 + i < hi) ? *reinterpret_cast<const float4*>(sl + (size_t)(b0 + i) * pitch) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < 16; ++i) { acc.x += v[i].x; acc.y += v[i].y; acc.z += v[i].z; acc.w += v[i].w; }
    }
    *reinterpret_cast<float4*>(part + ch * 64 + 4 * q4) = acc;          // [16 chunks][64]
  }
  RSTAMP(3);
  __syncthreads();
  RSTAMP(4);
  float g = 0.f, g2 = 0.f;
  if (tid < 256) {
    if (kind < 2) {
      if (tid < 64) {                                  // the two diagonal blocks of every wave's result, in wave order
        const int e0 = (tid >> 3) * 16 + (tid & 7), e1 = e0 + 8 * 16 + 8;
        g = ((vbuf[0][e0] + vbuf[0][e1]) + (vbuf[1][e0] + vbuf[1][e1])) + ((vbuf[2][e0] + vbuf[2][e1]) + (vbuf[3][e0] + vbuf[3][e1]));
      }
      if (tid < 8) g2 = ((bbuf[0][tid] + bbuf[0][8 + tid]) + (bbuf[1][tid] + bbuf[1][8 + tid])) +
                        ((bbuf[2][tid] + bbuf[2][8 + tid]) + (bbuf[3][tid] + bbuf[3][8 + tid]));
    } else if (kind == 2) {
      if (tid < 16) g = (part[tid] + part[16 + tid]) + (part[32 + tid] + part[48 + tid]);
    } else if (tid < 64) {
      float t[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) t[i] = part[i * 64 + tid];
      g = tree16(t);
    }
  }
  if (world > 1) {                               // (the owning lanes exchange; no barriers inside)
    const int seq = *a.step_dev + a.seq_bias;
    g = xgmi_exchange(a.x, 0, seq, p, own, g) * a.grad_scale;
    if (kind < 2 && n0 == 0) g2 = xgmi_exchange(a.x, 0, seq, p2, own2, g2) * a.grad_scale;
  }
  if (own) th0 = adam_apply(tl, theta, m, v, p, g, th0, m_0, v_0, bcs);
  if (own2) th2 = adam_apply(tl, theta, m, v, p2, g2, th2, m_2, v_2, bcs);
  if constexpr (AVG) {                               // (th0, th2: what adam_apply has just stored)
    if (theta != nullptr) {
      if (own) avp[p] = avg_rule(av_kind, av_w, av_start, hp_st, av0, th0);
      if (own2) avp[p2] = avg_rule(av_kind, av_w, av_start, hp_st, av2, th2);
    }
  }
  RSTAMP(5);
  RSTAMP_DUMP();
}

// ------------------------------------------------------------------------------ dynamic loss scaling (GradScaler's role)
// state: [0] scale  [1] growth tracker  [2] found_inf  [3] skipped steps  [4] ticket (int bits)
__global__ __launch_bounds__(256) void unscale_check_kernel(float* grad, int64_t n, float grad_scale, float* state) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= n) return;
  const float g = grad[p] * (grad_scale / state[0]);
  grad[p] = g;
  if (!isfinite(g)) state[2] = 1.f;                 // (every writer stores the same value)
}

// ------------------------------------------------------------------------------ weight decay, AdamW, gradient-norm clipping
// optim_step_kernel is the only statement of an optimiser step on a flat gradient: dmf_optim_step (include/dmf.h states the six
// steps) and, with neutral keys, dmf_adam_step, dmf_sgd_step, dmf_rmsprop_step and dmf_unscale_adam.  One block per 256
// elements.  With a scaler state or clipping EVERY block first walks the whole gradient — lane t takes g[t], g[t + 256], ... in
// index order into one double, the 256 doubles meet in a fixed LDS tree — so every block holds the same norm bits and the same
// skip decision and then updates its own 256 elements: no second launch, no grid barrier, no atomics on data.
// (double)g * (double)g is exact, so an fma and a multiply-add give the same sum.  The values a block needs from what the
// step's end changes (scale, step count, found_inf) are read before its ticket; the last block to take a ticket closes the
// step.  Without a scaler state nothing is read that the end changes (block 0 alone reads and advances the cursor), and there
// is no ticket; without clipping either there is no norm pass: the plain update of the kind.
// a.checked (dmf_unscale_adam alone): found_inf of this step is in state[2] already — unscale_check_kernel or the reduce launch
// put it there — so state[2] decides the skip and the gradient is not walked a second time.  a.bc1 != 0 (dmf_adam_step without
// a device step count): ADAM's bias corrections as the host formed them.
__device__ __forceinline__ float scaled_grad(const float* __restrict__ grad, int64_t i, float gs) {
#pragma clang fp contract(off)           // g is a float of its own, as torch's unscale_ / clip_grad_norm_ leave one in memory
  return grad[i] * gs;
}

// One instance per kind: with the kind a run-time branch the compiler merges the three updates' last subtraction into one
// unfused `theta - x`, and ADAM's theta then is an ulp away from the fused form it has always had
// (tests/golden/g11_optim_entry_bits.json holds the bits of every entry point).
// SCHED (the *_sched entry points): lr and, by kind, beta1 / beta2 or momentum come from the step's row of a.hp,
// read at entry beside the step count (and so, like it, before the ticket); everything below runs on them as on the launch
// arguments.  A step the scaler skips takes its count back: with hp.row_dev == nullptr the next step reads the same row again.
// AVG (the *_avg entry points): a lane that has updated theta[p] also keeps a.av.avg[p] by avg_rule, with the step
// count read at entry; a step the scaler skips leaves avg alone and, its count taken back, does not count for the mean.
template <int KIND, bool SCHED, bool AVG>
__global__ __launch_bounds__(256) void optim_step_kernel(
    const std::conditional_t<AVG, OptimAvgArgs, std::conditional_t<SCHED, OptimSchedArgs, OptimArgs>> a) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  const int64_t p = (int64_t)blockIdx.x * 256 + t;
  const int st = a.step_dev != nullptr ? *a.step_dev : a.step;
  float lr = a.lr, b1 = a.b1, b2 = a.b2, momentum = a.momentum;
  float av_old = 0.f;                                  // the element of avg, requested at entry (unconditional, clamped index)
  if constexpr (AVG) av_old = a.av.avg[p < a.n ? p : a.n - 1];
  if constexpr (SCHED) {
    int row = a.hp.row_dev != nullptr ? *a.hp.row_dev : st - 1;
    row = row < 0 ? 0 : (row > a.hp.rows - 1 ? a.hp.rows - 1 : row);
    const float* hr = a.hp.table + (size_t)row * 4;
    const float r0 = hr[0], r1 = hr[1], r2 = hr[2], r3 = hr[3];
    lr = r0;
    if (KIND == DMF_OPT_ADAM || KIND == DMF_OPT_ADAMW) { b1 = r1; b2 = r2; }
    if (KIND == DMF_OPT_SGD) momentum = r3;
  }
  const float gs = (a.state != nullptr && !a.unscaled) ? a.grad_scale / a.state[0] : a.grad_scale;
  const bool clip = a.max_norm > 0.f;
  bool skip = a.checked && a.state[2] != 0.f;          // (read, like the scale and the step count, before the ticket)
  float norm = 0.f, coef = 1.f;
  if ((a.state != nullptr && !a.checked) || clip) {
    double s = 0.0;
    int bad = 0;
    // 16 loads in flight per lane (unconditional, from a clamped index, masked where they are summed: a load under a lane
    // condition becomes a branch, and one load per trip is one L2 round trip per 256 elements: 32 in a row at n = 8,009,
    // measured as 8 us per launch); the sum keeps the index order, and a masked element adds +0.0
    for (int64_t i0 = t; i0 < a.n; i0 += 16 * 256) {
      float gq[16];
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int64_t i = i0 + (int64_t)q * 256;
        gq[q] = scaled_grad(a.grad, i < a.n ? i : a.n - 1, gs);
      }
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const bool in = i0 + (int64_t)q * 256 < a.n;
        const float g = in ? gq[q] : 0.f;
        bad |= !isfinite(g);
        s += (double)g * (double)g;
      }
    }
    part[t] = s;
    if (__syncthreads_or(bad) != 0 && a.state != nullptr && !a.checked) skip = true;
    for (int w = 128; w > 0; w >>= 1) {
      if (t < w) part[t] += part[t + w];
      __syncthreads();
    }
    if (clip) {
      norm = (float)sqrt(part[0]);
      const float c = a.max_norm / (norm + 1e-6f);
      coef = c > 1.f ? 1.f : c;                        // (a NaN norm stays a NaN coefficient: torch's clamp)
    }
  }
  if (!skip && p < a.n) {
    float g = scaled_grad(a.grad, p, gs);
    {
#pragma clang fp contract(off)
      if (clip) g *= coef;
      if (a.weight_decay != 0.f) {
        const float th = a.theta[p];
        if (KIND == DMF_OPT_ADAMW) a.theta[p] = th * (float)(1.0 - (double)lr * (double)a.weight_decay);
        else g += a.weight_decay * th;
      }
    }
    if (KIND == DMF_OPT_SGD) sgd_update(a.theta, a.m, p, g, lr, momentum, st);
    else if (KIND == DMF_OPT_RMSPROP) rmsprop_update(a.theta, a.m, p, g, lr, a.alpha, a.eps);
    else {
      float bc1 = a.bc1, bc2s = a.bc2_sqrt;
      if (bc1 == 0.f) bias_corrections(st, b1, b2, bc1, bc2s);
      adam_update(a.theta, a.m, a.v, p, g, lr, b1, b2, a.eps, bc1, bc2s);
    }
    if constexpr (AVG) a.av.avg[p] = avg_rule(a.av.kind, a.av.w, a.av.start, st, av_old, a.theta[p]);
  }
  bool closer = blockIdx.x == 0 && t == 0;
  if (a.state != nullptr) {
    // the last block to get here has seen every other block read the scale and the step count: it closes the step
    __syncthreads();
    closer = false;
    if (t == 0) {
      __threadfence();
      int* ticket = reinterpret_cast<int*>(a.state + 4);
      if (atomicAdd(ticket, 1) == (int)gridDim.x - 1) {
        *ticket = 0;
        closer = true;
        if (skip) {
          a.state[0] *= a.backoff; a.state[1] = 0.f; a.state[3] += 1.f;
          *a.step_dev -= 1;                             // a skipped step does not count for the bias corrections
        } else {
          const float tr = a.state[1] + 1.f;
          if (tr >= (float)a.interval) { a.state[0] *= a.growth; a.state[1] = 0.f; }
          else a.state[1] = tr;
        }
        a.state[2] = 0.f;
      }
    }
  }
  if (closer) {
    const int cur = a.cursor_dev != nullptr ? *a.cursor_dev : 0;
    if (clip && a.norm_hist != nullptr) a.norm_hist[cur] = norm;
    if (a.cursor_dev != nullptr) *a.cursor_dev = cur + 1;
  }
}

__global__ __launch_bounds__(256) void xgmi_allreduce_kernel(const XgmiDev x, float* buf, int64_t n, int seq) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const bool valid = i < n;
  const float s = xgmi_exchange(x, 1, seq, i, valid, valid ? buf[i] : 0.f);
  if (valid) buf[i] = s;
}

// ------------------------------------------------------------------------------ validation sum and best weights on the device
// acc[0] += sum_i (double)loss[i], ONE workgroup: lane t adds loss[t], loss[t + 256], ... in index order, then the 256 partial
// sums meet in a fixed tree: the same bits on every run.  Lane 0 alone reads, adds to and writes acc[0]; the launches before
// and after are ordered by the stream.
__global__ __launch_bounds__(256) void valid_accum_kernel(const float* __restrict__ loss, int n, double* acc) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int i = t; i < n; i += 256) s += (double)loss[i];
  part[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) part[t] += part[t + w];
    __syncthreads();
  }
  if (t == 0) acc[0] += part[0];
}

// The end of an epoch's validation pass, ONE workgroup (nobody else can read *best while it changes): val = acc[0] goes into
// val_hist[epoch]; a val strictly below *best (a NaN never is) becomes the best, with its epoch and a copy of theta; acc[0] is
// cleared for the next epoch.  Every lane has read acc[0] and *best before the barrier, lane 0 writes them after it.
__global__ __launch_bounds__(1024) void keep_best_kernel(double* acc, double* best, int32_t* best_epoch, int32_t epoch,
                                                         const float* __restrict__ theta, float* __restrict__ best_theta,
                                                         int64_t n, double* val_hist) {
  const double val = acc[0];
  const bool better = val < *best;
  __syncthreads();
  if (better) {
    // 16-byte pieces where both vectors allow it, then (or instead) the single floats
    const bool vec = ((reinterpret_cast<uintptr_t>(theta) | reinterpret_cast<uintptr_t>(best_theta)) & 15) == 0;
    const int64_t n4 = vec ? n / 4 : 0;
    const float4* src = reinterpret_cast<const float4*>(theta);
    float4* dst = reinterpret_cast<float4*>(best_theta);
    for (int64_t i = threadIdx.x; i < n4; i += 1024) dst[i] = src[i];
    for (int64_t i = 4 * n4 + threadIdx.x; i < n; i += 1024) best_theta[i] = theta[i];
  }
  if (threadIdx.x == 0) {
    val_hist[epoch] = val;
    if (better) { *best = val; *best_epoch = epoch; }
    acc[0] = 0.0;
  }
}


// ------------------------------------------------------------------------------ launchers
// Blocks per kind, tiles per row, packed for the kernel's preloaded scalars.  A geometry the packing cannot hold is refused:
// hipErrorInvalidValue, and *refusal names the reason.
hipError_t launch_grad_reduce(const ReduceArgs& a, const Layout& L, int B, const float* ws, hipStream_t st, const char** refusal,
                              const HpSched* hp, int32_t step, const AvgArgs* av) {
  *refusal = nullptr;
  if (av != nullptr && a.x.world > 1) {
    *refusal = "grad_reduce: the xgmi exchange has no averaging form";
    return hipErrorInvalidValue;
  }
  if (L.H % 8 != 0 || L.F2 % 8 != 0) {
    *refusal = "grad_reduce: hidden width and 2 x gmf.width must be multiples of 8";
    return hipErrorInvalidValue;
  }
  const int t1n = L.F2 / 8, t2n = L.H / 8;
  const int nFc1 = (L.H / 8) * t1n, nFc2 = ((L.K + 7) / 8) * t2n, nConv = (L.NCONV + 15) / 16;
  const int nAttn = L.attention ? (a.ASLAB + 63) / 64 : 0;
  if (nFc1 > 0xffff || nFc2 > 0xffff || nConv > 0xffff || nAttn > 0x7fff) {
    *refusal = "grad_reduce: too many blocks of one kind";
    return hipErrorInvalidValue;
  }
  int w3 = 0, w4 = 0;
  if (!reduce_words_pack(L, B, &w3, &w4)) {
    *refusal = "grad_reduce: the layout does not fit the packed launch words";
    return hipErrorInvalidValue;
  }
  const int grid = nFc1 + nFc2 + nConv + nAttn + 1;   // + the bookkeeping block
  if (av != nullptr) {
    ReduceAvgArgs aa{};
    static_cast<ReduceArgs&>(aa) = a;
    if (hp != nullptr) aa.hp = *hp;
    aa.step = step; aa.av = *av;
    if (hp != nullptr)
      hipLaunchKernelGGL((grad_reduce_kernel<true, true>), dim3(grid), dim3(320), 0, st, ws, a.theta, a.m, a.v, nFc1 | (t1n << 16),
                         nFc2 | (t2n << 16), nConv | (nAttn << 16), w3, w4, B, aa);
    else
      hipLaunchKernelGGL((grad_reduce_kernel<false, true>), dim3(grid), dim3(320), 0, st, ws, a.theta, a.m, a.v, nFc1 | (t1n << 16),
                         nFc2 | (t2n << 16), nConv | (nAttn << 16), w3, w4, B, aa);
  } else if (hp != nullptr) {
    ReduceSchedArgs as{};
    static_cast<ReduceArgs&>(as) = a;
    as.hp = *hp; as.step = step;
    hipLaunchKernelGGL((grad_reduce_kernel<true, false>), dim3(grid), dim3(320), 0, st, ws, a.theta, a.m, a.v, nFc1 | (t1n << 16),
                       nFc2 | (t2n << 16), nConv | (nAttn << 16), w3, w4, B, as);
  } else
    hipLaunchKernelGGL((grad_reduce_kernel<false, false>), dim3(grid), dim3(320), 0, st, ws, a.theta, a.m, a.v, nFc1 | (t1n << 16), nFc2 | (t2n << 16),
                       nConv | (nAttn << 16), w3, w4, B, a);
  return hipGetLastError();
}

static dim3 blocks256(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// the first launch of dmf_unscale_adam(unscaled = 0): unscale + found_inf check; launch_optim_step (checked) follows
hipError_t launch_unscale_check(float* grad, int64_t n, float grad_scale, float* state, hipStream_t st) {
  hipLaunchKernelGGL(unscale_check_kernel, blocks256(n), dim3(256), 0, st, grad, n, grad_scale, state);
  return hipGetLastError();
}

hipError_t launch_optim_step(const OptimArgs& a, hipStream_t st, const HpSched* hp, const AvgArgs* av) {
  if (a.checked && a.state == nullptr) return hipErrorInvalidValue;
  const dim3 grid = blocks256(a.n), block(256);
  OptimAvgArgs aa{};
  if (hp != nullptr || av != nullptr) static_cast<OptimArgs&>(aa) = a;
  if (hp != nullptr) aa.hp = *hp;
  if (av != nullptr) aa.av = *av;
  const OptimSchedArgs& as = aa;
#define DMF_OPTIM_LAUNCH(K) \
  if (av != nullptr && hp != nullptr) hipLaunchKernelGGL((optim_step_kernel<K, true, true>), grid, block, 0, st, aa); \
  else if (av != nullptr) hipLaunchKernelGGL((optim_step_kernel<K, false, true>), grid, block, 0, st, aa); \
  else if (hp != nullptr) hipLaunchKernelGGL((optim_step_kernel<K, true, false>), grid, block, 0, st, as); \
  else hipLaunchKernelGGL((optim_step_kernel<K, false, false>), grid, block, 0, st, a)
  switch (a.kind) {
    case DMF_OPT_ADAM: DMF_OPTIM_LAUNCH(DMF_OPT_ADAM); break;
    case DMF_OPT_ADAMW: DMF_OPTIM_LAUNCH(DMF_OPT_ADAMW); break;
    case DMF_OPT_SGD: DMF_OPTIM_LAUNCH(DMF_OPT_SGD); break;
    case DMF_OPT_RMSPROP: DMF_OPTIM_LAUNCH(DMF_OPT_RMSPROP); break;
    default: return hipErrorInvalidValue;
  }
#undef DMF_OPTIM_LAUNCH
  return hipGetLastError();
}

hipError_t launch_weight_average(const AvgArgs& av, const float* theta, int64_t n, int32_t step, const int32_t* step_dev,
                                 hipStream_t st) {
  hipLaunchKernelGGL(weight_average_kernel, blocks256(n), dim3(256), 0, st, av, theta, n, step, step_dev);
  return hipGetLastError();
}

hipError_t launch_xgmi_allreduce(const XgmiDev& x, float* buf, int64_t n, int seq, hipStream_t st) {
  hipLaunchKernelGGL(xgmi_allreduce_kernel, blocks256(n), dim3(256), 0, st, x, buf, n, seq);
  return hipGetLastError();
}

hipError_t launch_valid_accum(const float* loss, int n, double* acc, hipStream_t st) {
  hipLaunchKernelGGL(valid_accum_kernel, dim3(1), dim3(256), 0, st, loss, n, acc);
  return hipGetLastError();
}

hipError_t launch_keep_best(double* acc, double* best, int32_t* best_epoch, int32_t epoch, const float* theta, float* best_theta,
                            int64_t n, double* val_hist, hipStream_t st) {
  hipLaunchKernelGGL(keep_best_kernel, dim3(1), dim3(1024), 0, st, acc, best, best_epoch, epoch, theta, best_theta, n, val_hist);
  return hipGetLastError();
}

#ifdef DMF_STAMPS
hipError_t set_reduce_stamps(unsigned long long* p) { return hipMemcpyToSymbol(HIP_SYMBOL(g_rstamps), &p, sizeof(p)); }
#endif

}  // namespace dmf
