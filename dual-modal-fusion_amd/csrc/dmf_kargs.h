// Kernel argument blocks and internal entry points shared by the translation units of libdmf_hip.so.
// ONE definition each: dmf_capi.hip fills these structs and calls the launchers, the kernel files define both.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "../../include/dmf.h"
#include "dmf_shapes.h"
#include "dmf_xgmi.h"

namespace dmf {


// hipFuncSetAttribute(MaxDynamicSharedMemorySize) belongs to the (kernel, device) pair and is not capturable: every launch
// site keeps ONE of these per kernel instance (a function-local static) and calls set() before the launch — once per device,
// under a lock (two host threads may reach a first launch together).
struct LdsAttrOnce {
  std::mutex mu;
  bool done[64] = {};
  hipError_t set(const void* fn, int bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= 64) return hipErrorInvalidDevice;
    std::lock_guard<std::mutex> lock(mu);
    if (done[dev]) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    done[dev] = (e == hipSuccess);
    return e;
  }
};

enum { MODE_FWD = 0, MODE_TRAIN = 1, MODE_BWD = 2, MODE_TOKENS = 3, MODE_DENSE = 4, MODE_UNIT = 5 };
// TOKENS: conv stages only, for the attention kernel.  DENSE: conv backward from dense dL/dYa, dL/dYb maps [B][F][P2]
// (written by the attention kernel's backward) instead of the rank-1 pool x dz form; the head is skipped.
// UNIT (v2 kernel only): forward + the conv backward for a UNIT gradient on every pooled feature; `slab` then is
// [B][SLAB], one row of unit gradients per PATCH (dmf_forward_unit / dmf_backward_unit: a loss that couples the batch).

// patch kernel (dmf_patch_v2.hip)
struct KArgs {
  dmf_input in;
  const float* theta;
  const float* pool;
  const int32_t* labels;
  const float* dlogits;
  float loss_scale;
  const float* scaler;  // nullable: device loss-scaler state, [0] multiplies loss_scale (dmf_train_fwd_bwd_scaled)
  float* logits;
  float* loss;
  int32_t* pred;
  float* slab;   // [grid][SLAB]
  float* ws_z;   // [B][2F]
  float* ws_h;   // [B][H]
  float* ws_dh;  // [B][H]
  float* ws_dl;  // [B][KMAX]
  int32_t* adam_step;   // device step counter to advance (nullable)
  unsigned short* tokA; // MODE_TOKENS: bf16 token maps [B][128][64] (tokens x channels, zero padded) of both branches
  unsigned short* tokB;
  float* zout;          // MODE_TOKENS: pooled features [B][2F] before attention
  const float* dYa;     // MODE_DENSE: dL/d(spat_a output) [B][F][P][RS] (rows padded to 16 bytes)
  const float* dYb;     // MODE_DENSE: dL/d(spat_b output) [B][F][P][RS]
  int32_t K;
};
// wave-per-channel-block kernel (dmf_patch_v2.hip): FWD / TRAIN / BWD of the shapes it is built for
int patch_v2_supported(const dmf_shape& s, int mode, int half = 0);   // half: dmf_input.half (fp16 primary scene)
const char* patch_v2_half_shape_list();
hipError_t patch_v2_dispatch(const dmf_shape& s, int mode, const KArgs& a, hipStream_t st);
// second half of the unit-gradient step: per patch dh, dz from dlogits; slab row of workgroup g = sum over its patches of
// dz x unit row; ws_dh / ws_dl for the fc gradients
struct UnitBwdArgs {
  const float* theta; const float* dlogits; const float* unit; const float* ws_h;
  float* ws_dh; float* ws_dl; float* slab;
  int32_t B, K;
};
hipError_t patch_v2_unit_backward(const dmf_shape& s, const UnitBwdArgs& a, hipStream_t st);
const char* patch_v2_shape_list();

// attention kernels (dmf_attention.hip)
struct AttnTrainArgs {
  const unsigned short* tokA; const unsigned short* tokB;     // [B][128][64] bf16
  const float* zin;                     // [B][2F]
  const float* theta; const float* pool;
  const int32_t* labels; const int32_t* cursor;   // labels[(*cursor) * B + b]   (cursor may be null)
  const float* dlogits;                 // used when labels == null: caller-supplied dL/dlogits [B][K]
  float loss_scale;
  float* logits; float* loss;           // [B][K], [B] (loss may be null)
  float* ws_z; float* ws_h; float* ws_dh; float* ws_dl;   // head vectors for the gradient reduce
  float* dYa; float* dYb;               // [B][F][P][RS], RS = P rounded up to 4 (rows 16-byte aligned)
  float* aslab;                         // [gridDim][4*E*F] attention weight gradients (Wq, Wk, Wv, Wo)
  int32_t* pred;                        // forward-only launch: argmax per patch (may be null)
  const unsigned short* wprep;          // [NH][WPREP] bf16 weights of every head, already in the LDS layout (attn_prep_kernel)
  int64_t oWq, oWk, oWv, oWo, oFc1w, oFc1b, oFc2w, oFc2b;
  int32_t B, K;
  // Read by the criterion instances of the training kernel alone (dmf_train_attn_fwd_bwd_ce: class weights, label smoothing or a
  // focal term where the plain instance forms its cross-entropy); they FOLLOW the words above, whose offsets the plain instances
  // keep.  `labels` then is the GLOBAL batch's, rank-major (labels[((*cursor) * ranks + rank) * B + b], as CeArgs), and
  // denom[*cursor] its denominator (dmf_ce_denominators).
  const float* class_w;                 // [K], nullable = all ones
  const double* denom;                  // [plan rows]
  int32_t ranks, rank, kind;
  float eps, gamma, grad_scale;
};
size_t attn_prep_bytes();
hipError_t attn_prep_launch(const float* theta, int64_t oWq, int64_t oWk, int64_t oWv, int64_t oWo, void* out, hipStream_t st);
hipError_t attn_train_dispatch(const dmf_shape& s, const AttnTrainArgs& a, int grid, hipStream_t st);
hipError_t attn_train_ce_dispatch(const dmf_shape& s, const AttnTrainArgs& a, int grid, hipStream_t st);   // the criterion instances
hipError_t attn_forward_dispatch(const dmf_shape& s, const AttnTrainArgs& a, int grid, hipStream_t st);
int attn_shape_supported(const dmf_shape& s);

// ------------------------------------------------------------------------------ gradient reduction (+Adam)
//   conv params  : grad[p] = sum_blk slab[blk][p]
//   fc1.weight   : grad = sum_b dh[b][j] * z[b][i]      fc1.bias: sum_b dh[b][j]
//   fc2.weight   : grad = sum_b dl[b][k] * h[b][j]      fc2.bias: sum_b dl[b][k]
// (the conv slabs and head vectors z / h / dh / dl reach the kernel as leading scalar arguments: launch_grad_reduce)
// The device-resident schedule of the *_sched entry points (include/dmf.h: dmf_hp_schedule): table [rows][4] of
// (lr, beta1, beta2, momentum); the row of a step is *row_dev, or with row_dev == nullptr the 1-based step count - 1, clamped
// to [0, rows - 1].  The words follow ReduceArgs / OptimArgs in argument structs that only the schedule instances of the two
// kernels take: the default instances keep their kernel arguments byte for byte.
struct HpSched { const float* table; const int32_t* row_dev; int32_t rows; };
// The averaged copy of the weights of the *_avg entry points (include/dmf.h: dmf_weight_avg): avg [n] beside
// theta, kind DMF_AVG_*, w = float32(1 - decay) for DMF_AVG_EMA, start = the first averaged optimiser step (1-based).  The words
// follow the schedule's in argument structs that only the averaging instances take (which read the schedule when SCHED).
struct AvgArgs { float* avg; int32_t kind; float w; int32_t start; };
struct ReduceArgs {
  int B, NCONV, F2, H, K;
  int64_t oFc1w, oFc1b, oFc2w, oFc2b;
  float* grad;
  float* theta; float* m; float* v;   // Adam (theta == nullptr: reduce only)
  float lr, b1, b2, eps, bc1, bc2_sqrt;
  const int32_t* step_dev;            // optional device-side step count (overrides bc1 / bc2_sqrt)
  int32_t* cursor_dev;                // optional epoch-plan cursor to advance
  const float* loss; float* loss_hist;
  const float* aslab; int nablk, ASLAB; int64_t oAttn;   // attention weights: sum of the attention kernel's slabs
  XgmiDev x;                          // x.world > 1: exchange the gradient with the peer ranks before Adam
  float grad_scale; int seq_bias;
  float* scaler;                      // loss-scaler state (dmf_grad_reduce_scaled): grad <- sum / scaler[0], non-finite -> scaler[2]
};
// ... of grad_reduce_kernel<true>: the schedule, and the host step count (used when step_dev == nullptr)
struct ReduceSchedArgs : ReduceArgs { HpSched hp; int32_t step; };
// ... of grad_reduce_kernel<SCHED, true>: hp is read by the <true, true> instance alone, step by both
struct ReduceAvgArgs : ReduceSchedArgs { AvgArgs av; };
// dmf_reduce.hip.  launch_grad_reduce carves the head vectors and conv slabs out of the workspace `ws` itself; a geometry
// its block packing cannot hold is refused with hipErrorInvalidValue and *refusal set to the reason (else null).
// hp != nullptr launches the schedule instance, which also takes the host step count `step`; av != nullptr the averaging
// instance (with or without a schedule; not with the xgmi exchange).
hipError_t launch_grad_reduce(const ReduceArgs& a, const Layout& L, int B, const float* ws, hipStream_t st, const char** refusal,
                              const HpSched* hp = nullptr, int32_t step = 0, const AvgArgs* av = nullptr);
// The optimiser step on the flat gradient, one launch (optim_step_kernel): dmf_optim_step with weight decay / AdamW /
// gradient-norm clipping, and with neutral keys dmf_adam_step, dmf_sgd_step, dmf_rmsprop_step and dmf_unscale_adam.
// launch_optim_step and launch_unscale_check are the only flat-gradient optimiser launchers (launch_adam, launch_sgd,
// launch_rmsprop and launch_unscale_adam are gone with their kernels).
struct OptimArgs {
  float* theta; const float* grad; float* m; float* v; int64_t n;
  int kind;                           // DMF_OPT_*
  float lr, b1, b2, eps, momentum, alpha, weight_decay, max_norm, grad_scale;
  int32_t step; int32_t* step_dev; int32_t* cursor_dev;
  float* state;                       // nullable loss-scaler state
  float growth, backoff; int interval, unscaled;
  float* norm_hist;                   // nullable: norm_hist[*cursor_dev] = the pre-clip norm
  float bc1, bc2_sqrt;                // ADAM's bias corrections formed on the host; bc1 == 0: form them on the device from the step
  int checked;                        // found_inf of this step is already in state[2] (needs state): it alone decides the skip
};
struct OptimSchedArgs : OptimArgs { HpSched hp; };   // ... of optim_step_kernel<KIND, true>: lr, betas / momentum from the step's row
hipError_t launch_unscale_check(float* grad, int64_t n, float grad_scale, float* state, hipStream_t st);
struct OptimAvgArgs : OptimSchedArgs { AvgArgs av; };  // ... of optim_step_kernel<KIND, SCHED, true> (hp read when SCHED)
// hp: the schedule instance; av: the averaging instance
hipError_t launch_optim_step(const OptimArgs& a, hipStream_t st, const HpSched* hp = nullptr, const AvgArgs* av = nullptr);
// avg <- the averaging rule on theta [n], stand-alone (weight_average_kernel); the step count is *step_dev when given, else step
hipError_t launch_weight_average(const AvgArgs& av, const float* theta, int64_t n, int32_t step, const int32_t* step_dev,
                                 hipStream_t st);
hipError_t launch_xgmi_allreduce(const XgmiDev& x, float* buf, int64_t n, int seq, hipStream_t st);
// the validation sum of an epoch and what its end decides (dmf_valid_accum, dmf_keep_best): one workgroup each
hipError_t launch_valid_accum(const float* loss, int n, double* acc, hipStream_t st);
hipError_t launch_keep_best(double* acc, double* best, int32_t* best_epoch, int32_t epoch, const float* theta, float* best_theta,
                            int64_t n, double* val_hist, hipStream_t st);

// stage-2 kernels (dmf_qua.hip)
struct QuaArgs {
  const float* logits; int bs, K;
  const int32_t* labels; const int32_t* cursor;
  float alpha, beta, gamma, eps, tao, grad_scale;
  float* loss; float* loss_hist; float* dlogits;
  const float* scaler;   // nullable: device loss-scaler state, [0] multiplies grad_scale
  // the logits as all_gather_into_tensor leaves them, rank-major [ranks][4][bs_r][K] (bs = ranks * bs_r): global sample
  // g = r * bs_r + i of stream st at row r * 4 * bs_r + st * bs_r + i; dlogits is rank `rank`'s block [4][bs_r][K] only.
  // ranks = 1, rank = 0, bs_r = bs: the stream-major [4][bs][K] of one GPU.
  int ranks, rank, bs_r;
};
hipError_t launch_qua_loss(const QuaArgs& a, hipStream_t st);
hipError_t launch_pair_argmax(const float* logits, int bs, int K, int32_t* pred, hipStream_t st);
hipError_t launch_band_mean(const float* x, int layout, int64_t n_img, int64_t n_pix, int C, float* out, hipStream_t st);
hipError_t launch_confusion(const int32_t* pred, const int32_t* target, int B, int K, unsigned long long* matrix, hipStream_t st);
hipError_t launch_labelmap(const int32_t* pred, const int32_t* xy, int B, int W, int32_t* map, hipStream_t st);

// calibrated confidence (dmf_calib.hip)
struct SoftmaxStatsArgs {
  const float* logits; int B, K;
  const float* inv_temp;   // nullable device [1]: beta = 1 / T (NULL: 1)
  const int32_t* xy; int W;   // nullable [B][2]: row i writes index x * W + y instead of i
  int32_t* pred; float* conf; float* margin; float* entropy;   // each nullable
};
hipError_t launch_softmax_stats(const SoftmaxStatsArgs& a, hipStream_t st);
hipError_t launch_calib_accum(const float* conf, const int32_t* pred, const int32_t* target, int B, int K, int nbins,
                              unsigned long long* hist, hipStream_t st);
hipError_t launch_temperature_init(double* state, hipStream_t st);
// partial: [(N + 255) / 256][3] doubles (dmf_temperature_workspace_bytes)
hipError_t launch_temperature_step(const float* logits, const int32_t* labels, int N, int K, double* state, double* partial,
                                   int update, hipStream_t st);

// per-sample classification losses of the unit-gradient step (dmf_loss.hip)
struct CeArgs {
  const float* logits;   // [bs_r][K], this rank's rows
  const int32_t* labels; const int32_t* cursor;   // labels[(*cursor) * ranks * bs_r + r * bs_r + i]: the GLOBAL batch, rank-major
  const float* class_w;  // [K], nullable = all ones
  const float* scaler;   // nullable: device loss-scaler state, [0] multiplies grad_scale
  float* loss;           // [bs_r] nullable
  float* dlogits;        // [bs_r][K] nullable
  int ranks, rank, bs_r, K, kind;
  float eps, gamma, grad_scale;
};
hipError_t launch_ce_loss(const CeArgs& a, hipStream_t st);
// denom[r] = sum over the N labels of row r of (double)class_w[label] (NULL: ones), the bits ce_loss_kernel forms for that row
hipError_t launch_ce_denominators(const int32_t* labels, int N, int rows, int K, const float* class_w, double* denom, hipStream_t st);

// scene preparation (dmf_scene.hip)
struct ScenePrepArgs {
  const void* raw; const void* minmax; void* out;
  int H, W, C, pad;
  int row;           // elements of one padded output row, (W + pad) * C
  int shift;         // elements by which `out` lies past a 16-byte boundary
  int64_t n_out;     // (H + pad) * row
  double inv_row;    // 1 / row
};
int scene_raw_bytes(int dtype);      // element size of a DMF_RAW_* code, 0 for an unknown one
hipError_t launch_scene_minmax(const void* raw, int dtype, int64_t n, void* minmax, hipStream_t st);
hipError_t launch_scene_prepare(const ScenePrepArgs& a, int dtype, int half, hipStream_t st);
hipError_t launch_pan2ms(const double* pan, int pitch, int H, int W, double* out, hipStream_t st);

#ifdef DMF_STAMPS
hipError_t set_attn_stamps(unsigned long long* p);
hipError_t set_v2_stamps(unsigned long long* p);
hipError_t set_reduce_stamps(unsigned long long* p);
#endif

}  // namespace dmf
