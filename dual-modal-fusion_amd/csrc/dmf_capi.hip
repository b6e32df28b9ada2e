// dmf_capi.hip — the extern "C" entry points of libdmf_hip.so (declared in include/dmf.h).  Host code only: an entry point
// checks its arguments, carves its workspace, fills an argument struct of dmf_kargs.h and calls the launcher of the kernel
// file that owns the kernel.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "dmf_kargs.h"

namespace dmf {

static thread_local char g_err[512] = "";

static int fail(const char* fmt, const char* detail) {
  snprintf(g_err, sizeof(g_err), fmt, detail);
  return 1;
}
static int check(hipError_t e, const char* what) {
  if (e == hipSuccess) return 0;
  snprintf(g_err, sizeof(g_err), "%s: %s", what, hipGetErrorString(e));
  return 1;
}

static Layout layout_of(const dmf_shape& s) {
  return make_layout(s.C, s.C2, s.P, s.S, s.F, s.G, s.H, s.K, s.attention, s.E);
}

}  // namespace dmf

using namespace dmf;

// the conv launches of the attention network (MODE_TOKENS, MODE_DENSE)
static hipError_t conv_dispatch(const dmf_shape& s, int mode, const KArgs& a, hipStream_t st) {
  if (!patch_v2_supported(s, mode)) return hipErrorInvalidValue;
  return patch_v2_dispatch(s, mode, a, st);
}

// the batch and the patch source of a dmf_input; an empty batch passes (its tensors have null data pointers) and the caller
// returns before it looks at them
static int check_input(const dmf_input* in) {
  if (in->B < 0) return fail("%s", "negative batch");
  if (in->B == 0) return 0;
  if (in->mode == 0 && (in->a == nullptr || in->b == nullptr)) return fail("%s", "mode 0 needs a and b");
  if (in->mode == 1 && (in->sceneA == nullptr || in->sceneB == nullptr || in->xy == nullptr || in->Wp <= 0 || in->WpB <= 0))
    return fail("%s", "mode 1 needs sceneA, sceneB, xy, Wp, WpB");
  if (in->mode != 0 && in->mode != 1) return fail("%s", "input mode must be 0 or 1");
  return 0;
}

// the head vectors of the gradient reduce inside the workspace (KArgs and AttnTrainArgs name them alike)
template <class Args>
static void head_ws(float* ws, const WsLayout& w, Args& a) {
  a.ws_z = ws + w.z;
  a.ws_h = ws + w.h;
  a.ws_dh = ws + w.dh;
  a.ws_dl = ws + w.dl;
}

// The attention workspace, in order: two bf16 token maps and the pooled z per patch, for training the two dense gradient maps
// [B][F][P][RS], then the bf16 weight copies of every head.  base == nullptr: only `bytes` means anything.
struct AttnWs {
  unsigned short* tokA; unsigned short* tokB; float* z; float* dYa; float* dYb; unsigned short* wprep;
  int64_t bytes;
};
static AttnWs attn_ws(const dmf_shape& s, int64_t B, bool train, void* base) {
  constexpr int64_t TOKMAP = 128 * 64 * 2;                      // one token map: 128 tokens x 64 channels, bf16
  const int64_t RS = (s.P + 3) & ~3;                            // a gradient map's row, padded to 16 bytes
  const int64_t map = train ? (int64_t)s.F * s.P * RS * 4 : 0;
  const int64_t size[6] = {B * TOKMAP, B * TOKMAP, B * 2 * s.F * 4, B * map, B * map, (int64_t)attn_prep_bytes()};
  void* p[6];
  int64_t o = 0;
  for (int i = 0; i < 6; ++i) {
    p[i] = base != nullptr ? static_cast<char*>(base) + o : nullptr;
    o += size[i];
  }
  return AttnWs{static_cast<unsigned short*>(p[0]), static_cast<unsigned short*>(p[1]), static_cast<float*>(p[2]),
                static_cast<float*>(p[3]), static_cast<float*>(p[4]), static_cast<unsigned short*>(p[5]), o};
}

// What dmf_forward_attn and dmf_train_attn_fwd_bwd (`entry`) share behind their null checks: the remaining refusals, the
// workspace, the weight prep and token launches, and the fields of AttnTrainArgs that both kernels read.
static int attn_common(const char* entry, const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                       void* attn_workspace, bool train, float* logits, hipStream_t st, AttnWs& w, AttnTrainArgs& t) {
  if (!s->attention) return fail("%s needs shape->attention == 1", entry);
  if (in->half) return fail("%s", "fp16 scenes (dmf_input.half): late-fusion network only");
  if (dmf_shape_supported(s)) return 1;
  if (!attn_shape_supported(*s)) return fail("%s", "no compiled attention instance for this shape (E = 96, heads = 3, F = 40)");
  if (in->B < 0) return fail("%s", "negative batch");
  const Layout L = layout_of(*s);
  w = attn_ws(*s, in->B, train, attn_workspace);
  if (check(attn_prep_launch(theta, L.off[12], L.off[13], L.off[14], L.off[15], w.wprep, st), "attention weight prep launch")) return 1;
  KArgs a{};
  a.in = *in; a.theta = theta; a.pool = pool_w; a.K = s->K;
  a.tokA = w.tokA; a.tokB = w.tokB; a.zout = w.z;
  if (check(conv_dispatch(*s, MODE_TOKENS, a, st), "token kernel launch")) return 1;
  t.tokA = w.tokA; t.tokB = w.tokB; t.zin = w.z; t.theta = theta; t.pool = pool_w; t.logits = logits; t.wprep = w.wprep;
  t.oWq = L.off[12]; t.oWk = L.off[13]; t.oWv = L.off[14]; t.oWo = L.off[15];
  t.oFc1w = L.off[8]; t.oFc1b = L.off[9]; t.oFc2w = L.off[10]; t.oFc2b = L.off[11];
  t.B = in->B; t.K = s->K;
  return 0;
}

// bias corrections of Adam's step `step`, in double like torch's host-side scalars
static void host_bias_corrections(float b1, float b2, int32_t step, float* bc1, float* bc2_sqrt) {
  *bc1 = (float)(1.0 - pow((double)b1, (double)step));
  *bc2_sqrt = (float)sqrt(1.0 - pow((double)b2, (double)step));
}

// dmf_adam_step, dmf_sgd_step, dmf_rmsprop_step and dmf_unscale_adam are optim_step_kernel with neutral keys (weight decay 0,
// max_norm 0): what they share of its arguments.  (The kernel writes *step_dev only where a scaler step is skipped.)
static OptimArgs plain_step(int kind, float* theta, const float* grad, float* m, float* v, int64_t n, float lr, float grad_scale,
                            int32_t step, const int32_t* step_dev, int32_t* cursor_dev) {
  OptimArgs a{};
  a.theta = theta; a.grad = grad; a.m = m; a.v = v; a.n = n; a.kind = kind; a.lr = lr; a.grad_scale = grad_scale;
  a.step = step; a.step_dev = const_cast<int32_t*>(step_dev); a.cursor_dev = cursor_dev;
  return a;
}

// the schedule of a *_sched entry point (`entry`) -> the kernels' words; a NULL schedule or table and rows < 1 are refused
static int fill_sched(const char* entry, const dmf_hp_schedule* sc, HpSched& hp) {
  if (sc == nullptr || sc->table == nullptr) return fail("%s: null schedule or table", entry);
  if (sc->rows < 1) return fail("%s: a schedule needs rows >= 1", entry);
  hp.table = sc->table; hp.row_dev = sc->row_dev; hp.rows = sc->rows;
  return 0;
}

// the averaged copy of an *_avg entry point (`entry`) -> the kernels' words; refused: a NULL struct or vector, an unknown
// kind, an EMA weight outside (0, 1], start < 1, reserved != 0, and avg [n] overlapping theta [n]
static int fill_avg(const char* entry, const dmf_weight_avg* w, const float* theta, int64_t n, AvgArgs& av) {
  if (w == nullptr || w->avg == nullptr) return fail("%s: null dmf_weight_avg or avg", entry);
  if (w->kind != DMF_AVG_EMA && w->kind != DMF_AVG_MEAN) return fail("%s: unknown averaging kind (DMF_AVG_EMA, DMF_AVG_MEAN)", entry);
  if (w->kind == DMF_AVG_EMA && !(isfinite(w->weight) && w->weight > 0.f && w->weight <= 1.f))
    return fail("%s: the EMA weight (1 - decay) must lie in (0, 1]", entry);
  if (w->start < 1) return fail("%s: the first averaged step must be >= 1", entry);
  if (w->reserved != 0) return fail("%s: dmf_weight_avg.reserved must be 0", entry);
  if (theta != nullptr && n > 0 && w->avg < theta + n && theta < w->avg + n) return fail("%s: avg overlaps theta", entry);
  av.avg = w->avg; av.kind = w->kind; av.w = w->weight; av.start = w->start;
  return 0;
}

extern "C" {

int32_t dmf_version(void) { return DMF_VERSION; }
const char* dmf_last_error(void) { return g_err; }

int32_t dmf_shape_supported(const dmf_shape* s) {
  if (s == nullptr) return fail("%s", "null shape");
  if (s->attention ? (patch_v2_supported(*s, MODE_TOKENS) && attn_shape_supported(*s)) : patch_v2_supported(*s, MODE_TRAIN)) return 0;
  snprintf(g_err, sizeof(g_err),
           "no compiled kernel instance for C=%d C2=%d P=%d S=%d F=%d G=%d H=%d K=%d attention=%d; compiled (C/C2/P/S/F/G):%s "
           "(K <= 64, subject to 160 KiB of LDS at this K; attention: 200/1/11/1/40/10 and 8/1/5/1/40/2 with E = 96, 3 heads); "
           "`python dual-modal-fusion_amd/build.py --shapes FILE` adds rows",
           s->C, s->C2, s->P, s->S, s->F, s->G, s->H, s->K, s->attention, patch_v2_shape_list());
  return 1;
}

int32_t dmf_patch_variant(const dmf_shape* s, int32_t mode) {   // the same decision as run_patch / dmf_shape_supported
  if (s == nullptr) return 0;
  return patch_v2_supported(*s, mode) ? 2 : 0;
}

int32_t dmf_param_layout(const dmf_shape* s, int64_t offsets[17]) {
  if (s == nullptr || offsets == nullptr) return fail("%s", "null argument");
  const Layout L = layout_of(*s);
  for (int i = 0; i < 17; ++i) offsets[i] = L.off[i];
  return 0;
}

int64_t dmf_workspace_bytes(const dmf_shape* s, int32_t B) {
  if (s == nullptr || B < 0) return -1;
  const Layout L = layout_of(*s);
  return make_ws(L, B).total * 4;
}

static int run_patch(const dmf_shape* s, const dmf_input* in, int mode, const float* theta, const float* pool_w,
                     const int32_t* labels, const float* dlogits, float loss_scale, float* logits, float* loss,
                     int32_t* pred, void* workspace, int32_t* adam_step, void* stream, const float* scaler = nullptr) {
  if (s == nullptr || in == nullptr || theta == nullptr || pool_w == nullptr) return fail("%s", "null argument");
  if (dmf_shape_supported(s)) return 1;
  if (s->attention) return fail("%s", "attention network: use dmf_forward_attn / dmf_train_attn_fwd_bwd");
  if (in->half && dmf_half_supported(s)) return 1;
  if (check_input(in)) return 1;
  if (in->B == 0) return 0;
  KArgs a{};
  a.in = *in;
  a.theta = theta;
  a.pool = pool_w;
  a.labels = labels;
  a.dlogits = dlogits;
  a.loss_scale = loss_scale;
  a.scaler = scaler;
  a.logits = logits;
  a.loss = loss;
  a.pred = pred;
  a.adam_step = adam_step;
  a.K = s->K;
  if (mode != MODE_FWD) {
    if (workspace == nullptr) return fail("%s", "null workspace");
    const Layout L = layout_of(*s);
    const WsLayout w = make_ws(L, in->B);
    float* ws = static_cast<float*>(workspace);
    a.slab = ws + w.slab;
    head_ws(ws, w, a);
  }
  // (S > 1: the aux patch image is fetched in 16-byte LDS-DMA pieces whose source addresses are only dword aligned when the
  // aux row pitch is not a multiple of 4 floats — the reference pads a 1024-wide PAN to 1087; the buffer loads take that:
  // tests/test_gpu_parity.py::test_aux_scene_pitch_not_a_multiple_of_four)
  if (!patch_v2_supported(*s, mode, in->half)) return fail("%s", "no compiled kernel instance for this shape / mode (dmf_shape_supported names the rows)");
  return check(patch_v2_dispatch(*s, mode, a, static_cast<hipStream_t>(stream)), "patch kernel launch");
}

int64_t dmf_attn_workspace_bytes(const dmf_shape* s, int32_t B) {
  if (s == nullptr || B < 0) return -1;
  return attn_ws(*s, B, false, nullptr).bytes;
}

int32_t dmf_forward_attn(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                         void* workspace, float* logits, int32_t* pred, void* stream) {
  if (in != nullptr && in->B == 0) return 0;
  if (s == nullptr || in == nullptr || theta == nullptr || pool_w == nullptr || workspace == nullptr || logits == nullptr)
    return fail("%s", "null argument");
  hipStream_t st = static_cast<hipStream_t>(stream);
  AttnWs aw;
  AttnTrainArgs t{};
  if (attn_common("dmf_forward_attn", s, in, theta, pool_w, workspace, false, logits, st, aw, t)) return 1;
  t.pred = pred;
  const int grid = in->B < 2 * MAX_BLOCKS ? in->B : 2 * MAX_BLOCKS;
  return check(attn_forward_dispatch(*s, t, grid, st), "attention kernel launch");
}

int64_t dmf_attn_train_workspace_bytes(const dmf_shape* s, int32_t B) {
  if (s == nullptr || B < 0) return -1;
  return attn_ws(*s, B, true, nullptr).bytes;
}

// The train step of the attention network behind dmf_train_attn_fwd_bwd and dmf_train_attn_fwd_bwd_ce (`entry`), whose own
// arguments the caller has checked: token kernel, attention fwd+bwd kernel, conv backward.  ce == nullptr: the plain instance
// with `labels` (this rank's) or `dlogits`; else the criterion instance, `labels` = ce->labels_global.
static int attn_train_step(const char* entry, const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                           const int32_t* labels, const float* dlogits, float loss_scale, const dmf_ce_fused* ce, float* logits,
                           float* loss, void* workspace, void* attn_workspace, int32_t* adam_step_dev, hipStream_t st) {
  AttnWs aw;
  AttnTrainArgs t{};
  if (attn_common(entry, s, in, theta, pool_w, attn_workspace, true, logits, st, aw, t)) return 1;
  const WsLayout w = make_ws(layout_of(*s), in->B);
  float* ws = static_cast<float*>(workspace);
  t.labels = labels; t.cursor = in->cursor; t.dlogits = dlogits; t.loss_scale = loss_scale; t.loss = loss;
  head_ws(ws, w, t);
  t.dYa = aw.dYa; t.dYb = aw.dYb; t.aslab = ws + w.aslab;
  const int grid = in->B < MAX_BLOCKS ? in->B : MAX_BLOCKS;          // one slab per workgroup, as the conv kernel
  if (ce != nullptr) {
    const dmf_ce_params* p = ce->params;
    t.class_w = ce->class_w; t.denom = ce->denom; t.ranks = ce->ranks; t.rank = ce->rank; t.kind = p->kind;
    t.eps = p->kind == 0 ? p->label_smoothing : 0.f; t.gamma = p->kind == 1 ? p->gamma : 0.f; t.grad_scale = ce->grad_scale;
    t.loss = nullptr;                                  // (the value: the launch behind the conv backward)
    if (check(attn_train_ce_dispatch(*s, t, grid, st), "attention training kernel launch")) return 1;
  } else if (check(attn_train_dispatch(*s, t, grid, st), "attention training kernel launch")) {
    return 1;
  }
  KArgs d{};
  d.in = *in; d.theta = theta; d.pool = pool_w; d.K = s->K;
  d.slab = ws + w.slab; d.dYa = aw.dYa; d.dYb = aw.dYb; d.adam_step = adam_step_dev;
  if (check(conv_dispatch(*s, MODE_DENSE, d, st), "dense conv backward launch")) return 1;
  if (ce == nullptr || loss == nullptr) return 0;
  // The per-patch value N t_i / D: ce_loss_kernel, value only, on the logits the attention kernel stored — the float64
  // arithmetic of the value does not fit the attention kernel's registers.  Behind the conv backward, which
  // the gradient reduce waits for; nothing but the loss history reads `loss`.
  CeArgs v{logits, labels, in->cursor, ce->class_w, nullptr, loss, nullptr, ce->ranks, ce->rank, in->B, s->K, t.kind, t.eps, t.gamma,
           ce->grad_scale};
  return check(launch_ce_loss(v, st), "ce_loss (value) launch");
}

int32_t dmf_train_attn_fwd_bwd(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                               const int32_t* labels, const float* dlogits, float loss_scale, float* logits, float* loss,
                               void* workspace, void* attn_workspace, int32_t* adam_step_dev, void* stream) {
  if (in != nullptr && in->B == 0) return 0;
  if (s == nullptr || in == nullptr || theta == nullptr || pool_w == nullptr || workspace == nullptr ||
      attn_workspace == nullptr || logits == nullptr)
    return fail("%s", "null argument");
  if ((labels == nullptr) == (dlogits == nullptr)) return fail("%s", "give exactly one of labels / dlogits");
  return attn_train_step("dmf_train_attn_fwd_bwd", s, in, theta, pool_w, labels, dlogits, loss_scale, nullptr, logits, loss, workspace,
                         attn_workspace, adam_step_dev, static_cast<hipStream_t>(stream));
}

// what dmf_ce_loss and dmf_train_attn_fwd_bwd_ce (`entry`) refuse of a criterion and of the place of a rank in the global batch
static int check_ce(const char* entry, const dmf_ce_params* prm, int32_t ranks, int32_t rank, int32_t bs_r, int32_t K) {
  if (ranks < 1 || rank < 0 || rank >= ranks) return fail("%s: ranks must be positive and 0 <= rank < ranks", entry);
  if (bs_r <= 0 || K < 1 || K > KMAX) return fail("%s: bs must be positive and 1 <= K <= DMF_KMAX", entry);
  if ((int64_t)ranks * bs_r > INT32_MAX || (int64_t)bs_r * K > INT32_MAX) return fail("%s: the batch is too large", entry);
  if (prm->kind != 0 && prm->kind != 1) return fail("%s: kind must be 0 (cross-entropy) or 1 (focal)", entry);
  if (!(prm->label_smoothing >= 0.f && prm->label_smoothing < 1.f)) return fail("%s: label_smoothing must lie in [0, 1)", entry);
  if (!(prm->gamma == 0.f || (prm->gamma >= 1.f && isfinite(prm->gamma)))) return fail("%s: gamma must be 0 or >= 1", entry);
  return 0;
}

int32_t dmf_train_attn_fwd_bwd_ce(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                                  const dmf_ce_fused* ce, float* logits, float* loss, void* workspace, void* attn_workspace,
                                  int32_t* adam_step_dev, void* stream) {
  if (in != nullptr && in->B == 0) return 0;
  if (s == nullptr || in == nullptr || theta == nullptr || pool_w == nullptr || workspace == nullptr ||
      attn_workspace == nullptr || logits == nullptr)
    return fail("%s", "null argument");
  if (ce == nullptr || ce->params == nullptr || ce->labels_global == nullptr || ce->denom == nullptr)
    return fail("%s", "dmf_train_attn_fwd_bwd_ce: null dmf_ce_fused, params, labels_global or denom");
  if (ce->reserved != 0) return fail("%s", "dmf_train_attn_fwd_bwd_ce: dmf_ce_fused.reserved must be 0");
  if (check_ce("dmf_train_attn_fwd_bwd_ce", ce->params, ce->ranks, ce->rank, in->B, s->K)) return 1;
  return attn_train_step("dmf_train_attn_fwd_bwd_ce", s, in, theta, pool_w, ce->labels_global, nullptr, 0.f, ce, logits, loss,
                         workspace, attn_workspace, adam_step_dev, static_cast<hipStream_t>(stream));
}

int32_t dmf_forward(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                    float* logits, int32_t* pred, void* stream) {
  if (in != nullptr && in->B == 0) return 0;          // an empty batch is a no-op (its tensors have null data pointers)
  if (logits == nullptr) return fail("%s", "null logits");
  if (s != nullptr && s->attention) return fail("%s", "attention network: use dmf_forward_attn");
  return run_patch(s, in, MODE_FWD, theta, pool_w, nullptr, nullptr, 0.f, logits, nullptr, pred, nullptr, nullptr, stream);
}

int32_t dmf_forward_ce(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w, const int32_t* labels,
                       float* logits, float* loss, int32_t* pred, void* stream) {
  if (in != nullptr && in->B == 0) return 0;
  if (logits == nullptr || labels == nullptr || loss == nullptr) return fail("%s", "null logits/labels/loss");
  if (s == nullptr || s->attention || !(in != nullptr && in->half ? patch_v2_supported(*s, MODE_FWD, 1) : patch_v2_supported(*s, MODE_FWD)))
    return fail("%s", "dmf_forward_ce: no evaluation kernel with a fused cross-entropy for this shape (use dmf_forward)");
  return run_patch(s, in, MODE_FWD, theta, pool_w, labels, nullptr, 0.f, logits, loss, pred, nullptr, nullptr, stream);
}

int32_t dmf_train_fwd_bwd(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                          const int32_t* labels, float loss_scale, float* logits, float* loss, void* workspace,
                          int32_t* adam_step_dev, void* stream) {
  if (in != nullptr && in->B == 0) return 0;
  if (labels == nullptr || logits == nullptr || loss == nullptr) return fail("%s", "null labels/logits/loss");
  return run_patch(s, in, MODE_TRAIN, theta, pool_w, labels, nullptr, loss_scale, logits, loss, nullptr, workspace, adam_step_dev, stream);
}

int32_t dmf_train_fwd_bwd_scaled(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                                 const int32_t* labels, float loss_scale, const float* scaler_state, float* logits,
                                 float* loss, void* workspace, int32_t* adam_step_dev, void* stream) {
  if (in != nullptr && in->B == 0) return 0;
  if (labels == nullptr || logits == nullptr || loss == nullptr || scaler_state == nullptr)
    return fail("%s", "null labels/logits/loss/scaler_state");
  return run_patch(s, in, MODE_TRAIN, theta, pool_w, labels, nullptr, loss_scale, logits, loss, nullptr, workspace,
                   adam_step_dev, stream, scaler_state);
}

int32_t dmf_scaler_init(float* state, float init_scale, void* stream) {
  if (state == nullptr || !(init_scale > 0.f)) return fail("%s", "scaler: null state or non-positive scale");
  const float h[DMF_SCALER_FLOATS] = {init_scale, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (check(hipMemcpyAsync(state, h, sizeof(h), hipMemcpyHostToDevice, st), "scaler init")) return 1;
  return check(hipStreamSynchronize(st), "scaler init");       // (h is a stack buffer)
}

int32_t dmf_unscale_adam(float* theta, float* grad, float* m, float* v, int64_t n, float lr, float beta1, float beta2,
                         float eps, float grad_scale, float* scaler_state, float growth_factor, float backoff_factor,
                         int32_t growth_interval, int32_t unscaled, int32_t* adam_step_dev, int32_t* cursor_dev, void* stream) {
  if (theta == nullptr || grad == nullptr || m == nullptr || v == nullptr || scaler_state == nullptr || adam_step_dev == nullptr)
    return fail("%s", "null argument (dmf_unscale_adam needs the device step count)");
  if (n <= 0 || growth_interval < 1 || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f))
    return fail("%s", "unscale_adam: bad n / growth_interval / factors");
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (!unscaled && check(launch_unscale_check(grad, n, grad_scale, scaler_state, st), "unscale launch")) return 1;
  // grad is unscaled in memory by now and found_inf is in state[2]: the kernel takes it as it is and closes the scaler's step
  OptimArgs a = plain_step(DMF_OPT_ADAM, theta, grad, m, v, n, lr, 1.f, 0, adam_step_dev, cursor_dev);
  a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  a.state = scaler_state; a.growth = growth_factor; a.backoff = backoff_factor; a.interval = growth_interval;
  a.unscaled = 1; a.checked = 1;
  return check(launch_optim_step(a, st), "scaled adam launch");
}

int32_t dmf_half_supported(const dmf_shape* s) {
  if (s == nullptr) return fail("%s", "null shape");
  if (s->attention || !patch_v2_supported(*s, MODE_TRAIN, 1))
    return fail("no fp16-scene kernel for this shape (instances C/C2/P/S/F/G:%s)", patch_v2_half_shape_list());
  return 0;
}

int32_t dmf_unit_supported(const dmf_shape* s) {
  if (s == nullptr) return fail("%s", "null shape");
  if (s->attention || !patch_v2_supported(*s, MODE_UNIT))
    return fail("no unit-gradient kernel for this shape (instances C/C2/P/S/F/G:%s)", patch_v2_shape_list());
  return 0;
}

int32_t dmf_forward_unit(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w, float* logits,
                         void* workspace, int32_t* adam_step_dev, void* stream) {
  if (s == nullptr || in == nullptr || theta == nullptr || pool_w == nullptr || logits == nullptr || workspace == nullptr)
    return fail("%s", "null argument");
  if (dmf_unit_supported(s)) return 1;
  if (in->half && dmf_half_supported(s)) return 1;
  if (check_input(in)) return 1;
  if (in->B == 0) return 0;
  const Layout L = layout_of(*s);
  const WsLayout w = make_ws(L, in->B);
  float* ws = static_cast<float*>(workspace);
  KArgs a{};
  a.in = *in;
  a.theta = theta;
  a.pool = pool_w;
  a.logits = logits;
  a.adam_step = adam_step_dev;
  a.K = s->K;
  a.slab = ws + w.unit;          // MODE_UNIT: one row per patch
  head_ws(ws, w, a);
  return check(patch_v2_dispatch(*s, MODE_UNIT, a, static_cast<hipStream_t>(stream)), "patch kernel (v2, unit) launch");
}

int32_t dmf_backward_unit(const dmf_shape* s, int32_t B, const float* theta, const float* dlogits, void* workspace,
                          void* stream) {
  if (s == nullptr || theta == nullptr || dlogits == nullptr || workspace == nullptr) return fail("%s", "null argument");
  if (dmf_unit_supported(s)) return 1;
  if (B < 0) return fail("%s", "negative batch");
  if (B == 0) return 0;
  const Layout L = layout_of(*s);
  const WsLayout w = make_ws(L, B);
  float* ws = static_cast<float*>(workspace);
  UnitBwdArgs a{theta, dlogits, ws + w.unit, ws + w.h, ws + w.dh, ws + w.dl, ws + w.slab, B, s->K};
  return check(patch_v2_unit_backward(*s, a, static_cast<hipStream_t>(stream)), "unit backward launch");
}

int32_t dmf_backward_dlogits(const dmf_shape* s, const dmf_input* in, const float* theta, const float* pool_w,
                             const float* dlogits, void* workspace, void* stream) {
  if (in != nullptr && in->B == 0) return 0;
  if (dlogits == nullptr) return fail("%s", "null dlogits");
  return run_patch(s, in, MODE_BWD, theta, pool_w, nullptr, dlogits, 1.f, nullptr, nullptr, nullptr, workspace, nullptr, stream);
}

static int fill_xgmi(const dmf_xgmi_comm* c, XgmiDev& x) {
  if (c->world < 2 || c->world > XGMI_MAX || c->rank < 0 || c->rank >= c->world) return fail("%s", "bad xgmi world/rank");
  if (c->capacity <= 0) return fail("%s", "bad xgmi capacity");
  x.world = c->world; x.rank = c->rank;
  x.cap = (c->capacity + 255) / 256 * 256;
  x.timeout_ticks = (int64_t)(c->timeout_ms > 0 ? c->timeout_ms : 20000) * 100000;   // wall_clock64 runs at 100 MHz
  for (int r = 0; r < c->world; ++r) {
    if (c->data[r] == nullptr || c->flags[r] == nullptr) return fail("%s", "xgmi peer buffer missing");
    x.data[r] = static_cast<unsigned long long*>(c->data[r]);
    x.flags[r] = static_cast<int32_t*>(c->flags[r]);
  }
  return 0;
}

// what a reduce launch does beyond summing: every entry point fills only what it uses
struct ReduceOpts {
  float* grad = nullptr;                       // where the summed gradient goes (optional with Adam)
  float* theta = nullptr; float* m = nullptr; float* v = nullptr;   // the fused Adam (theta == nullptr: reduce only)
  float lr = 0.f, b1 = 0.f, b2 = 0.f, eps = 0.f;
  int32_t step = 0;                            // host step count, used when step_dev == nullptr
  const int32_t* step_dev = nullptr;
  int32_t* cursor_dev = nullptr;
  const float* loss = nullptr; float* loss_hist = nullptr;
  const dmf_xgmi_comm* comm = nullptr;         // exchange the gradient with the peer ranks before Adam
  float grad_scale = 1.f;
  float* scaler = nullptr;                     // loss-scaler state: unscale and check the sum
  const dmf_hp_schedule* sched = nullptr;      // the fused Adam takes lr, b1, b2 from its row (the *_sched entry points)
  const dmf_weight_avg* avg = nullptr;         // the fused Adam keeps the averaged copy (the *_avg entry points)
};

static int run_reduce(const dmf_shape* s, int32_t B, const void* workspace, const ReduceOpts& o, void* stream) {
  if (s == nullptr || workspace == nullptr) return fail("%s", "null argument");
  if (B <= 0) return fail("%s", "batch must be positive");
  if (o.comm != nullptr && o.step_dev == nullptr) return fail("%s", "the xgmi exchange needs adam_step_dev");
  const Layout L = layout_of(*s);
  const float* ws = static_cast<const float*>(workspace);
  ReduceArgs a{};
  a.B = B; a.NCONV = L.NCONV; a.F2 = L.F2; a.H = L.H; a.K = L.K;
  a.oFc1w = L.off[8]; a.oFc1b = L.off[9]; a.oFc2w = L.off[10]; a.oFc2b = L.off[11];
  a.aslab = ws + make_ws(L, B).aslab; a.nablk = B < MAX_BLOCKS ? B : MAX_BLOCKS; a.ASLAB = 4 * L.E * L.F;
  a.oAttn = L.attention ? L.off[12] : L.n_params;
  a.grad = o.grad; a.theta = o.theta; a.m = o.m; a.v = o.v;
  a.lr = o.lr; a.b1 = o.b1; a.b2 = o.b2; a.eps = o.eps;
  if (o.theta != nullptr) {
    if (o.m == nullptr || o.v == nullptr || (o.step < 1 && o.step_dev == nullptr)) return fail("%s", "Adam needs m, v and step >= 1");
    // (with a schedule the row's betas are on the device: the kernel forms the corrections)
    if (o.sched == nullptr && o.step_dev == nullptr) host_bias_corrections(o.b1, o.b2, o.step, &a.bc1, &a.bc2_sqrt);
  }
  a.step_dev = o.step_dev; a.cursor_dev = o.cursor_dev; a.loss = o.loss; a.loss_hist = o.loss_hist;
  a.grad_scale = o.grad_scale;
  a.scaler = o.scaler;
  if (o.comm != nullptr) {
    if (o.comm->capacity < L.n_params) return fail("%s", "xgmi communicator smaller than the parameter vector");
    if (fill_xgmi(o.comm, a.x)) return 1;
    a.seq_bias = o.comm->seq_bias;
  }
  HpSched hp{};
  if (o.sched != nullptr && fill_sched("grad_reduce_adam_sched", o.sched, hp)) return 1;
  AvgArgs av{};
  if (o.avg != nullptr) {
    if (o.theta == nullptr || o.comm != nullptr) return fail("%s", "grad_reduce_adam_avg: needs theta, and has no xgmi form");
    if (fill_avg("grad_reduce_adam_avg", o.avg, o.theta, L.n_params, av)) return 1;
  }
  const char* refusal = nullptr;
  const hipError_t e = launch_grad_reduce(a, L, B, ws, static_cast<hipStream_t>(stream), &refusal, o.sched != nullptr ? &hp : nullptr,
                                          o.step, o.avg != nullptr ? &av : nullptr);
  return refusal != nullptr ? fail("%s", refusal) : check(e, "grad_reduce launch");
}

// the fused Adam of the reduce, its step count on the host (step) or on the device (step_dev)
static ReduceOpts adam_opts(float* theta, float* m, float* v, float lr, float b1, float b2, float eps, int32_t step,
                            const int32_t* step_dev, int32_t* cursor_dev, const float* loss, float* loss_hist) {
  ReduceOpts o;
  o.theta = theta; o.m = m; o.v = v;
  o.lr = lr; o.b1 = b1; o.b2 = b2; o.eps = eps;
  o.step = step; o.step_dev = step_dev; o.cursor_dev = cursor_dev;
  o.loss = loss; o.loss_hist = loss_hist;
  return o;
}

int32_t dmf_grad_reduce(const dmf_shape* s, int32_t B, const void* workspace, float* grad, void* stream) {
  if (grad == nullptr) return fail("%s", "null grad");
  ReduceOpts o;
  o.grad = grad;
  return run_reduce(s, B, workspace, o, stream);
}

int32_t dmf_grad_reduce_scaled(const dmf_shape* s, int32_t B, const void* workspace, float* grad, float* scaler_state,
                               int32_t* cursor_dev, const float* loss, float* loss_hist, void* stream) {
  if (grad == nullptr || scaler_state == nullptr) return fail("%s", "null grad / scaler_state");
  ReduceOpts o;
  o.grad = grad; o.scaler = scaler_state;
  o.cursor_dev = cursor_dev; o.loss = loss; o.loss_hist = loss_hist;
  return run_reduce(s, B, workspace, o, stream);
}

int32_t dmf_grad_reduce_adam(const dmf_shape* s, int32_t B, const void* workspace, float* theta, float* m, float* v,
                             float* grad, float lr, float beta1, float beta2, float eps, int32_t step,
                             const int32_t* adam_step_dev, int32_t* cursor_dev, const float* loss, float* loss_hist,
                             void* stream) {
  if (theta == nullptr) return fail("%s", "null theta");
  ReduceOpts o = adam_opts(theta, m, v, lr, beta1, beta2, eps, step, adam_step_dev, cursor_dev, loss, loss_hist);
  o.grad = grad;
  return run_reduce(s, B, workspace, o, stream);
}

int32_t dmf_grad_reduce_adam_sched(const dmf_shape* s, int32_t B, const void* workspace, float* theta, float* m, float* v,
                                   float* grad, const dmf_hp_schedule* sched, float eps, int32_t step,
                                   const int32_t* adam_step_dev, int32_t* cursor_dev, const float* loss, float* loss_hist,
                                   void* stream) {
  if (theta == nullptr) return fail("%s", "null theta");
  HpSched hp{};
  if (fill_sched("grad_reduce_adam_sched", sched, hp)) return 1;
  ReduceOpts o = adam_opts(theta, m, v, 0.f, 0.f, 0.f, eps, step, adam_step_dev, cursor_dev, loss, loss_hist);
  o.grad = grad; o.sched = sched;
  return run_reduce(s, B, workspace, o, stream);
}

int32_t dmf_grad_reduce_adam_avg(const dmf_shape* s, int32_t B, const void* workspace, float* theta, float* m, float* v,
                                 float* grad, float lr, float beta1, float beta2, float eps, int32_t step,
                                 const int32_t* adam_step_dev, int32_t* cursor_dev, const float* loss, float* loss_hist,
                                 const dmf_hp_schedule* sched, const dmf_weight_avg* avg, void* stream) {
  if (theta == nullptr) return fail("%s", "null theta");
  if (avg == nullptr) return fail("%s", "grad_reduce_adam_avg: null dmf_weight_avg or avg");
  ReduceOpts o = sched != nullptr ? adam_opts(theta, m, v, 0.f, 0.f, 0.f, eps, step, adam_step_dev, cursor_dev, loss, loss_hist)
                                  : adam_opts(theta, m, v, lr, beta1, beta2, eps, step, adam_step_dev, cursor_dev, loss, loss_hist);
  o.grad = grad; o.sched = sched; o.avg = avg;
  return run_reduce(s, B, workspace, o, stream);
}

// dmf_train_plan_steps and its schedule form: `adam` holds the launch arguments or the schedule
static int plan_steps(const dmf_shape* s, const dmf_input* in, float* theta, const float* pool_w, const int32_t* labels,
                      float loss_scale, float* logits, float* loss, void* workspace, const ReduceOpts& adam, int32_t n_steps,
                      void* stream) {
  if (s == nullptr || in == nullptr || theta == nullptr || labels == nullptr || logits == nullptr || loss == nullptr ||
      adam.step_dev == nullptr || adam.cursor_dev == nullptr)
    return fail("%s", "null argument (dmf_train_plan_steps needs the device step count and cursor)");
  if (in->mode != 1 || in->cursor != nullptr) return fail("%s", "dmf_train_plan_steps: gather mode, no plan cursor (the batches are consecutive)");
  if (s->attention) return fail("%s", "dmf_train_plan_steps: late-fusion network only");
  if (n_steps < 0 || in->B <= 0) return fail("%s", "dmf_train_plan_steps: negative step count or empty batch");
  int32_t* adam_step_dev = const_cast<int32_t*>(adam.step_dev);
  dmf_input ik = *in;
  for (int32_t k = 0; k < n_steps; ++k) {
    ik.xy = in->xy + (size_t)2 * in->B * k;
    if (run_patch(s, &ik, MODE_TRAIN, theta, pool_w, labels + (size_t)in->B * k, nullptr, loss_scale, logits, loss, nullptr, workspace,
                  adam_step_dev, stream))
      return 1;
    if (run_reduce(s, in->B, workspace, adam, stream)) return 1;
  }
  return 0;
}

int32_t dmf_train_plan_steps(const dmf_shape* s, const dmf_input* in, float* theta, const float* pool_w, const int32_t* labels,
                             float loss_scale, float* logits, float* loss, void* workspace, float* m, float* v, float lr,
                             float beta1, float beta2, float eps, int32_t* adam_step_dev, int32_t* cursor_dev, float* loss_hist,
                             int32_t n_steps, void* stream) {
  return plan_steps(s, in, theta, pool_w, labels, loss_scale, logits, loss, workspace,
                    adam_opts(theta, m, v, lr, beta1, beta2, eps, 0, adam_step_dev, cursor_dev, loss, loss_hist), n_steps, stream);
}

int32_t dmf_train_plan_steps_sched(const dmf_shape* s, const dmf_input* in, float* theta, const float* pool_w,
                                   const int32_t* labels, float loss_scale, float* logits, float* loss, void* workspace, float* m,
                                   float* v, const dmf_hp_schedule* sched, float eps, int32_t* adam_step_dev, int32_t* cursor_dev,
                                   float* loss_hist, int32_t n_steps, void* stream) {
  HpSched hp{};
  if (fill_sched("dmf_train_plan_steps_sched", sched, hp)) return 1;
  ReduceOpts adam = adam_opts(theta, m, v, 0.f, 0.f, 0.f, eps, 0, adam_step_dev, cursor_dev, loss, loss_hist);
  adam.sched = sched;
  return plan_steps(s, in, theta, pool_w, labels, loss_scale, logits, loss, workspace, adam, n_steps, stream);
}

int32_t dmf_train_plan_steps_avg(const dmf_shape* s, const dmf_input* in, float* theta, const float* pool_w, const int32_t* labels,
                                 float loss_scale, float* logits, float* loss, void* workspace, float* m, float* v, float lr,
                                 float beta1, float beta2, float eps, int32_t* adam_step_dev, int32_t* cursor_dev, float* loss_hist,
                                 const dmf_hp_schedule* sched, const dmf_weight_avg* avg, int32_t n_steps, void* stream) {
  HpSched hp{};
  AvgArgs av{};
  if (sched != nullptr && fill_sched("dmf_train_plan_steps_avg", sched, hp)) return 1;
  if (fill_avg("dmf_train_plan_steps_avg", avg, theta, s != nullptr ? layout_of(*s).n_params : 0, av)) return 1;   // (before any launch)
  ReduceOpts adam = sched != nullptr ? adam_opts(theta, m, v, 0.f, 0.f, 0.f, eps, 0, adam_step_dev, cursor_dev, loss, loss_hist)
                                     : adam_opts(theta, m, v, lr, beta1, beta2, eps, 0, adam_step_dev, cursor_dev, loss, loss_hist);
  adam.sched = sched; adam.avg = avg;
  return plan_steps(s, in, theta, pool_w, labels, loss_scale, logits, loss, workspace, adam, n_steps, stream);
}

int32_t dmf_grad_reduce_xgmi_adam(const dmf_shape* s, int32_t B, const void* workspace, float* theta, float* m,
                                  float* v, const dmf_xgmi_comm* comm, float lr, float beta1, float beta2, float eps,
                                  float grad_scale, const int32_t* adam_step_dev, int32_t* cursor_dev,
                                  const float* loss, float* loss_hist, void* stream) {
  if (theta == nullptr || comm == nullptr) return fail("%s", "null theta/comm");
  ReduceOpts o = adam_opts(theta, m, v, lr, beta1, beta2, eps, 0, adam_step_dev, cursor_dev, loss, loss_hist);
  o.comm = comm; o.grad_scale = grad_scale;
  return run_reduce(s, B, workspace, o, stream);
}

// ------------------------------------------------------------------------------ xgmi buffers + small all-reduce
int32_t dmf_xgmi_sizes(int64_t capacity, int32_t world, int64_t* data_bytes, int64_t* flag_bytes) {
  if (capacity <= 0 || world < 1 || world > XGMI_MAX || data_bytes == nullptr || flag_bytes == nullptr)
    return fail("%s", "bad xgmi_sizes argument");
  const int64_t cap = (capacity + 255) / 256 * 256;
  *data_bytes = 4 * cap * world * (int64_t)sizeof(unsigned long long);   // inbox: [region 2][parity 2][src world][cap] tagged words
  *flag_bytes = 16 * (int64_t)sizeof(int32_t);                           // the status word (+ spare)
  return 0;
}

int32_t dmf_xgmi_alloc(int64_t bytes, void** ptr) {
  if (bytes <= 0 || ptr == nullptr) return fail("%s", "bad xgmi_alloc argument");
  void* p = nullptr;
  if (check(hipExtMallocWithFlags(&p, (size_t)bytes, hipDeviceMallocUncached), "hipExtMallocWithFlags(uncached)")) return 1;
  if (check(hipMemset(p, 0, (size_t)bytes), "hipMemset") || check(hipDeviceSynchronize(), "hipDeviceSynchronize")) {
    (void)hipFree(p);
    return 1;
  }
  *ptr = p;
  return 0;
}

int32_t dmf_xgmi_free(void* ptr) { return ptr == nullptr ? 0 : check(hipFree(ptr), "hipFree"); }

int32_t dmf_xgmi_export(void* ptr, uint8_t handle[64]) {
  static_assert(sizeof(hipIpcMemHandle_t) == 64, "HIP IPC handle size");
  if (ptr == nullptr || handle == nullptr) return fail("%s", "null argument");
  hipIpcMemHandle_t h;
  if (check(hipIpcGetMemHandle(&h, ptr), "hipIpcGetMemHandle")) return 1;
  memcpy(handle, &h, 64);
  return 0;
}

int32_t dmf_xgmi_open(const uint8_t handle[64], void** ptr) {
  if (ptr == nullptr || handle == nullptr) return fail("%s", "null argument");
  hipIpcMemHandle_t h;
  memcpy(&h, handle, 64);
  return check(hipIpcOpenMemHandle(ptr, h, hipIpcMemLazyEnablePeerAccess), "hipIpcOpenMemHandle");
}

int32_t dmf_xgmi_close(void* ptr) { return ptr == nullptr ? 0 : check(hipIpcCloseMemHandle(ptr), "hipIpcCloseMemHandle"); }

int32_t dmf_xgmi_status(const dmf_xgmi_comm* c, int32_t* status) {
  if (c == nullptr || status == nullptr) return fail("%s", "null argument");
  XgmiDev x{};
  if (fill_xgmi(c, x)) return 1;
  if (check(hipDeviceSynchronize(), "hipDeviceSynchronize")) return 1;
  return check(hipMemcpy(status, x.flags[x.rank], sizeof(int32_t), hipMemcpyDeviceToHost),
               "hipMemcpy(status)");
}

int32_t dmf_xgmi_allreduce(const dmf_xgmi_comm* c, float* buf, int64_t n, int32_t seq, void* stream) {
  if (c == nullptr || buf == nullptr) return fail("%s", "null argument");
  XgmiDev x{};
  if (fill_xgmi(c, x)) return 1;
  if (n <= 0 || n > x.cap || seq < 1) return fail("%s", "xgmi_allreduce: n must be in [1, capacity], seq >= 1");
  return check(launch_xgmi_allreduce(x, buf, n, seq, static_cast<hipStream_t>(stream)), "xgmi_allreduce launch");
}

int32_t dmf_adam_step(float* theta, const float* grad, float* m, float* v, int64_t n, float lr, float beta1,
                      float beta2, float eps, int32_t step, float grad_scale, const int32_t* adam_step_dev,
                      int32_t* cursor_dev, void* stream) {
  if (theta == nullptr || grad == nullptr || m == nullptr || v == nullptr) return fail("%s", "null argument");
  if (n <= 0 || (step < 1 && adam_step_dev == nullptr)) return fail("%s", "n and step must be positive");
  OptimArgs a = plain_step(DMF_OPT_ADAM, theta, grad, m, v, n, lr, grad_scale, step, adam_step_dev, cursor_dev);
  a.b1 = beta1; a.b2 = beta2; a.eps = eps;
  if (adam_step_dev == nullptr) host_bias_corrections(beta1, beta2, step, &a.bc1, &a.bc2_sqrt);   // (else: the kernel, from the device count)
  return check(launch_optim_step(a, static_cast<hipStream_t>(stream)), "adam launch");
}

int32_t dmf_sgd_step(float* theta, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                     int32_t step, float grad_scale, const int32_t* step_dev, int32_t* cursor_dev, void* stream) {
  if (theta == nullptr || grad == nullptr || (momentum != 0.f && momentum_buf == nullptr)) return fail("%s", "null argument");
  if (n <= 0 || (step < 1 && step_dev == nullptr)) return fail("%s", "n and step must be positive");
  OptimArgs a = plain_step(DMF_OPT_SGD, theta, grad, momentum_buf, nullptr, n, lr, grad_scale, step, step_dev, cursor_dev);
  a.momentum = momentum;
  return check(launch_optim_step(a, static_cast<hipStream_t>(stream)), "sgd launch");
}

int32_t dmf_rmsprop_step(float* theta, const float* grad, float* square_avg, int64_t n, float lr, float alpha, float eps,
                         float grad_scale, int32_t* cursor_dev, void* stream) {
  if (theta == nullptr || grad == nullptr || square_avg == nullptr) return fail("%s", "null argument");
  if (n <= 0) return fail("%s", "n must be positive");
  OptimArgs a = plain_step(DMF_OPT_RMSPROP, theta, grad, square_avg, nullptr, n, lr, grad_scale, 0, nullptr, cursor_dev);
  a.alpha = alpha; a.eps = eps;
  return check(launch_optim_step(a, static_cast<hipStream_t>(stream)), "rmsprop launch");
}

// dmf_optim_step and dmf_optim_step_sched: with a schedule lr, beta1, beta2 and momentum are unused (the row holds them), and
// SGD needs its momentum buffer whatever the row says
static int optim_step(float* theta, const float* grad, float* m, float* v, int64_t n, int32_t kind, float lr, float beta1,
                      float beta2, float eps, float momentum, float alpha, float weight_decay, float max_norm, int32_t step,
                      float grad_scale, int32_t* step_dev, int32_t* cursor_dev, float* scaler_state, float growth_factor,
                      float backoff_factor, int32_t growth_interval, int32_t unscaled, float* norm_hist,
                      const dmf_hp_schedule* sched, void* stream, const dmf_weight_avg* avg = nullptr, bool averaging = false) {
  if (theta == nullptr || grad == nullptr) return fail("%s", "optim_step: null theta or grad");
  if (kind != DMF_OPT_ADAM && kind != DMF_OPT_ADAMW && kind != DMF_OPT_SGD && kind != DMF_OPT_RMSPROP)
    return fail("%s", "optim_step: unknown kind (DMF_OPT_ADAM, _ADAMW, _SGD, _RMSPROP)");
  const bool adam = kind == DMF_OPT_ADAM || kind == DMF_OPT_ADAMW;
  if ((adam && (m == nullptr || v == nullptr)) || (kind == DMF_OPT_RMSPROP && m == nullptr) ||
      (kind == DMF_OPT_SGD && (momentum != 0.f || sched != nullptr) && m == nullptr))
    return fail("%s", "optim_step: null m or v (ADAM / ADAMW need both, RMSprop m, SGD m when momentum != 0)");
  if (n < 0) return fail("%s", "optim_step: negative n");
  if (!(weight_decay >= 0.f) || !isfinite(weight_decay)) return fail("%s", "optim_step: weight_decay must be finite and >= 0");
  if (!isfinite(max_norm)) return fail("%s", "optim_step: max_norm must be finite (<= 0 switches clipping off)");
  if (scaler_state == nullptr) {
    if (growth_factor != 0.f || backoff_factor != 0.f || growth_interval != 0 || unscaled != 0)
      return fail("%s", "optim_step: scaler hyper-parameters (growth, backoff, interval, unscaled) without a scaler state");
    if (step < 1 && step_dev == nullptr) return fail("%s", "optim_step: step must be positive (or step_dev given)");
  } else {
    if (step_dev == nullptr) return fail("%s", "optim_step: a scaler state needs the device step count");
    if (growth_interval < 1 || !(growth_factor >= 1.f) || !(backoff_factor > 0.f && backoff_factor <= 1.f))
      return fail("%s", "optim_step: bad growth_interval / factors");
  }
  AvgArgs av{};
  if (averaging && fill_avg("optim_step_avg", avg, theta, n, av)) return 1;
  if (n == 0) return 0;
  OptimArgs a{theta, grad, m, v, n, kind, lr, beta1, beta2, eps, momentum, alpha, weight_decay, max_norm, grad_scale,
              step, step_dev, cursor_dev, scaler_state, growth_factor, backoff_factor, growth_interval, unscaled != 0, norm_hist};
  HpSched hp{};
  if (sched != nullptr && fill_sched("optim_step_sched", sched, hp)) return 1;
  return check(launch_optim_step(a, static_cast<hipStream_t>(stream), sched != nullptr ? &hp : nullptr, averaging ? &av : nullptr),
               "optim_step launch");
}

int32_t dmf_optim_step(float* theta, const float* grad, float* m, float* v, int64_t n, int32_t kind, float lr, float beta1,
                       float beta2, float eps, float momentum, float alpha, float weight_decay, float max_norm, int32_t step,
                       float grad_scale, int32_t* step_dev, int32_t* cursor_dev, float* scaler_state, float growth_factor,
                       float backoff_factor, int32_t growth_interval, int32_t unscaled, float* norm_hist, void* stream) {
  return optim_step(theta, grad, m, v, n, kind, lr, beta1, beta2, eps, momentum, alpha, weight_decay, max_norm, step, grad_scale,
                    step_dev, cursor_dev, scaler_state, growth_factor, backoff_factor, growth_interval, unscaled, norm_hist, nullptr,
                    stream);
}

int32_t dmf_optim_step_sched(float* theta, const float* grad, float* m, float* v, int64_t n, int32_t kind,
                             const dmf_hp_schedule* sched, float eps, float alpha, float weight_decay, float max_norm, int32_t step,
                             float grad_scale, int32_t* step_dev, int32_t* cursor_dev, float* scaler_state, float growth_factor,
                             float backoff_factor, int32_t growth_interval, int32_t unscaled, float* norm_hist, void* stream) {
  HpSched hp{};
  if (fill_sched("optim_step_sched", sched, hp)) return 1;
  return optim_step(theta, grad, m, v, n, kind, 0.f, 0.f, 0.f, eps, 0.f, alpha, weight_decay, max_norm, step, grad_scale, step_dev,
                    cursor_dev, scaler_state, growth_factor, backoff_factor, growth_interval, unscaled, norm_hist, sched, stream);
}

int32_t dmf_optim_step_avg(float* theta, const float* grad, float* m, float* v, int64_t n, int32_t kind, float lr, float beta1,
                           float beta2, float eps, float momentum, float alpha, float weight_decay, float max_norm, int32_t step,
                           float grad_scale, int32_t* step_dev, int32_t* cursor_dev, float* scaler_state, float growth_factor,
                           float backoff_factor, int32_t growth_interval, int32_t unscaled, float* norm_hist,
                           const dmf_hp_schedule* sched, const dmf_weight_avg* avg, void* stream) {
  HpSched hp{};
  if (sched != nullptr) {
    if (fill_sched("optim_step_avg", sched, hp)) return 1;
    lr = beta1 = beta2 = momentum = 0.f;
  }
  return optim_step(theta, grad, m, v, n, kind, lr, beta1, beta2, eps, momentum, alpha, weight_decay, max_norm, step, grad_scale,
                    step_dev, cursor_dev, scaler_state, growth_factor, backoff_factor, growth_interval, unscaled, norm_hist, sched,
                    stream, avg, true);
}

int32_t dmf_weight_average(const dmf_weight_avg* avg, const float* theta, int64_t n, int32_t step, const int32_t* step_dev,
                           void* stream) {
  if (theta == nullptr) return fail("%s", "weight_average: null theta");
  if (n < 0) return fail("%s", "weight_average: negative n");
  if (step < 1 && step_dev == nullptr) return fail("%s", "weight_average: step must be positive (or step_dev given)");
  AvgArgs av{};
  if (fill_avg("weight_average", avg, theta, n, av)) return 1;
  if (n == 0) return 0;
  return check(launch_weight_average(av, theta, n, step, step_dev, static_cast<hipStream_t>(stream)), "weight_average launch");
}

int32_t dmf_qua_loss_ranks(const float* gathered, int32_t ranks, int32_t rank, int32_t bs_r, int32_t K,
                           const int32_t* labels_global, const int32_t* cursor, const dmf_qua_params* prm, float grad_scale,
                           const float* scaler_state, float* loss, float* loss_hist, float* dlogits_rank, void* stream) {
  if (gathered == nullptr || labels_global == nullptr || prm == nullptr) return fail("%s", "null argument");
  if (ranks < 1 || rank < 0 || rank >= ranks) return fail("%s", "qua_loss: ranks must be positive and 0 <= rank < ranks");
  if (bs_r <= 0 || K < 2 || K > KMAX) return fail("%s", "qua_loss: bs must be positive and 2 <= K <= DMF_KMAX");
  if ((int64_t)ranks * 4 * bs_r * K > INT32_MAX) return fail("%s", "qua_loss: the gathered batch is too large");
  QuaArgs a{gathered, ranks * bs_r, K, labels_global, cursor, prm->alpha, prm->beta, prm->gamma, prm->epsilon, prm->tao,
            grad_scale, loss, loss_hist, dlogits_rank, scaler_state, ranks, rank, bs_r};
  return check(launch_qua_loss(a, static_cast<hipStream_t>(stream)), "qua_loss launch");
}

int32_t dmf_qua_loss_scaled(const float* logits, int32_t bs, int32_t K, const int32_t* labels, const int32_t* cursor,
                            const dmf_qua_params* prm, float grad_scale, const float* scaler_state, float* loss,
                            float* loss_hist, float* dlogits, void* stream) {
  return dmf_qua_loss_ranks(logits, 1, 0, bs, K, labels, cursor, prm, grad_scale, scaler_state, loss, loss_hist, dlogits,
                            stream);
}

int32_t dmf_qua_loss(const float* logits, int32_t bs, int32_t K, const int32_t* labels, const int32_t* cursor,
                     const dmf_qua_params* prm, float grad_scale, float* loss, float* loss_hist, float* dlogits,
                     void* stream) {
  return dmf_qua_loss_scaled(logits, bs, K, labels, cursor, prm, grad_scale, nullptr, loss, loss_hist, dlogits, stream);
}

int32_t dmf_ce_loss(const float* logits, int32_t ranks, int32_t rank, int32_t bs_r, int32_t K, const int32_t* labels_global,
                    const int32_t* cursor, const float* class_w, const dmf_ce_params* prm, float grad_scale,
                    const float* scaler_state, float* loss, float* dlogits, void* stream) {
  if (logits == nullptr || labels_global == nullptr || prm == nullptr) return fail("%s", "null argument");
  if (check_ce("ce_loss", prm, ranks, rank, bs_r, K)) return 1;
  CeArgs a{logits, labels_global, cursor, class_w, scaler_state, loss, dlogits, ranks, rank, bs_r, K, prm->kind,
           prm->kind == 0 ? prm->label_smoothing : 0.f, prm->kind == 1 ? prm->gamma : 0.f, grad_scale};
  return check(launch_ce_loss(a, static_cast<hipStream_t>(stream)), "ce_loss launch");
}

int32_t dmf_ce_denominators(const int32_t* labels_global, int32_t N, int32_t rows, int32_t K, const float* class_w, double* denom,
                            void* stream) {
  if (labels_global == nullptr || denom == nullptr) return fail("%s", "ce_denominators: null labels or denom");
  if (N < 1 || rows < 0) return fail("%s", "ce_denominators: N must be positive and rows >= 0");
  if (K < 1 || K > KMAX) return fail("%s", "ce_denominators: 1 <= K <= DMF_KMAX");
  if (rows == 0) return 0;
  return check(launch_ce_denominators(labels_global, N, rows, K, class_w, denom, static_cast<hipStream_t>(stream)),
               "ce_denominators launch");
}

int32_t dmf_pair_argmax(const float* logits, int32_t bs, int32_t K, int32_t* pred, void* stream) {
  if (logits == nullptr || pred == nullptr) return fail("%s", "null argument");
  if (bs <= 0) return 0;
  if (K < 1) return fail("%s", "pair_argmax: K must be positive");
  return check(launch_pair_argmax(logits, bs, K, pred, static_cast<hipStream_t>(stream)), "pair_argmax launch");
}

int32_t dmf_band_mean(const float* x, int32_t layout, int64_t n_img, int64_t n_pix, int32_t C, float* out, void* stream) {
  if (x == nullptr || out == nullptr) return fail("%s", "null argument");
  if ((layout != 0 && layout != 1) || n_img <= 0 || n_pix <= 0 || C <= 0 || (layout == 0 && n_img != 1))
    return fail("%s", "bad band_mean geometry");
  return check(launch_band_mean(x, layout, n_img, n_pix, C, out, static_cast<hipStream_t>(stream)), "band_mean launch");
}

int32_t dmf_confusion_accum(const int32_t* pred, const int32_t* target, int32_t B, int32_t K, int64_t* matrix, void* stream) {
  if (pred == nullptr || target == nullptr || matrix == nullptr) return fail("%s", "null argument");
  if (B <= 0) return 0;
  return check(launch_confusion(pred, target, B, K, reinterpret_cast<unsigned long long*>(matrix), static_cast<hipStream_t>(stream)),
               "confusion launch");
}

int32_t dmf_valid_accum(const float* loss, int32_t n, double* acc, void* stream) {
  if (loss == nullptr || acc == nullptr) return fail("%s", "null argument");
  if (n < 0) return fail("%s", "valid_accum: negative n");
  if (n == 0) return 0;
  return check(launch_valid_accum(loss, n, acc, static_cast<hipStream_t>(stream)), "valid_accum launch");
}

int32_t dmf_keep_best(double* acc, double* best, int32_t* best_epoch, int32_t epoch, const float* theta, float* best_theta,
                      int64_t n, double* val_hist, void* stream) {
  if (acc == nullptr || best == nullptr || best_epoch == nullptr || theta == nullptr || best_theta == nullptr || val_hist == nullptr)
    return fail("%s", "null argument");
  if (epoch < 0 || n < 0) return fail("%s", "keep_best: negative epoch or n");
  if (theta == best_theta) return fail("%s", "keep_best: best_theta must not be theta");
  return check(launch_keep_best(acc, best, best_epoch, epoch, theta, best_theta, n, val_hist, static_cast<hipStream_t>(stream)),
               "keep_best launch");
}

int32_t dmf_labelmap_write(const int32_t* pred, const int32_t* xy, int32_t B, int32_t W, int32_t* map, void* stream) {
  if (pred == nullptr || xy == nullptr || map == nullptr) return fail("%s", "null argument");
  if (B <= 0) return 0;
  return check(launch_labelmap(pred, xy, B, W, map, static_cast<hipStream_t>(stream)), "labelmap launch");
}

int32_t dmf_softmax_stats(const float* logits, int32_t B, int32_t K, const float* inv_temp, const int32_t* xy, int32_t W,
                          int32_t* pred, float* conf, float* margin, float* entropy, void* stream) {
  if (logits == nullptr) return fail("%s", "softmax_stats: null logits");
  if (B < 0) return fail("%s", "softmax_stats: negative B");
  if (K < 1 || K > KMAX) return fail("%s", "softmax_stats: 1 <= K <= DMF_KMAX");
  if (xy != nullptr && W < 1) return fail("%s", "softmax_stats: xy needs W >= 1");
  if (pred == nullptr && conf == nullptr && margin == nullptr && entropy == nullptr)
    return fail("%s", "softmax_stats: every output is NULL");
  if (B == 0) return 0;
  const SoftmaxStatsArgs a{logits, B, K, inv_temp, xy, W, pred, conf, margin, entropy};
  return check(launch_softmax_stats(a, static_cast<hipStream_t>(stream)), "softmax_stats launch");
}

int32_t dmf_calib_accum(const float* conf, const int32_t* pred, const int32_t* target, int32_t B, int32_t K, int32_t nbins,
                        int64_t* hist, void* stream) {
  if (conf == nullptr || pred == nullptr || target == nullptr || hist == nullptr) return fail("%s", "calib_accum: null argument");
  if (nbins < 1 || nbins > 1024) return fail("%s", "calib_accum: 1 <= nbins <= 1024");
  if (B < 0) return fail("%s", "calib_accum: negative B");
  if (B == 0) return 0;
  return check(launch_calib_accum(conf, pred, target, B, K, nbins, reinterpret_cast<unsigned long long*>(hist),
                                  static_cast<hipStream_t>(stream)), "calib_accum launch");
}

int32_t dmf_temperature_init(double* state, void* stream) {
  if (state == nullptr) return fail("%s", "temperature_init: null state");
  return check(launch_temperature_init(state, static_cast<hipStream_t>(stream)), "temperature_init launch");
}

int64_t dmf_temperature_workspace_bytes(int32_t N) {
  if (N < 0) return -1;
  return ((int64_t)N + 255) / 256 * 3 * (int64_t)sizeof(double);
}

int32_t dmf_temperature_step(const float* logits, const int32_t* labels, int32_t N, int32_t K, double* state, void* workspace,
                             int32_t update, void* stream) {
  if (logits == nullptr || labels == nullptr || state == nullptr) return fail("%s", "temperature_step: null logits, labels or state");
  if (N < 1) return fail("%s", "temperature_step: N must be positive");
  if (K < 1 || K > KMAX) return fail("%s", "temperature_step: 1 <= K <= DMF_KMAX");
  if (workspace == nullptr) return fail("%s", "temperature_step: null workspace");
  return check(launch_temperature_step(logits, labels, N, K, state, static_cast<double*>(workspace), update != 0,
                                       static_cast<hipStream_t>(stream)), "temperature_step launch");
}

int32_t dmf_pan2ms(const double* pan, int32_t pitch, int32_t H, int32_t W, double* out, void* stream) {
  if (pan == nullptr || out == nullptr) return fail("%s", "null argument");
  if (H <= 0 || W <= 0 || pitch < 4 * W) return fail("%s", "bad pan2ms geometry");
  return check(launch_pan2ms(pan, pitch, H, W, out, static_cast<hipStream_t>(stream)), "pan2ms launch");
}

int32_t dmf_scene_minmax(const void* raw, int32_t dtype, int64_t n, void* minmax, void* stream) {
  if (raw == nullptr || minmax == nullptr) return fail("%s", "null argument");
  const int es = scene_raw_bytes(dtype);
  if (es == 0) return fail("%s", "scene_minmax: dtype is not a DMF_RAW_* code");
  if (n < 1) return fail("%s", "scene_minmax: empty scene");
  if (reinterpret_cast<uintptr_t>(raw) % es || reinterpret_cast<uintptr_t>(minmax) % es)
    return fail("%s", "scene_minmax: raw / minmax not aligned to the raw element size");
  return check(launch_scene_minmax(raw, dtype, n, minmax, static_cast<hipStream_t>(stream)), "scene_minmax launch");
}

int32_t dmf_scene_prepare(const void* raw, int32_t dtype, int32_t H, int32_t W, int32_t C, const void* minmax, int32_t pad,
                          int32_t half, void* out, void* stream) {
  if (raw == nullptr || minmax == nullptr || out == nullptr) return fail("%s", "null argument");
  const int es = scene_raw_bytes(dtype), os = half ? 2 : 4;
  if (es == 0) return fail("%s", "scene_prepare: dtype is not a DMF_RAW_* code");
  if (H < 1 || W < 1 || C < 1 || pad < 0) return fail("%s", "bad scene_prepare geometry");
  if (pad > H - 1 || pad > W - 1) return fail("%s", "scene_prepare: the reflection needs pad <= H - 1 and pad <= W - 1");
  const int64_t row = ((int64_t)W + pad) * C;
  if (row > INT32_MAX) return fail("%s", "scene_prepare: a padded row of more than 2^31 - 1 elements");
  if (reinterpret_cast<uintptr_t>(raw) % es || reinterpret_cast<uintptr_t>(minmax) % es || reinterpret_cast<uintptr_t>(out) % os)
    return fail("%s", "scene_prepare: raw / minmax / out not aligned to their element size");
  ScenePrepArgs a;
  a.raw = raw; a.minmax = minmax; a.out = out;
  a.H = H; a.W = W; a.C = C; a.pad = pad;
  a.row = (int)row;
  a.shift = (int)((reinterpret_cast<uintptr_t>(out) & 15) / os);
  a.n_out = ((int64_t)H + pad) * row;
  a.inv_row = 1.0 / (double)row;
  if (a.n_out >= ((int64_t)1 << 40)) return fail("%s", "scene_prepare: more than 2^40 output elements");
  return check(launch_scene_prepare(a, dtype, half != 0, static_cast<hipStream_t>(stream)), "scene_prepare launch");
}

#ifdef DMF_STAMPS
int32_t dmf_debug_set_reduce_stamps(void* p) { return check(dmf::set_reduce_stamps(static_cast<unsigned long long*>(p)), "set_reduce_stamps"); }
int32_t dmf_debug_set_attn_stamps(void* p) { return check(dmf::set_attn_stamps(static_cast<unsigned long long*>(p)), "set_attn_stamps"); }
int32_t dmf_debug_set_v2_stamps(void* p) { return check(dmf::set_v2_stamps(static_cast<unsigned long long*>(p)), "set_v2_stamps"); }
#endif

}  // extern "C"
