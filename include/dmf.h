/*
 * dmf.h — C ABI of the MI355X-native dual-modal fusion hot path (libdmf_hip.so).
 *
 * The reference (salalalala23/Dual-modal-fusion) is pure Python and defines NO FFI: its plug-in boundary
 * is the model loader `importlib.import_module('model.' + net_name).Net(args=cfg)`
 * (solver/mainsolver.py:31-34) whose product is called as `net(ms, pan)` (mainsolver.py:52) and trained by
 * `CrossEntropyLoss` + `loss.backward()` + `Adam.step()` (mainsolver.py:49-55).  This library sits one level
 * below that boundary: dual-modal-fusion_amd/model/gmfnet.py::Net binds these entry points with ctypes
 * (INTEGRATION.md shows the stub).  Each entry point names the reference call site it replaces.
 *
 * Conventions: every function returns 0 on success, non-zero on error (text via dmf_last_error());
 * all pointers except `shape`/`in` are DEVICE pointers owned by the caller; no allocation and no host
 * synchronisation inside; `stream` is a hipStream_t passed as void* (NULL = default stream).
 */
#ifndef DMF_H
#define DMF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMF_VERSION 307   /* 0.3.6: dmf_hp_schedule and the *_sched entry points (lr, betas, momentum from a device table); 0.3.5: dmf_optim_step (weight decay, AdamW and gradient-norm clipping on the flat gradient); 0.3.4: dmf_valid_accum, dmf_keep_best (validation sum and best weights stay on the device); 0.3.3: dmf_ce_loss (class weights, label smoothing, focal loss for the unit-gradient step); 0.3.2: dmf_scene_minmax, dmf_scene_prepare (scene preparation on the device); 0.3.1: dmf_qua_loss_ranks (stage-2 loss on the gathered data-parallel batch); 0.3.0 (round 3): dmf_train_plan_steps, dmf_forward_ce, tagged-word exchange (dmf_xgmi_sizes grew), one patch kernel; 0.2.0: dmf_input.half, unit-gradient step, loss scaler, SGD / RMSprop steps */
#define DMF_KMAX 64       /* max number of logits (Categories_Number, utils/config.py:25) */

/* Network / patch geometry (oracle/gmfnet_ref.py::arch_from_cfg). */
typedef struct dmf_shape {
  int32_t C;    /* primary bands           (DATA_DICT[city].size[2], config.yml:77-80)          */
  int32_t C2;   /* auxiliary bands                                                               */
  int32_t P;    /* patch_size              (config.yml:27)                                       */
  int32_t S;    /* aux / primary resolution ratio (reference hard-codes 4, dataset.py:166)       */
  int32_t F;    /* feature width                                                                 */
  int32_t G;    /* spectral groups                                                               */
  int32_t H;    /* hidden width of the head                                                      */
  int32_t K;    /* Categories_Number (logits), <= DMF_KMAX                                       */
  int32_t attention;   /* 0 = late fusion only, 1 = cross-modal attention block                  */
  int32_t heads;       /* attention heads (config.yml:70), head_dim = E / heads                  */
  int32_t E;           /* attention embed dim (config.yml:69)                                    */
  int32_t reserved;
} dmf_shape;

/* Where a batch of patches comes from. */
typedef struct dmf_input {
  int32_t mode;        /* 0: materialised patches (the reference dataloader's tensors, dataset.py:168-185)
                          1: gather from the resident padded scene by pixel coordinates            */
  int32_t B;           /* patches in this batch                                                    */
  /* mode 0 */
  const float* a;      /* [B, C, P, P]        band-major patches                                   */
  const float* b;      /* [B, C2, S*P, S*P]                                                        */
  /* mode 1 */
  const float* sceneA; /* [Hp, Wp, C]   padded, normalised primary scene, pixel-major (function.py:99-117) */
  const float* sceneB; /* [HpB, WpB, C2] padded aux scene                                          */
  const int32_t* xy;   /* [B, 2] top-left pixel (x = row, y = col) of each patch (dataset.py:171-172) */
  int32_t Wp;          /* row pitch of sceneA in pixels                                            */
  int32_t WpB;         /* row pitch of sceneB in pixels                                            */
  /* optional (mode 1): device int holding the index of the current batch inside a pre-uploaded epoch plan;
     when non-NULL, patch b reads xy[(*cursor)*B + b] and labels[(*cursor)*B + b].  Lets a captured
     hipGraph of many steps be replayed without host-side pointer updates. */
  const int32_t* cursor;
  /* mode 1: sceneA holds IEEE fp16 [Hp, Wp, C] instead of fp32 (half the gather bytes).  The first 1x1 conv then runs on
     fp16 operands (window and weights rounded to nearest even) with fp32 accumulation; everything behind it, gradients
     included, stays fp32 (oracle: cfg['gmf']['half'] = 1).  mode 0 with half != 0: the fp32 patches `a` are rounded to
     fp16 as they are staged.  Shapes: dmf_half_supported. */
  int32_t half;
  int32_t reserved;
} dmf_input;

int32_t dmf_version(void);
const char* dmf_last_error(void);

/* 0 if a compiled kernel instance exists for this shape. */
int32_t dmf_shape_supported(const dmf_shape* shape);

/* Which patch kernel dmf_forward (mode 0), dmf_train_fwd_bwd (1) or dmf_backward_dlogits (2) launches for this shape:
 * 2 = the wave-per-channel-segment kernel (csrc/dmf_patch_v2.hip), 0 = no instance.  (1 was round 1's generic kernel,
 * retired in round 3.)  Reporting only (bench.py names the kernel it times). */
int32_t dmf_patch_variant(const dmf_shape* shape, int32_t mode);

/* Flat parameter vector theta (fp32).  Tensor order and offsets (in floats):
 *   0 spec_a.weight [F, C/G]   1 spec_a.bias [F]   2 spat_a.weight [F, 9]   3 spat_a.bias [F]
 *   4 lift_b.weight [F, C2*S*S] 5 lift_b.bias [F]  6 spat_b.weight [F, 9]   7 spat_b.bias [F]
 *   8 fc1.weight [H, 2F]       9 fc1.bias [H]     10 fc2.weight [K, H]     11 fc2.bias [K]
 *  12 attn_wq [E, F]  13 attn_wk [E, F]  14 attn_wv [E, F]  15 attn_wo [F, E]   (attention only)
 * offsets[i] = start of tensor i, offsets[16] = total count. */
int32_t dmf_param_layout(const dmf_shape* shape, int64_t offsets[17]);

/* Bytes of scratch the train/backward entry points need for a batch of B patches.  The workspace may hold anything at entry
 * (no launch reads a word that no launch of the same step wrote) and serves any batch <= B, laid out for that batch; after a
 * launch only the head vectors z, h, dh and dl[:, :K] of rows < B are defined, and no launch writes outside these bytes or
 * outside the extents its other arguments state (which also lists the buffers the caller initialises). */
int64_t dmf_workspace_bytes(const dmf_shape* shape, int32_t B);

/* `pool_w` [P*P] is the network's fixed pooling profile (buffer `pool_w` of the Net).
 *
 * Replaces `output = self.cur_model(data1, data2)` in eval (mainsolver.py:109,169,180) and
 * `pred = output.data.max(1)` (mainsolver.py:139,170).  logits [B, K]; pred [B] int32 may be NULL. */
int32_t dmf_forward(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                    float* logits, int32_t* pred, void* stream);
/* The same launch with the per-patch cross-entropy against labels [B] int32 written to loss [B] — the validation pass,
 * `loss = self.loss(output, target.long())` under no_grad (mainsolver.py:62-76), by the training kernel's own formula.
 * Fails (use dmf_forward_attn + the caller's loss) for the attention network. */
int32_t dmf_forward_ce(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                       const int32_t* labels, float* logits, float* loss, int32_t* pred, void* stream);

/* Forward of the network WITH the cross-modal attention block (shape->attention == 1; BASELINE configs[2]):
 * the conv stages emit bf16 token maps, then a matrix-core kernel (bf16 MFMA operands, fp32 accumulate) does the
 * projections, Q K^T, softmax, P V, the output projection, the pooling correction and the head.
 * `workspace` needs dmf_attn_workspace_bytes(shape, B) bytes; it may hold anything at entry, nothing in it is defined
 * afterwards, and the launches write only inside it and logits [B, K] / pred [B].  Training: dmf_train_attn_fwd_bwd below. */
int64_t dmf_attn_workspace_bytes(const dmf_shape* shape, int32_t B);
int32_t dmf_forward_attn(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                         void* workspace, float* logits, int32_t* pred, void* stream);

/* Replaces forward + `self.loss(output, target.long())` + `loss.backward()` (mainsolver.py:52-54) in ONE
 * launch.  labels [B] int32.  loss_scale multiplies dlogits (1/B for CrossEntropyLoss' mean reduction,
 * utils/utils.py:29).  Writes logits [B, K] and per-patch CE loss [B] (unscaled); leaves per-block weight-
 * gradient slabs and head vectors in `workspace` for dmf_grad_reduce*. */
int32_t dmf_train_fwd_bwd(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                          const int32_t* labels, float loss_scale,
                          float* logits, float* loss, void* workspace, int32_t* adam_step_dev, void* stream);
/* adam_step_dev (may be NULL): device int incremented by one per call (the optimiser step count a later
 * dmf_grad_reduce_adam / dmf_adam_step on the same stream reads instead of its host `step` argument). */

/* The same step for the attention network (shape->attention == 1; BASELINE configs[2]): forward, loss, backward of
 * head, attention block and conv stages in three launches (token kernel, attention fwd+bwd kernel, conv backward
 * from dense gradient maps).  Exactly one of labels (fused cross-entropy, as dmf_train_fwd_bwd) and dlogits
 * (caller-supplied dL/dlogits, as dmf_backward_dlogits; logits are still written) is non-NULL; loss may be NULL.
 * `workspace` as for dmf_train_fwd_bwd (dmf_workspace_bytes counts the attention slabs when shape->attention),
 * `attn_workspace` = dmf_attn_train_workspace_bytes(shape, B) bytes; like `workspace` it may hold anything at entry (token
 * maps, gradient maps and weight copies are written before they are read), nothing in it is defined afterwards, and no launch
 * of the step writes outside the two workspaces, logits [B, K] and loss [B].  Gradients leave through dmf_grad_reduce*. */
int64_t dmf_attn_train_workspace_bytes(const dmf_shape* shape, int32_t B);
int32_t dmf_train_attn_fwd_bwd(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                               const int32_t* labels, const float* dlogits, float loss_scale,
                               float* logits, float* loss, void* workspace, void* attn_workspace,
                               int32_t* adam_step_dev, void* stream);

/* The train step for a loss that couples the whole batch (qua_loss: tostagesolver.py:275-277), in two launches around the
 * caller's loss kernel and WITHOUT a second pass over the patches:
 *   dmf_forward_unit   forward (logits [B, K]) + the conv backward for a UNIT gradient on every pooled feature; leaves the
 *                      head vectors and one row of unit gradients per patch in `workspace`
 *   (loss kernel)      dL/dlogits [B, K] from the logits of the whole batch (dmf_qua_loss)
 *   dmf_backward_unit  dh, dz per patch from dL/dlogits, slab rows = sum of dz x unit rows; then dmf_grad_reduce* as usual
 * Exact, not an approximation: the net is piecewise linear and a feature channel reaches the head only through its two
 * pooled scalars.  Returns non-zero for shapes without such a kernel (dmf_unit_supported; use dmf_forward +
 * dmf_backward_dlogits there).  adam_step_dev as in dmf_train_fwd_bwd. */
int32_t dmf_unit_supported(const dmf_shape* shape);
int32_t dmf_forward_unit(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                         float* logits, void* workspace, int32_t* adam_step_dev, void* stream);
int32_t dmf_backward_unit(const dmf_shape* shape, int32_t B, const float* theta, const float* dlogits, void* workspace,
                          void* stream);

/* The loss kernel of that step for classification with class weights, label smoothing or a focal term — the criteria the
 * patch kernel's fused cross-entropy does not state (`nn.CrossEntropyLoss(weight=, label_smoothing=)`, utils/utils.py:29).
 * With p = softmax(logits[i]), y = the sample's label and w = class_w (NULL: all ones), the per-sample term is
 *   kind 0   t_i = (1 - eps) w[y] (-log p_y) + (eps / K) sum_c w[c] (-log p_c)
 *   kind 1   t_i = w[y] (1 - p_y)^gamma (-log p_y)                                    (gamma = 0: kind 0 with eps = 0)
 * and the batch loss is sum_i t_i / D, D = sum_j w[y_j] over the GLOBAL batch of ranks * bs_r samples — torch's
 * reduction='mean' (the smoothing term is not part of the denominator).  logits [bs_r, K] are rank `rank`'s rows; the global
 * batch's labels are labels_global[(*cursor) * ranks * bs_r + r * bs_r + i] (rank-major as in dmf_qua_loss_ranks; cursor may be
 * NULL).  loss [bs_r] (may be NULL) gets ranks * bs_r * t_i / D: its mean over the rows, averaged over the ranks, is the batch
 * loss (what dmf_grad_reduce* put into loss_hist).  dlogits [bs_r, K] (NULL: value only, the validation pass) gets
 * d(batch loss)/d logits times grad_scale * (scaler_state ? scaler_state[0] : 1).  One launch, no collective: every rank
 * computes the same D from the labels, and its rows are bit-identical to those of a one-rank call on the whole batch.
 * Fails unless 1 <= K <= DMF_KMAX, eps in [0, 1), gamma == 0 or gamma >= 1, kind 0 or 1.  Every w must be > 0. */
typedef struct dmf_ce_params {
  int32_t kind;             /* 0 cross-entropy (weights and label smoothing apply), 1 focal (weights and gamma apply) */
  float   label_smoothing;  /* eps in [0, 1), kind 0 */
  float   gamma;            /* kind 1: 0 or >= 1 */
} dmf_ce_params;
int32_t dmf_ce_loss(const float* logits, int32_t ranks, int32_t rank, int32_t bs_r, int32_t K,
                    const int32_t* labels_global, const int32_t* cursor, const float* class_w,
                    const dmf_ce_params* params, float grad_scale, const float* scaler_state,
                    float* loss, float* dlogits, void* stream);

/* The same criterion INSIDE the attention network's train step: the attention kernel evaluates class weights,
 * label smoothing or the focal term where it otherwise forms the plain cross-entropy, so the step keeps its three launches and
 * visits the patches once.  Two calls:
 *   dmf_ce_denominators        denom[r] = sum over the N labels of plan row r of (double)class_w[label] (NULL: ones), r < rows —
 *                              one 256-thread workgroup per row, in dmf_ce_loss's own summation order: the bits of the D that
 *                              dmf_ce_loss forms for that row.  Once per plan upload (or per eager batch, rows = 1).
 *                              Fails for NULL labels or denom, N < 1, rows < 0, K outside 1..DMF_KMAX; rows == 0 is a no-op.
 *   dmf_train_attn_fwd_bwd_ce  dmf_train_attn_fwd_bwd with the criterion `ce`: labels_global [plan rows][ranks * B] rank-major
 *                              and denom [plan rows], both indexed by *in->cursor (row 0 without a cursor); rank `rank` trains on
 *                              its B rows.  logits [B, K] and the gradient are bit for bit what dmf_train_attn_fwd_bwd(labels) ->
 *                              dmf_ce_loss(grad_scale) -> dmf_train_attn_fwd_bwd(dlogits) leave, and loss [B] (may be NULL) the
 *                              rows dmf_ce_loss writes: N t_i / D, from a value-only launch of its kernel behind the step's three.
 *                              Fails where dmf_train_attn_fwd_bwd or dmf_ce_loss fail, for a NULL struct, params, labels_global
 *                              or denom, and for reserved != 0. */
typedef struct dmf_ce_fused {
  const dmf_ce_params* params; const float* class_w; const int32_t* labels_global; const double* denom;
  int32_t ranks, rank; float grad_scale; int32_t reserved;
} dmf_ce_fused;
int32_t dmf_ce_denominators(const int32_t* labels_global, int32_t N, int32_t rows, int32_t K,
                            const float* class_w /* NULL: ones */, double* denom /* [rows] */, void* stream);
int32_t dmf_train_attn_fwd_bwd_ce(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                                  const dmf_ce_fused* ce, float* logits, float* loss /* nullable */,
                                  void* workspace, void* attn_workspace, int32_t* adam_step_dev, void* stream);

/* 0 if the fp16-scene kernels (dmf_input.half) exist for this shape. */
int32_t dmf_half_supported(const dmf_shape* shape);

/* ---- dynamic loss scaling: the role of `torch.cuda.amp.GradScaler` (tostagesolver.py:83-84 creates two, :98 / :119
 * `scaler.scale(loss).backward(); scaler.step(opt); scaler.update()`), device-resident so that a captured graph can
 * carry it.  state = DMF_SCALER_FLOATS floats on the device: [0] scale, [1] growth tracker, [2] found_inf of the step in
 * flight, [3] number of skipped steps so far, [4..] internal.
 *   dmf_scaler_init            state <- (init_scale, 0, 0, 0)                       GradScaler(init_scale=65536.)
 *   dmf_train_fwd_bwd_scaled   dmf_train_fwd_bwd with dL/dlogits multiplied by loss_scale * state[0]   scaler.scale(loss)
 *   dmf_qua_loss_scaled        the same for the stage-2 loss kernel (dlogits multiplied by grad_scale * state[0])
 *   dmf_grad_reduce_scaled     dmf_grad_reduce with the unscale (grad = sum / state[0]) and the non-finite check folded in,
 *                              plus the bookkeeping of dmf_grad_reduce_adam (loss_hist[cursor] = mean loss, cursor += 1);
 *                              follow with dmf_unscale_adam(unscaled = 1).  Single GPU: data parallel must check AFTER
 *                              the all-reduce (dmf_grad_reduce, all-reduce, dmf_unscale_adam(unscaled = 0))
 *   dmf_unscale_adam           grad *= grad_scale / state[0] (skipped when unscaled != 0);
 *                              any non-finite element -> the WHOLE step is skipped (no Adam state
 *                              change, adam_step_dev taken back), scale *= backoff_factor, tracker = 0; else Adam as
 *                              dmf_adam_step and tracker += 1, at growth_interval: scale *= growth_factor, tracker = 0
 *                              (scaler.unscale_ + scaler.step + scaler.update).  grad is the flat gradient of
 *                              dmf_grad_reduce (after the all-reduce when data parallel); adam_step_dev is required. */
#define DMF_SCALER_FLOATS 8
int32_t dmf_scaler_init(float* state, float init_scale, void* stream);
int32_t dmf_train_fwd_bwd_scaled(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                                 const int32_t* labels, float loss_scale, const float* scaler_state,
                                 float* logits, float* loss, void* workspace, int32_t* adam_step_dev, void* stream);
int32_t dmf_unscale_adam(float* theta, float* grad, float* m, float* v, int64_t n,
                         float lr, float beta1, float beta2, float eps, float grad_scale,
                         float* scaler_state, float growth_factor, float backoff_factor, int32_t growth_interval,
                         int32_t unscaled, int32_t* adam_step_dev, int32_t* cursor_dev, void* stream);
int32_t dmf_grad_reduce_scaled(const dmf_shape* shape, int32_t B, const void* workspace, float* grad, float* scaler_state,
                               int32_t* cursor_dev, const float* loss, float* loss_hist, void* stream);

/* Backward for a caller-supplied dL/dlogits [B, K] (the autograd path: torch computes the loss). */
int32_t dmf_backward_dlogits(const dmf_shape* shape, const dmf_input* in, const float* theta, const float* pool_w,
                             const float* dlogits, void* workspace, void* stream);

/* Workspace -> flat gradient [n_params] (deterministic fixed-order sums). */
int32_t dmf_grad_reduce(const dmf_shape* shape, int32_t B, const void* workspace, float* grad, void* stream);

/* Replaces `self.optimizer.step()` for torch.optim.Adam(lr) defaults (utils/utils.py:10-12;
 * betas 0.9/0.999, eps 1e-8, no weight decay: with one, or AdamW, or a clipped gradient norm, dmf_optim_step).  step = 1-based step count.  grad_scale multiplies grad
 * first (1/world_size after an all-reduce(sum)). */
int32_t dmf_adam_step(float* theta, const float* grad, float* m, float* v, int64_t n,
                      float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale,
                      const int32_t* adam_step_dev, int32_t* cursor_dev, void* stream);
/* adam_step_dev (may be NULL): when given, the step count is read from the device instead of `step`.
 * cursor_dev (may be NULL): device int advanced by one (the epoch-plan cursor of dmf_input). */

/* The reference's other two optimisers (utils/utils.py:13-16), on the flat gradient of dmf_grad_reduce:
 * `torch.optim.SGD(params, lr, momentum)` — momentum_buf [n] may be NULL when momentum == 0; step (or *step_dev) == 1 marks the
 * first step, where torch initialises the buffer with the gradient — and `torch.optim.RMSprop(params, lr, alpha)` (eps 1e-8
 * is torch's default; square_avg [n] starts at zero).  grad_scale, cursor_dev as in dmf_adam_step. */
int32_t dmf_sgd_step(float* theta, const float* grad, float* momentum_buf, int64_t n, float lr, float momentum,
                     int32_t step, float grad_scale, const int32_t* step_dev, int32_t* cursor_dev, void* stream);
int32_t dmf_rmsprop_step(float* theta, const float* grad, float* square_avg, int64_t n, float lr, float alpha, float eps,
                         float grad_scale, int32_t* cursor_dev, void* stream);

/* ---- weight decay, AdamW and gradient-norm clipping: ONE launch on the flat gradient of dmf_grad_reduce (after
 * the all-reduce when data parallel) that does what a torch user writes between backward() and the end of step():
 *   [scaler.unscale_(opt)]  torch.nn.utils.clip_grad_norm_(params, max_norm)  [scaler.step(opt); scaler.update()] / opt.step()
 * for opt = torch.optim.Adam / AdamW / SGD / RMSprop(..., weight_decay=).  Per element, in this order:
 *   1. g = grad[i] * grad_scale; with a scaler state and unscaled == 0: g = grad[i] * (grad_scale / state[0]), the product
 *      dmf_unscale_adam forms.  grad is only read.
 *   2. with a scaler state, any non-finite g skips the WHOLE step as dmf_unscale_adam does: theta, m, v stay, scale *= backoff,
 *      tracker = 0, skipped steps += 1, *step_dev -= 1; the cursor still advances (and a clipped step still records its norm,
 *      which then is inf or NaN).
 *   3. max_norm > 0: S = sum_i (double)g^2 in a fixed order, norm = (float)sqrt(S), coef = min(1, max_norm / (norm + 1e-6f)),
 *      g *= coef (a NaN norm gives NaN, as torch's clamp does); norm_hist (may be NULL) gets norm_hist[*cursor_dev] = norm, the
 *      PRE-clip norm that clip_grad_norm_ returns (norm_hist[0] without a cursor).  max_norm <= 0: no clipping, norm_hist is
 *      not written.
 *   4. weight decay: DMF_OPT_ADAM, _SGD, _RMSPROP  g += weight_decay * theta   (torch's `weight_decay=`: L2, before anything else)
 *                    DMF_OPT_ADAMW                 theta *= 1 - lr * weight_decay   (decoupled)
 *   5. the update of the kind by the arithmetic of dmf_adam_step (m, v), dmf_sgd_step (m = momentum buffer, may be NULL when
 *      momentum == 0; v unused) or dmf_rmsprop_step (m = square_avg, `eps`; v unused); the step count (bias corrections, SGD's
 *      first step) is *step_dev when given, else `step`.
 *   6. scaler growth as in dmf_unscale_adam; *cursor_dev += 1 (may be NULL).
 * Every workgroup forms S and the skip decision itself from the whole gradient, in the same order, and then updates its own
 * 256 elements: the same coef bits everywhere, no second launch and no grid barrier.  Without a scaler state growth_factor,
 * backoff_factor, growth_interval and unscaled must be 0; with one, step_dev is required.  n == 0 is a no-op.
 * Fails on: NULL theta / grad, NULL m or v where the kind needs it, n < 0, an unknown kind, a negative or non-finite
 * weight_decay, a non-finite max_norm, scaler hyper-parameters without a scaler state. */
#define DMF_OPT_ADAM    0
#define DMF_OPT_ADAMW   1
#define DMF_OPT_SGD     2
#define DMF_OPT_RMSPROP 3
int32_t dmf_optim_step(float* theta, const float* grad, float* m, float* v, int64_t n, int32_t kind,
                       float lr, float beta1, float beta2, float eps, float momentum, float alpha,
                       float weight_decay, float max_norm, int32_t step, float grad_scale,
                       int32_t* step_dev, int32_t* cursor_dev,
                       float* scaler_state, float growth_factor, float backoff_factor, int32_t growth_interval,
                       int32_t unscaled, float* norm_hist, void* stream);

/* dmf_grad_reduce + dmf_adam_step in one launch (single-GPU step). grad may be NULL. */
int32_t dmf_grad_reduce_adam(const dmf_shape* shape, int32_t B, const void* workspace,
                             float* theta, float* m, float* v, float* grad,
                             float lr, float beta1, float beta2, float eps, int32_t step,
                             const int32_t* adam_step_dev, int32_t* cursor_dev,
                             const float* loss, float* loss_hist, void* stream);
/* loss / loss_hist (may be NULL): when both are given, loss_hist[cursor] = mean(loss[0..B)) (fixed-order sum),
 * i.e. the value the reference prints per step (`loss.item()`, mainsolver.py:58) without a host sync. */

/* The reference's whole inner loop `for batch in loader: zero_grad; forward; CE; backward; Adam.step` (mainsolver.py:49-55)
 * over n_steps consecutive batches of a resident plan, as ONE call: step k = dmf_train_fwd_bwd on the B patches at
 * in->xy + 2 B k with labels + B k, then dmf_grad_reduce_adam (device step count, cursor, loss history) — 2 n_steps launches
 * enqueued by one C loop, nothing else between them.  in->mode must be 1 and in->cursor NULL; adam_step_dev and cursor_dev are
 * required (device ints: steps taken so far, next row of loss_hist).  Late-fusion network, ADAM, one GPU. */
int32_t dmf_train_plan_steps(const dmf_shape* shape, const dmf_input* in, float* theta, const float* pool_w,
                             const int32_t* labels, float loss_scale, float* logits, float* loss, void* workspace,
                             float* m, float* v, float lr, float beta1, float beta2, float eps,
                             int32_t* adam_step_dev, int32_t* cursor_dev, float* loss_hist, int32_t n_steps, void* stream);

/* ---- a device-resident schedule of the step's hyper-parameters ------------------------------------
 * table [rows][4] fp32 on the device, row = (lr, beta1, beta2, momentum): the optimiser kernels read the row of their step
 * themselves, so a captured hipGraph or the launch loop of dmf_train_plan_steps follows a learning-rate scheduler without new
 * launch arguments.  The row of a step:
 *   row_dev != NULL  (unit `epoch`)  row = *row_dev, a device int32 that the host sets between epochs by a stream-ordered
 *                                    fill (never inside a captured graph);
 *   row_dev == NULL  (unit `step`)   row = st - 1, st the 1-based optimiser step count the kernel already has (*step_dev /
 *                                    *adam_step_dev when given, else the `step` argument).  The forward launch has advanced
 *                                    the device count before the update launch reads it.  A step that the loss scaler skips
 *                                    takes its count back (dmf_optim_step, 2.), so the next step reads the SAME row again:
 *                                    the schedule counts optimiser steps taken, as torch's scheduler.step() after a skipped
 *                                    GradScaler step is usually guarded to do.
 * In both units the row is clamped to [0, rows - 1].  lr always comes from the row; beta1 and beta2 for DMF_OPT_ADAM / _ADAMW
 * (bias corrections from the row's betas and st, always formed on the device; AdamW's 1 - lr * weight_decay from the row's
 * lr); momentum for DMF_OPT_SGD.  eps, alpha, weight_decay and max_norm stay launch arguments.  The table is only read.
 * Each *_sched entry point is its twin with (lr, beta1, beta2[, momentum]) replaced by the schedule, does the same arithmetic
 * on the same fp32 values, and fails on: a NULL schedule or table, rows < 1, and everything its twin fails on;
 * dmf_optim_step_sched also on DMF_OPT_SGD without m (the host cannot see the row's momentum). */
typedef struct dmf_hp_schedule { const float* table; int32_t rows; const int32_t* row_dev; } dmf_hp_schedule;
int32_t dmf_optim_step_sched(float* theta, const float* grad, float* m, float* v, int64_t n, int32_t kind,
                             const dmf_hp_schedule* sched, float eps, float alpha,
                             float weight_decay, float max_norm, int32_t step, float grad_scale,
                             int32_t* step_dev, int32_t* cursor_dev,
                             float* scaler_state, float growth_factor, float backoff_factor, int32_t growth_interval,
                             int32_t unscaled, float* norm_hist, void* stream);
int32_t dmf_grad_reduce_adam_sched(const dmf_shape* shape, int32_t B, const void* workspace,
                                   float* theta, float* m, float* v, float* grad,
                                   const dmf_hp_schedule* sched, float eps, int32_t step,
                                   const int32_t* adam_step_dev, int32_t* cursor_dev,
                                   const float* loss, float* loss_hist, void* stream);
int32_t dmf_train_plan_steps_sched(const dmf_shape* shape, const dmf_input* in, float* theta, const float* pool_w,
                                   const int32_t* labels, float loss_scale, float* logits, float* loss, void* workspace,
                                   float* m, float* v, const dmf_hp_schedule* sched, float eps,
                                   int32_t* adam_step_dev, int32_t* cursor_dev, float* loss_hist, int32_t n_steps, void* stream);

/* ---- an averaged copy of the weights, kept by the update launch -------------------------------------
 * The role of `torch.optim.swa_utils.AveragedModel(model[, multi_avg_fn=get_ema_multi_avg_fn(decay)])` with
 * `update_parameters(model)` after every optimiser step: avg [n] fp32 on the device, in theta's layout.  With st the 1-based
 * count of the optimiser step just taken (*step_dev / *adam_step_dev when given, else the `step` argument: the count the
 * update already reads) and start >= 1 the first averaged step:
 *   st <= start   avg[i] = theta[i]                        (a copy: avg is a valid weight vector from the first step on;
 *                                                          st == start is AveragedModel's first update_parameters)
 *   st >  start   avg[i] = lerp(avg[i], theta[i], w)       n = st - start
 *                 DMF_AVG_EMA   w = `weight`, the float32 of 1 - decay (formed in double by the caller, as torch forms it)
 *                 DMF_AVG_MEAN  w = 1.f / (float)(n + 1)   (torch's default equal average)
 *   lerp(a, b, w) = |w| < 0.5 ? fmaf(w, b - a, a) : fmaf(-(1 - w), b - a, b)      (torch.lerp; nothing else is contracted)
 * theta is the vector the step has just updated.  A step the loss scaler skips leaves avg untouched and takes its count back,
 * so n counts optimiser steps taken.  Averaging is local to a rank: every rank holds the same theta after the update.
 *   dmf_weight_average          the rule alone, one launch over n elements (n == 0: a no-op)
 *   dmf_optim_step_avg          dmf_optim_step (sched == NULL) or dmf_optim_step_sched (then lr, beta1, beta2 and momentum are
 *                               ignored) with the rule applied by the lane that updated theta[i]
 *   dmf_grad_reduce_adam_avg    dmf_grad_reduce_adam / _sched likewise, inside the reduce + Adam launch
 *   dmf_train_plan_steps_avg    dmf_train_plan_steps / _sched on dmf_grad_reduce_adam_avg
 * theta, m, v, grad, the loss history and every other output keep the bits of the twin.  Each entry point fails on: a NULL
 * dmf_weight_avg or avg pointer, an unknown kind, DMF_AVG_EMA with a weight that is not finite or not in (0, 1], start < 1, avg
 * overlapping theta, and everything its twin fails on.  `reserved` must be 0. */
#define DMF_AVG_EMA  0
#define DMF_AVG_MEAN 1
typedef struct dmf_weight_avg { float* avg; int32_t kind; float weight; int32_t start; int32_t reserved; } dmf_weight_avg;
int32_t dmf_weight_average(const dmf_weight_avg* avg, const float* theta, int64_t n, int32_t step, const int32_t* step_dev,
                           void* stream);
int32_t dmf_optim_step_avg(float* theta, const float* grad, float* m, float* v, int64_t n, int32_t kind,
                           float lr, float beta1, float beta2, float eps, float momentum, float alpha,
                           float weight_decay, float max_norm, int32_t step, float grad_scale,
                           int32_t* step_dev, int32_t* cursor_dev,
                           float* scaler_state, float growth_factor, float backoff_factor, int32_t growth_interval,
                           int32_t unscaled, float* norm_hist,
                           const dmf_hp_schedule* sched /* NULL: the launch arguments */, const dmf_weight_avg* avg, void* stream);
int32_t dmf_grad_reduce_adam_avg(const dmf_shape* shape, int32_t B, const void* workspace,
                                 float* theta, float* m, float* v, float* grad,
                                 float lr, float beta1, float beta2, float eps, int32_t step,
                                 const int32_t* adam_step_dev, int32_t* cursor_dev,
                                 const float* loss, float* loss_hist,
                                 const dmf_hp_schedule* sched, const dmf_weight_avg* avg, void* stream);
int32_t dmf_train_plan_steps_avg(const dmf_shape* shape, const dmf_input* in, float* theta, const float* pool_w,
                                 const int32_t* labels, float loss_scale, float* logits, float* loss, void* workspace,
                                 float* m, float* v, float lr, float beta1, float beta2, float eps,
                                 int32_t* adam_step_dev, int32_t* cursor_dev, float* loss_hist,
                                 const dmf_hp_schedule* sched, const dmf_weight_avg* avg, int32_t n_steps, void* stream);

/* ---- stage 2 of the two-stage path (solver/tostagesolver.py:259-346) ---------------------------------------
 * The stage-2 net takes ONE input, the four streams (ms, pan, ms_gan, pan_gan) stacked on the batch axis
 * (`torch.concat([data1..data4])`, tostagesolver.py:272), and is trained with `qua_loss`. */
typedef struct dmf_qua_params { float alpha, beta, gamma, epsilon, tao; } dmf_qua_params;   /* cfg['dqtl'][...] */
/* Replaces `self.loss(output, bs, target, cfg)` + the logits part of `loss.backward()` (tostagesolver.py:275-277,
 * train/loss_function.py:57-76).  logits [4*bs, K]; labels [bs] int32 (the reference passes float class ids);
 * cursor (may be NULL) as in dmf_input: labels[(*cursor)*bs + i], loss_hist[*cursor].  loss [1] and loss_hist may be
 * NULL; dlogits [4*bs, K] may be NULL (loss only: the validation loop, tostagesolver.py:293-295) and is multiplied
 * by grad_scale.
 * Limits, where a float32 probability y is 0 or so small that a term of the formula underflows (a logit some 50 or more
 * below its row's maximum): y log y and its derivative count as 0 at y == 0; exp(-|c / y|) of the beta term and its
 * derivative exp(-|c / y|) |c| / y^2 count as 0 wherever the exponential has underflowed (both tend to 0 with y, although
 * y * y reaches 0 first and the plain quotient would be 0 / 0).  With these a row with such a class gives a finite loss and
 * finite dlogits: the values of the formula in exact arithmetic, to within float32 rounding. */
int32_t dmf_qua_loss(const float* logits, int32_t bs, int32_t K, const int32_t* labels, const int32_t* cursor,
                     const dmf_qua_params* params, float grad_scale, float* loss, float* loss_hist, float* dlogits,
                     void* stream);
int32_t dmf_qua_loss_scaled(const float* logits, int32_t bs, int32_t K, const int32_t* labels, const int32_t* cursor,
                            const dmf_qua_params* params, float grad_scale, const float* scaler_state,
                            float* loss, float* loss_hist, float* dlogits, void* stream);
/* The same loss for data-parallel stage 2, on the logits as all_gather_into_tensor leaves them: gathered
 * [ranks][4][bs_r][K] (rank-major; global sample g = r*bs_r + i of stream s at row r*4*bs_r + s*bs_r + i).  The global batch
 * is bs = ranks*bs_r in the order [rank][bs_r]: labels_global[(*cursor)*bs + g]; loss / loss_hist[*cursor] get the GLOBAL
 * loss; dlogits_rank [4][bs_r][K] (may be NULL) gets rank `rank`'s rows only, multiplied by grad_scale * scaler_state[0]
 * (scaler_state may be NULL).  Loss and rows are bit-identical to dmf_qua_loss_scaled on the same batch restacked
 * stream-major [4][bs][K]; ranks = 1, rank = 0 is dmf_qua_loss_scaled. */
int32_t dmf_qua_loss_ranks(const float* gathered, int32_t ranks, int32_t rank, int32_t bs_r, int32_t K,
                           const int32_t* labels_global, const int32_t* cursor, const dmf_qua_params* params,
                           float grad_scale, const float* scaler_state, float* loss, float* loss_hist,
                           float* dlogits_rank, void* stream);
/* Replaces `(output[:bs] + output[bs:2*bs]).softmax(dim=-1).data.max(1)[1]` (tostagesolver.py:337,366,378). */
int32_t dmf_pair_argmax(const float* logits, int32_t bs, int32_t K, int32_t* pred, void* stream);
/* Auxiliary input of the single-stream net: per-pixel mean over bands, ((x0+x1)+x2)+... then / C.
 * layout 0: pixel-major scene [n_pix, C] (n_img = 1) -> out [n_pix]; 1: band-major patches [n_img, C, n_pix] -> out [n_img, n_pix]. */
int32_t dmf_band_mean(const float* x, int32_t layout, int64_t n_img, int64_t n_pix, int32_t C, float* out, void* stream);

/* ---- data-parallel gradient exchange over xGMI ------------------------------------
 * The reference has no multi-GPU path (BaseSolver builds one loader on one device, basesolver.py:86-105); the
 * coupling between data-parallel ranks is the parameter update of mainsolver.py:54-55 only.  One-shot exchange
 * for the sub-MB gradient: every rank writes its local gradient into an inbox slot in EVERY rank's uncached device
 * buffer over xGMI — each value together with its sequence number in ONE 8-byte store, so the value is its own
 * arrival mark — and each rank then polls its own inbox and adds the values in rank order (same bits on every
 * rank, no atomics), inside the gradient-reduce + Adam launch.  Buffers are shared
 * between the per-GPU processes with HIP IPC handles; the caller moves the 64-byte handles between ranks (any
 * host channel: torch.distributed all_gather_object, a file, a pipe).  Everything is device-side, so a whole
 * data-parallel step can be captured in a hipGraph. */
#define DMF_XGMI_MAX_RANKS 16
typedef struct dmf_xgmi_comm {
  int32_t world, rank;
  int64_t capacity;       /* floats per exchange this communicator was sized for (>= n_params)             */
  int32_t timeout_ms;     /* a rank that waits longer for a peer sets status = 1 and stops waiting          */
  int32_t seq_bias;       /* added to the device step count to form the exchange sequence number; the host  */
                          /* raises it whenever it rewinds the device step count (graph warm-up)            */
  void* data[DMF_XGMI_MAX_RANKS];    /* data[r]: rank r's inbox (own allocation or IPC mapping)             */
  void* flags[DMF_XGMI_MAX_RANKS];   /* flags[r]: rank r's status block (only the owner's is used)          */
} dmf_xgmi_comm;
int32_t dmf_xgmi_sizes(int64_t capacity, int32_t world, int64_t* data_bytes, int64_t* flag_bytes);
int32_t dmf_xgmi_alloc(int64_t bytes, void** ptr);          /* uncached device memory, zero-filled (host sync) */
int32_t dmf_xgmi_free(void* ptr);
int32_t dmf_xgmi_export(void* ptr, uint8_t handle[64]);     /* hipIpcGetMemHandle                              */
int32_t dmf_xgmi_open(const uint8_t handle[64], void** ptr);/* hipIpcOpenMemHandle (another process' buffer)   */
int32_t dmf_xgmi_close(void* ptr);
int32_t dmf_xgmi_status(const dmf_xgmi_comm* comm, int32_t* status);   /* host sync; 0 ok, 1 a wait timed out   */
/* buf[0..n) <- sum over ranks in rank order (n <= capacity).  seq: 1, 2, 3 ... per call, same on all ranks. */
int32_t dmf_xgmi_allreduce(const dmf_xgmi_comm* comm, float* buf, int64_t n, int32_t seq, void* stream);
/* dmf_grad_reduce + exchange + dmf_adam_step(grad_scale) in one launch: the data-parallel form of
 * dmf_grad_reduce_adam.  adam_step_dev is required (the sequence number is *adam_step_dev + seq_bias). */
int32_t dmf_grad_reduce_xgmi_adam(const dmf_shape* shape, int32_t B, const void* workspace,
                                  float* theta, float* m, float* v, const dmf_xgmi_comm* comm,
                                  float lr, float beta1, float beta2, float eps, float grad_scale,
                                  const int32_t* adam_step_dev, int32_t* cursor_dev,
                                  const float* loss, float* loss_hist, void* stream);

/* Replaces the per-sample `.item()` loop `test_matrix[pred][target] += 1` (mainsolver.py:140-141):
 * matrix [K, K] int64, rows = prediction. */
int32_t dmf_confusion_accum(const int32_t* pred, const int32_t* target, int32_t B, int32_t K,
                            int64_t* matrix, void* stream);

/* ---- an epoch's validation pass without the host (mainsolver.py:62-81; `train.epoch_block`) -----------
 * acc[0] += sum_{i<n} (double)loss[i]: replaces `val_loss += loss.item() * n` per batch (mainsolver.py:70-71) with loss the
 * per-patch terms dmf_forward_ce / dmf_ce_loss leave.  ONE workgroup, fixed order (lane t adds loss[t], loss[t + 256], ... in
 * index order, then a fixed tree over the 256 lanes): the same bits on every run.  One lane reads, adds to and writes acc[0];
 * the stream orders it against its neighbours.  n == 0 is a no-op. */
int32_t dmf_valid_accum(const float* loss, int32_t n, double* acc, void* stream);
/* The end of that pass, `if val_loss < best_loss` (mainsolver.py:77-81), in ONE launch of ONE workgroup: val = acc[0];
 * val_hist[epoch] = val; if val < *best (strict; a NaN is never the best): *best = val, *best_epoch = epoch and
 * best_theta[0..n) = theta[0..n); acc[0] = 0 for the next epoch.  The caller sizes val_hist (epoch < its length) and starts
 * *best at +inf.  theta and best_theta must not overlap. */
int32_t dmf_keep_best(double* acc, double* best, int32_t* best_epoch, int32_t epoch, const float* theta, float* best_theta,
                      int64_t n, double* val_hist, void* stream);

/* Replaces `label_np[x][y] = pred` (mainsolver.py:171-173,182-183): map [H, W] int32. */
int32_t dmf_labelmap_write(const int32_t* pred, const int32_t* xy, int32_t B, int32_t W, int32_t* map, void* stream);

/* ---- calibrated confidence: how far a pixel's class can be trusted, from the logits [B, K] that the forward
 * entry points leave on the device.  New symbols at an unchanged DMF_VERSION: detect them by name.
 *
 * Per row, with beta = inv_temp[0] (device; NULL: 1) and m the row maximum: pred = the FIRST maximal index (the rule of the
 * forward entry points' own pred); t_c = (l_c - m) * beta in fp32, e_c = expf(t_c), Z = sum e_c in a fixed order;
 * conf = 1 / Z; margin = (1 - e2) / Z with e2 the largest e_c over c != pred (K == 1: 0); entropy = max(0, logf(Z) -
 * (sum e_c t_c) / Z), a term with e_c == 0 counting as 0.  Each output may be NULL, not all of them.  xy == NULL: row i
 * writes index i; else xy [B, 2] and row i writes index x * W + y (the addressing of the label-map entry point below, whose
 * launch this one replaces where the confidence is wanted too).  Finite logits and beta > 0 are the caller's contract.
 * Fails on NULL logits, B < 0, K outside 1..DMF_KMAX, xy with W < 1, and when every output is NULL; B == 0 is a no-op. */
int32_t dmf_softmax_stats(const float* logits, int32_t B, int32_t K, const float* inv_temp, const int32_t* xy, int32_t W,
                          int32_t* pred, float* conf, float* margin, float* entropy, void* stream);
/* The reliability histogram hist [nbins][3] int64 (the caller zeroes it): a row whose target lies outside [0, K) is skipped,
 * else b = min(nbins - 1, (int)(conf * (float)nbins)) and hist[b][0] += 1, hist[b][1] += (pred == target),
 * hist[b][2] += llrint((double)conf * 2^32): integers, so the result is exact and independent of the order.
 * Fails on a NULL argument, nbins outside 1..1024 and B < 0; B == 0 is a no-op. */
int32_t dmf_calib_accum(const float* conf, const int32_t* pred, const int32_t* target, int32_t B, int32_t K, int32_t nbins,
                        int64_t* hist, void* stream);
/* Temperature scaling (Guo et al. 2017) without a host round trip.  state = DMF_TEMP_DOUBLES doubles on the device:
 * [0] beta = 1 / T, [1] nll, [2] g = d nll / d beta, [3] h = d2 nll / d beta2 (sums over the rows, at the beta the step
 * started from), [4] lo, [5] hi, [6] steps taken, [7] reserved.  The init sets beta = 1, lo = 2^-6, hi = 2^6.
 * A step is two launches: (a) workgroups of 256 rows form, in double, with d_c = l_c - m, Z = sum exp(beta d_c) and
 * p_c = exp(beta d_c) / Z: nll_i = ln Z - beta d_y, g_i = sum p_c d_c - d_y, h_i = sum p_c d_c^2 - (sum p_c d_c)^2 (a row whose
 * label lies outside [0, K) adds nothing) and leave their three sums, taken in a fixed tree order, in `workspace`; (b) one
 * workgroup adds those in index order and stores nll, g, h.  With update != 0 it then takes the safeguarded Newton step:
 * g > 0 -> hi = beta, else lo = beta; beta <- beta - g / h, or sqrt(lo hi) if h <= 0 or that candidate is not finite or not
 * strictly inside (lo, hi); steps += 1.  update == 0 only evaluates (the NLL of a split at a given beta).
 * The workspace query needs N >= 0 (else -1); the step fails on NULL logits, labels, state or workspace, N < 1 and K outside 1..DMF_KMAX. */
#define DMF_TEMP_DOUBLES 8
int32_t dmf_temperature_init(double* state, void* stream);
int64_t dmf_temperature_workspace_bytes(int32_t N);
int32_t dmf_temperature_step(const float* logits, const int32_t* labels, int32_t N, int32_t K, double* state, void* workspace,
                             int32_t update, void* stream);

/* ---- flip / rotate augmentation and test-time augmentation from a scene atlas.  New symbols at an unchanged
 * DMF_VERSION: detect them by name.
 *
 * Variant k in 0..7 of an array X [rows, cols, C]: Y = X transposed (axes 0 and 1) if k & 4; then the rows of Y reversed if
 * k & 2; then its columns reversed if k & 1.  k = 0 is the identity; 0..3 are the flips, 0..7 the dihedral group.
 * dmf_scene_atlas writes dst [n_ops * slot_rows, dst_pitch, C]: slot s (rows [s * slot_rows, (s + 1) * slot_rows)) holds variant
 * ops[s] of src's leading [rows, cols] pixels at its top-left corner and zero elsewhere.  src is [>= rows, src_pitch, C],
 * pixel-major; elements of elem_bytes (2 or 4) bytes are moved as bits, never converted.  EVERY byte of dst is written (the
 * caller need not clear it), in one launch.  `ops` is a HOST array.  A flipped or transposed patch of the scene is then an
 * ordinary patch of the atlas at a mirrored top-left coordinate: with the patch window n, the extent (Hp, Wp) of the region,
 *   if k & 4: x, y, Hp, Wp = y, x, Wp, Hp;   if k & 2: x = Hp - n - x;   if k & 1: y = Wp - n - y;   x += s * slot_rows.
 * Returns 0, or without a launch: 1 a NULL pointer; 2 rows, cols or C < 1, or src_pitch < cols; 3 elem_bytes not 2 or 4;
 * 4 n_ops outside 1..8 or an op outside 0..7; 5 slot_rows or dst_pitch too small for a requested variant (a transposed one
 * needs slot_rows >= cols and dst_pitch >= rows); 6 src or dst not aligned to elem_bytes; 7 dst overlaps src; 8 a row of more
 * than 2^31 - 1 bytes or more workgroups than a grid holds; and 9 where the launch itself failed.  (These two entry points
 * report by code: they do not set the text of dmf_last_error.) */
int32_t dmf_scene_atlas(const void* src, int32_t elem_bytes, int32_t rows, int32_t cols, int32_t src_pitch, int32_t C,
                        const int32_t* ops /* host */, int32_t n_ops, int32_t slot_rows, int32_t dst_pitch,
                        void* dst, void* stream);
/* The mean of V variants' logits: logits[b][c] = (((l_0 + l_1) + l_2) + ...) / (float)V in fp32, in variant order, from
 * logits_v [V][B][K]; pred[b] (may be NULL) = the FIRST maximal index of that row of the mean (the rule of the forward entry
 * points).  V = 1 copies; B == 0 is a no-op.  Returns 1 for NULL logits_v or logits, 2 for V < 1 or B < 0, 3 for K outside
 * 1..DMF_KMAX, 9 where the launch failed. */
int32_t dmf_logits_mean(const float* logits_v /* [V][B][K] */, int32_t V, int32_t B, int32_t K,
                        float* logits /* [B][K] */, int32_t* pred /* nullable */, void* stream);

/* ---- spatial regularisation of class maps: a scene-guided bilateral filter on the class probabilities.  New
 * symbols at an unchanged DMF_VERSION: detect them by name.
 *
 * Pixel x = (i, j) of an H x W scene is element (i, j) of the resident padded primary scene [>= H, pitch_pixels >= W, C]
 * (padded at the bottom and the right only; slot 0 of a scene atlas).  Radius r in 1..3, n = (2r + 1)^2, offset index
 * k = (di + r)(2r + 1) + (dj + r) for di, dj in -r..r.  Everything is pixel-major.
 *   affinity   aff [H W][n] fp32, once per scene.  For the neighbour y = x + (di, dj): 0 where y lies outside
 *              [0, H) x [0, W); else d2 = (sum_c (a_c(x) - a_c(y))^2) / (float)C in fp32 (an fp16 scene widened exactly first;
 *              the bands summed in ascending order, each term by one fmaf) and
 *              aff = expf(-(((float)(di^2 + dj^2) * cs) + (d2 * cr))), the two products and the sum each rounded once;
 *              cs = 1 / (2 sigma_s^2), cr = 1 / (2 sigma_r^2).  The centre (k = (n - 1) / 2) is exactly 1.
 *   scatter    per row of logits [B, K], with beta = inv_temp[0] (device; NULL: 1): t_c, e_c and Z exactly as
 *              dmf_softmax_stats forms them; prob[(x W + y) K + c] = e_c / Z for (x, y) = xy[row], and mask[x W + y] = 1.
 *              prob[pred] is the bits of dmf_softmax_stats's conf.  Cells that no row names are left alone: the caller
 *              clears prob and mask first.  Coordinates inside [0, H) x [0, W) are the caller's contract.
 *   filter     one iteration.  For a pixel x with mask 1: w_k = aff[x][k] * mask(y_k) (mask(y) = 0 outside the scene),
 *              N_c = sum_k w_k p_c(y_k) by fmaf in ascending k from 0, D = sum_k w_k in ascending k (D >= 1: the centre),
 *              out_c = N_c / D; label_map[x] = the FIRST maximal index of out (the forward entry points' rule).  A pixel
 *              with mask 0 gets an all-zero row of prob_out and its label-map cell is left alone; what its row of prob_in
 *              holds is never read.  prob_out must not overlap prob_in.
 * No float atomics and fixed orders: two runs give the same bits.  All three report by code, without a launch (and so with
 * every output as it was): 1 a NULL pointer (inv_temp may be NULL); 2 H, W or C < 1 (scatter: B < 0 or W < 1); 3 K outside
 * 1..DMF_KMAX; 4 r outside 1..3; 5 elem_bytes not 2 or 4; 6 pitch_pixels < W; 7 prob_out overlaps prob_in; 8 the scene not
 * aligned to elem_bytes, or more workgroups than a grid holds; and 9 where the launch itself failed.  B == 0 is a no-op.
 * (They do not set the text of dmf_last_error.) */
int32_t dmf_prob_scatter(const float* logits, int32_t B, int32_t K, const float* inv_temp, const int32_t* xy, int32_t W,
                         float* prob, uint8_t* mask, void* stream);
int32_t dmf_spatial_affinity(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C,
                             int32_t r, float cs, float cr, float* aff, void* stream);
int32_t dmf_spatial_filter(const float* prob_in, const uint8_t* mask, const float* aff, int32_t H, int32_t W, int32_t K,
                           int32_t r, float* prob_out, int32_t* label_map, void* stream);

/* ---- band reduction: the device stages of a PCA of the primary scene in front of the network.  New symbols at
 * an unchanged DMF_VERSION: detect them by name.  The eigen-decomposition between them is the caller's (utils/spectral.py).
 *
 * x is N pixels of C fp32 bands, `pitch` floats apart (pitch >= C); C in 1..512, any remainder mod 4.  Everything is device
 * memory; x and y need 4-byte, mean, cov and workspace 8-byte alignment.
 *   moments   mean[c] = (sum_n x[n][c]) / N, summed in double in a fixed tree (slices of the pixels, added as 16 interleaved chains;
 *             inside a slice four row groups of four interleaved chains each).  cov[i][j] = (sum_n d[n][i] d[n][j]) / (N - 1) with
 *             d[n][i] = x[n][i] - (float)mean[i] formed in fp32.  The products of a run of DMF_PCA_RUN consecutive pixels
 *             (run q = pixels [q R, (q + 1) R)) are one fp32 fmaf chain in pixel order, on the fp32 matrix cores; the runs are
 *             added in double, in ascending order inside a slice of runs and then over the slices in ascending order, and the
 *             sum is divided by N - 1 in double.  Only the upper triangle is computed; cov[j][i] is written from the sum of
 *             cov[i][j]: the same bits.  N >= 2.  `workspace` needs dmf_band_moments_workspace_bytes(N, C) bytes (-1 for an N
 *             or C out of range); four launches, the last one the finishing launch.
 *   project   y[n][k] = sum_c (x[n][c] - (float)mean[c]) * basis[c][k]: one fp32 fmaf chain over the bands in ascending order
 *             from 0, on the fp32 matrix cores.  basis [C][K] fp32, K in 1..min(C, 64), y [N][K].  One pass over x; N == 0 is
 *             a no-op.
 * No float atomics and fixed orders that depend on (N, C) only: two runs give the same bits.  Both report by code, without a
 * launch (and so with every output as it was): 1 a NULL pointer; 2 N < 2 (project: N < 0); 3 C outside 1..512; 4 K outside
 * 1..min(C, 64); 5 pitch < C; 6 a misaligned pointer; 8 N * pitch beyond 64-bit byte offsets, or more workgroups than a grid
 * holds; and 9 where a launch itself failed.  (They do not set the text of dmf_last_error.) */
#define DMF_PCA_RUN 256   /* R: pixels one fp32 accumulator of the covariance covers */
int64_t dmf_band_moments_workspace_bytes(int64_t N, int32_t C);
int32_t dmf_band_moments(const float* x, int64_t N, int32_t C, int64_t pitch, double* mean /* [C] */, double* cov /* [C][C] */,
                         void* workspace, void* stream);
int32_t dmf_band_project(const float* x, int64_t N, int32_t C, int64_t pitch, const double* mean, const float* basis /* [C][K] */,
                         int32_t K, float* y /* [N][K] */, void* stream);

/* ---- noise moments for the noise-adjusted transform, `band_reduce_noise`.  New symbols at an unchanged
 * DMF_VERSION: detect them by name.  The generalised eigen-fit is the caller's (utils/spectral.py, fit_noise_adjusted).
 *
 * x is the scene of H x W pixels, flat pixel p = row * W + column, C fp32 bands each, `pitch` floats apart: the contract of
 * dmf_band_moments (device memory; pitch >= C; C in 1..512, any remainder mod 4; x 4-byte, ncov and workspace 8-byte aligned).
 * For a direction with pixel step s — 0 horizontal, s = 1, the right neighbour in the row; 1 vertical, s = W, the pixel below —
 *   e[p] = x[p] - x[p + s]      formed in fp32 (one rounding), for every pixel p that has that neighbour,
 *   e[p] = 0                    for a pixel without it (last column; last row): by selection, not by multiplication — nothing
 *                               behind the last pixel is read, and no value of the scene reaches a product through such a pixel,
 *   M    = the number of pixels that have the neighbour: H (W - 1) horizontal, (H - 1) W vertical,
 *   ncov[i][j] = (sum_p e[p][i] e[p][j]) / (2 M)      uncentred; the 2 is the shift-difference estimator's.
 * The arithmetic is the covariance's: the products of run q = pixels [q R, (q + 1) R) of the flat scene, R = DMF_PCA_RUN, are one
 * fp32 fmaf chain in pixel order on the fp32 matrix cores; the runs are added in double, ascending inside a slice of runs and
 * then over the slices in ascending order by the finishing launch, which divides by 2 M in double.  Only the upper triangle is
 * computed; ncov[j][i] is written from the sum of ncov[i][j].  Two launches; no allocation, no host synchronisation, no float
 * atomics; the orders depend on (H, W, C, direction) only: two runs give the same bits.  `workspace` needs
 * dmf_band_noise_workspace_bytes(H, W, C) bytes (-1 for H or W < 1, H W < 2 or C out of range).
 * Reports by code as dmf_band_moments does, without a launch and with ncov as it was: 1 a NULL pointer; 2 M < 1 (a one-column
 * scene horizontally, a one-row scene vertically; H or W < 1); 3 C outside 1..512; 5 pitch < C; 6 a misaligned pointer; 7 a
 * direction outside 0..1; 8 H W pitch beyond 64-bit byte offsets; 9 where a launch itself failed. */
int64_t dmf_band_noise_workspace_bytes(int32_t H, int32_t W, int32_t C);
int32_t dmf_band_noise_moments(const float* x, int32_t H, int32_t W, int32_t C, int64_t pitch,
                               int32_t direction /* 0 horizontal, 1 vertical */, double* ncov /* [C][C] */, void* workspace,
                               void* stream);

/* ---- superpixel voting of class maps: SLIC segments of the primary scene and a per-segment vote.  New symbols
 * at an unchanged DMF_VERSION: detect them by name.
 *
 * The scene is the leading H x W pixels of the resident padded primary scene [>= H, pitch_pixels >= W, C], as
 * dmf_spatial_affinity takes it (fp32, or fp16 widened exactly; slot 0 of a scene atlas).  Everything is device memory.
 *   grid      segment size S in DMF_SEG_SMIN..DMF_SEG_SMAX; gh = ceil(H / S), gw = ceil(W / S), Kc = gh gw; cluster
 *             k = gi gw + gj belongs to cell (gi, gj) and keeps that index for life.  The cell of pixel x = (i, j) is
 *             (i div S, j div S); its candidates are the clusters of the cells (gi + u, gj + v), u, v in {-1, 0, 1}, that lie
 *             inside the grid, visited in ascending slot s = 3 (u + 1) + (v + 1).
 *   centres   [Kc][C + 2] fp32: C spectrum values, then row and column as floats.
 *   init      cluster k sits at pixel (min(H - 1, gi S + S div 2), min(W - 1, gj S + S div 2)) and takes its spectrum.
 *   assign    d2 = (sum_c (a_c(x) - mu_c)^2) / (float)C in fp32, the bands in ascending order, each term one fmaf of the rounded
 *             difference; sp = fl(fl(di di) + fl(dj dj)) with di = fl((float)i - row_k), dj = fl((float)j - col_k);
 *             D = fl(d2 + fl(cw sp)), cw = the double (compactness / S)^2 rounded to fp32.  seg[x] (int32) = the candidate with
 *             the smallest D, the first slot on equality (a NaN D never wins; the pixel's own cell is the fallback).
 *   update    the members of k are the pixels of its 3 x 3 cells with seg == k; counts[k] (int32) = their number.  Per cell and
 *             candidate, the members' spectra are summed in fp32 from +0 over the cell's pixels in row order, and their rows and
 *             columns as integers; cluster k adds its up to nine cell partials in double, in ascending slot of its own 3 x 3
 *             cells, and divides once in double: the mean spectrum, the mean row and the mean column, each rounded to fp32.  A
 *             cluster without a member keeps its row of centres.  A seg value that is none of a pixel's candidates is a
 *             member of nothing.  Two launches; `workspace` needs dmf_slic_workspace_bytes(H, W, C, S) bytes, 16-byte aligned
 *             (-1 for an argument out of range), and what it holds between calls does not matter.
 *   vote      prob [H W][K] and mask [H W] as dmf_prob_scatter leaves them.  The masked members of k are the pixels of its 3 x 3
 *             cells with seg == k and mask 1; segcount[k] = their number.  DMF_VOTE_MEAN: segprob[k][c] = (sum p_c) / (float)count
 *             in fp32, the members in row order of the 3S x 3S window, an all-zero row for count 0.  DMF_VOTE_MAJORITY:
 *             segprob[k][c] = the number of masked members whose FIRST maximal class is c, an exact integer in fp32 (at most
 *             9 S^2 < 2^24).  label_map[x], for a pixel with mask 1, = the first maximal index of its segment's row; a pixel with
 *             mask 0 keeps its cell and its row of prob is never read.  prob_out (may be NULL) [H W][K] = the segment's row, all
 *             zeros where mask is 0.  A masked pixel whose seg value is none of its candidates counts for no segment and stands
 *             for itself: its own first maximal class, and in prob_out its own row (mean) or 1 at that class (majority).  Labels
 *             are compared with the candidates' indices and never used as an index, so this holds for any contents of seg.
 * n iterations = init, n x (assign, update), a last assign; nothing synchronises with the host.  Connectivity is the business of
 * dmf_label_components and dmf_region_merge below, and dmf_region_vote votes over the regions they give.
 * No float atomics and fixed orders: two runs give the same bits.  All report by code, without a launch (and so with every
 * output as it was): 1 a NULL pointer (prob_out may be NULL); 2 H, W or C < 1; 3 K outside 1..DMF_KMAX; 4 S outside
 * DMF_SEG_SMIN..DMF_SEG_SMAX; 5 elem_bytes not 2 or 4; 6 pitch_pixels < W; 7 an output overlaps an input or another output;
 * 8 the scene not aligned to elem_bytes, the workspace not to 16 bytes, or more workgroups than a grid holds; 9 a launch itself
 * failed; 10 a compactness that is not finite and >= 0; 11 a mode other than the two; 12 workspace_bytes too small.
 * (They do not set the text of dmf_last_error.) */
#define DMF_SEG_SMIN 4
#define DMF_SEG_SMAX 32
#define DMF_VOTE_MEAN 0
#define DMF_VOTE_MAJORITY 1
int64_t dmf_slic_workspace_bytes(int32_t H, int32_t W, int32_t C, int32_t S);
int32_t dmf_slic_init(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C, int32_t S,
                      float* centres /* [Kc][C + 2] */, void* stream);
int32_t dmf_slic_assign(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C, int32_t S,
                        float compactness, const float* centres, int32_t* seg /* [H W] */, void* stream);
int32_t dmf_slic_update(const void* scene, int32_t elem_bytes, int32_t pitch_pixels, int32_t H, int32_t W, int32_t C, int32_t S,
                        const int32_t* seg, float* centres, int32_t* counts /* [Kc] */, void* workspace, int64_t workspace_bytes,
                        void* stream);
int32_t dmf_segment_vote(const float* prob, const uint8_t* mask, const int32_t* seg, int32_t H, int32_t W, int32_t K, int32_t S,
                         int32_t mode, float* segprob /* [Kc][K] */, int32_t* segcount /* [Kc] */, int32_t* label_map /* [H W] */,
                         float* prob_out /* nullable */, void* stream);

/* ---- connected superpixels: the 4-connected components of a label image, the merge of small fragments, and a vote over regions
 * of any shape.  New symbols at an unchanged DMF_VERSION: detect them by name.  Everything is device memory and
 * integer arithmetic: no order of execution can change a bit.
 *   components  labels [H][W] int32 may hold any values: they are compared for equality and never used as an index.  Two pixels
 *               are joined when they are 4-neighbours with equal labels.  comp[x] (int32) = the smallest raster index i W + j
 *               among the pixels of x's component: its root.  Three launches whatever the image holds.  H W < 2^31.
 *   kept        size[r] = the pixel count of the component with root r.  With n_labels > 0 every label k in 0..n_labels - 1 that
 *               occurs has a main component: its largest, on equal size the one with the smaller root; other labels have none.  A
 *               component is kept when size >= min_size, or it is a main component, or its root is pixel 0.  Every other
 *               component is a fragment.
 *   target      of a fragment: the component of the pixel to the left of its root, or, for a root in column 0, of the pixel
 *               above it.  Both have a smaller raster index than the root, so they lie outside the component (the previously
 *               visited adjacent label of scikit-image's enforce_connectivity), and the target's root is strictly smaller than
 *               the fragment's: targets form a forest.  final[r] = r for a kept component and final[target] otherwise, chains
 *               followed to the end.  Sizes do NOT accumulate along a chain: a target that is itself a fragment stays one however
 *               many pixels it absorbs.  min_size = 1 keeps every component: it splits clusters and absorbs nothing.
 *   regions     numbered 0..R - 1 in ascending order of their kept roots.  region [H][W] int32; region_size [H W] int32: the
 *               first R cells the pixel counts with absorbed pixels included, the others 0; stats [4] int32 = R, the number of
 *               components, the number of fragments absorbed, 0.  `comp` must be what dmf_label_components left for `labels`:
 *               with other contents the regions are unspecified, but nothing is read or written out of range and every chain ends.
 *   workspace   dmf_region_workspace_bytes(H, W, n_labels) bytes serve both calls (n_labels 0 for the labelling alone);
 *               dmf_region_vote_workspace_bytes(R, K) the vote; -1 for an argument out of range; 16-byte aligned; what a
 *               workspace holds between calls does not matter.
 *   vote        prob [H W][K] and mask [H W] as dmf_prob_scatter leaves them.  The members of region r are the pixels with
 *               region == r and mask 1; regcount[r] = their number.  A pixel's first maximal class is the smallest class index at
 *               which its row of prob is largest.  DMF_VOTE_MAJORITY: regprob[r][c] = the number of members whose first maximal
 *               class is c, counted as an integer and converted to fp32 (exact below 2^24).  DMF_VOTE_MEAN is exact fixed point, so
 *               no summation order exists: each term is q = rint(clamp(p, 0, 1) 2^36), half to even, a NaN counted as 0 (the
 *               product by 2^36 is exact in fp32); the terms are added as 64-bit integers (H W < 2^27 members of at most 2^36: below
 *               2^63); regprob[r][c] = (float)((double)sum / ((double)count 2^36)), the int64 -> double conversion rounding to
 *               nearest even, an all-zero row for count 0.  label_map[x], for a pixel with mask 1, = the first maximal index of its
 *               region's row; a pixel with mask 0 keeps its cell and its row of prob is never read.  prob_out (may be NULL)
 *               [H W][K] = the region's row, all zeros where mask is 0.  A masked pixel whose region value is outside 0..R - 1
 *               counts for no region and stands for itself, as in dmf_segment_vote: its own first maximal class, and in prob_out
 *               its own row (mean) or 1 at that class (majority).
 *   bound       against the plain float64 mean m of clamp(p, 0, 1): |q 2^-36 - p| <= 2^-37 for every term, so the exact rational
 *               sum / (count 2^36) is within 2^-37 of m; the conversion and the division in double add at most 2^-52 relative,
 *               and the one rounding to fp32 of a value <= 1 at most 2^-25:  |regprob - m| <= 2^-37 + 2^-25 + 2^-50.
 * Return codes, all before any launch (and so with every output as it was): 1 a NULL pointer (prob_out may be NULL); 2 H, W or R
 * < 1, or R > H W; 3 K outside 1..DMF_KMAX; 7 an output or the workspace overlaps an input, or two of them each other; 8 a pointer
 * not aligned to its type, the workspace not to 16 bytes, or more workgroups than a grid holds; 9 a launch itself failed; 11 a
 * mode other than the two; 12 workspace_bytes too small; 13 H W >= DMF_REGION_PIXELS_MAX (components, merge) or >=
 * DMF_REGION_VOTE_PIXELS_MAX (vote); 14 min_size < 1; 15 n_labels < 0.  (They do not set the text of dmf_last_error.) */
#define DMF_REGION_PIXELS_MAX 2147483648LL      /* 2^31: a root is an int32 */
#define DMF_REGION_VOTE_PIXELS_MAX 134217728LL  /* 2^27: 2^27 terms of at most 2^36 stay below 2^63 */
int64_t dmf_region_workspace_bytes(int32_t H, int32_t W, int32_t n_labels);
int64_t dmf_region_vote_workspace_bytes(int32_t R, int32_t K);
int32_t dmf_label_components(const int32_t* labels, int32_t H, int32_t W, int32_t* comp /* [H W] */, void* workspace,
                             int64_t workspace_bytes, void* stream);
int32_t dmf_region_merge(const int32_t* labels, const int32_t* comp, int32_t H, int32_t W, int32_t n_labels, int32_t min_size,
                         int32_t* region /* [H W] */, int32_t* region_size /* [H W] */, int32_t* stats /* [4] */, void* workspace,
                         int64_t workspace_bytes, void* stream);
int32_t dmf_region_vote(const float* prob, const uint8_t* mask, const int32_t* region, int32_t H, int32_t W, int32_t K, int32_t R,
                        int32_t mode, float* regprob /* [R][K] */, int32_t* regcount /* [R] */, int32_t* label_map /* [H W] */,
                        float* prob_out /* nullable */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- connected superpixels, the spectrum-aware fragment merge: dmf_region_merge's positional target replaced by
 * the adjacent group with the nearest mean spectrum, with groups of fragments that grow until they reach min_size (a Boruvka
 * style merge over the region adjacency graph).  New symbols at an unchanged DMF_VERSION: detect them by name.  All sums are
 * integers and every double operation is rounded on its own, so no order of execution can change a bit.
 *   inputs      labels [H][W] int32 and comp as dmf_label_components leaves it; the scene as dmf_slic_* take it (the leading
 *               H x W pixels of the resident padded primary scene, pitch_pixels, C bands, fp32, or fp16 widened exactly); n_labels
 *               and min_size as in dmf_region_merge.  H W < DMF_REGION_VOTE_PIXELS_MAX, as for the vote.
 *   features    every scene value a gives q = rint(clamp(a, 0, 1) 2^36), half to even, a NaN counted as 0: dmf_region_vote's
 *               quantiser.  sum[r][b] = the 64-bit integer sum of q over the pixels of component r, n[r] its pixel count.
 *   groups      every component starts as a group of its own, kept by the rule of dmf_region_merge unchanged (size >= min_size, or
 *               the main component of a label in 0..n_labels - 1, or root 0).  A group's id is the smallest root among its
 *               components; a group is active while it is not kept.
 *   round       all choices use the state at the start of the round.  Every active group f looks at every group g != f that
 *               shares a 4-neighbour pixel pair with it.  m_f[b] = (double)sum_f[b] / ((double)n_f 2^36) (the conversion rounding
 *               to nearest even, the divisor exact); d(f, g) = sum_b (m_f[b] - m_g[b])^2 in double from 0, the bands in ascending
 *               order, each subtraction, product and addition rounded on its own (nothing contracted).  f chooses the g with the
 *               smallest (d, id of g), compared lexicographically; then every pair (f, choice(f)) is united.  Kept groups choose
 *               nothing, so a united group holds at most one group that was kept at the start of the round: two kept regions never
 *               merge.  Sums and counts add exactly; the new group is kept if a member was kept or its count >= min_size; its id
 *               is the smallest root in it.
 *   end         rounds repeat until no group is active.  Every active group is united with another, so the active groups at least
 *               halve per round: at most 1 + floor(log2(fragments)) rounds, fragments = the initially active groups.  Root 0 is
 *               kept and the image is connected, so the process ends.
 *   result      regions numbered 0..R - 1 in ascending order of group id.  region [H][W] int32; region_size [H W] int32: the first R
 *               cells the pixel counts, the others 0; stats [4] int32 = R, the number of components, components - R, the rounds
 *               run.  With min_size = 1 nothing is active: region, region_size and the first three statistics equal
 *               dmf_region_merge's at min_size = 1.
 *   calls       dmf_region_graph_count leaves counts [2] int32 = the number of components and of fragments; the caller reads them
 *               (the one host read), sizes the workspace with them and hands them to dmf_region_graph_merge, which enqueues
 *               1 + floor(log2(fragments)) rounds (a round that finds no active group does nothing) and reads nothing itself.
 *               `comp`, `components` and `fragments` must be what dmf_label_components and the count left: with other contents the
 *               regions are unspecified, but nothing is read or written out of range and every loop ends.
 *   workspace   dmf_region_graph_workspace_bytes(H, W, C, n_labels, components) bytes, 16-byte aligned; -1 for an argument out of
 *               range; sums and means are indexed by component and cost 16 C bytes each.  The count needs the bytes of
 *               (H, W, 1, n_labels, 1).  What a workspace holds between calls does not matter.
 * Return codes, all before any launch (and so with every output as it was), numbered as above: 1 a NULL pointer; 2 H, W or C < 1;
 * 5 elem_bytes not 2 or 4; 6 pitch_pixels < W; 7 an output or the workspace overlaps an input, or two of them each other; 8 a
 * pointer not aligned to its type (the scene to elem_bytes) or the workspace not to 16 bytes (every grid fits: H W < 2^27);
 * 9 a launch itself failed; 12 workspace_bytes too small; 13 H W >= DMF_REGION_VOTE_PIXELS_MAX; 14 min_size < 1; 15 n_labels < 0;
 * 16 components outside 1..H W or fragments outside 0..components - 1.  (They do not set the text of dmf_last_error.) */
#define DMF_REGION_GRAPH_ROUNDS_MAX 27          /* fragments < 2^27 */
int64_t dmf_region_graph_workspace_bytes(int32_t H, int32_t W, int32_t C, int32_t n_labels, int32_t components);
int32_t dmf_region_graph_count(const int32_t* labels, const int32_t* comp, int32_t H, int32_t W, int32_t n_labels, int32_t min_size,
                               int32_t* counts /* [2] */, void* workspace, int64_t workspace_bytes, void* stream);
int32_t dmf_region_graph_merge(const int32_t* labels, const int32_t* comp, const void* scene, int32_t elem_bytes, int32_t pitch_pixels,
                               int32_t H, int32_t W, int32_t C, int32_t n_labels, int32_t min_size, int32_t components,
                               int32_t fragments, int32_t* region /* [H W] */, int32_t* region_size /* [H W] */,
                               int32_t* stats /* [4] */, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- morphological profiles of the reduced bands, `band_profile: morph`: openings and closings by reconstruction
 * of the first P components of the scores that dmf_band_project leaves, at a ladder of n radii.  New symbols at an unchanged
 * DMF_VERSION: detect them by name.  All arithmetic is min / max of fp32 values, so no order of execution can change a bit.
 *   input       scores [H][W] pixels of K fp32 components, `pitch` floats apart (pitch >= K), finite (the caller refuses
 *               anything else).  Every value read is canonicalised once as x + 0.0f: -0 becomes +0.
 *   operators   on one plane f [H][W]; B_r the (2 r + 1) x (2 r + 1) square, the window clipped to the image (the same as padding
 *               with +inf for the erosion and -inf for the dilation):
 *                 eps_r(f) = min over B_r                          delta_r(f) = max over B_r
 *                 R^delta(m | f), m <= f: the limit of j <- min(delta_1(j), f) from j = m (connectivity 8); R^eps(m | f), m >= f,
 *                 its dual: the limit of j <- max(eps_1(j), f)
 *                 gamma_r(f) = R^delta(eps_r(f) | f)   the opening,   phi_r(f) = R^eps(delta_r(f) | f)   the closing by reconstruction
 *   planes      the closing side is computed on g = -f (negation is exact; -0 is canonicalised again): phi_r(f) =
 *               -R^delta(eps_r(g) | g).  Side s (0 opening, 1 closing), component p < P and radius index i < n give mask plane
 *               s P + p (f or -f) and plane q = (s P + p) n + i; planes are [H][W] fp32, planar, H W floats apart.
 *   markers     mask [2 P] planes and markers [2 n P] planes = eps_{r_i}(mask plane q / n), by separable row and column passes with
 *               a running minimum over LDS-staged lines; `scratch` [2 n P] planes holds the row pass.  radii: HOST memory, n
 *               strictly increasing values in 1..DMF_MORPH_RMAX.  Two launches.
 *   reconstruct X holds the markers on entry.  Round k reads X for even k and Y for odd k and writes the other; a workgroup owns a
 *               tile of DMF_MORPH_TILE x DMF_MORPH_TILE pixels, iterates it with a halo in LDS to its own stability and writes it
 *               back, so the result and the number of rounds depend on (H, W, data) only.  A tile is skipped in a round when
 *               neither it nor one of its 8 neighbours changed in the round before (both buffers then hold its value); a launch
 *               whose predecessor changed no tile returns at once.  One call enqueues the rounds first_round .. first_round +
 *               rounds - 1 (first_round a multiple of DMF_MORPH_BATCH, 1 <= rounds <= DMF_MORPH_BATCH; the first call has
 *               first_round 0) and reads nothing.  `state` (device, dmf_morph_state_bytes(H, W, planes) bytes, 4-byte aligned, any
 *               contents before round 0) starts with 2 DMF_MORPH_BATCH int32 counters: counter k mod (2 DMF_MORPH_BATCH) = the
 *               tiles that round k changed.  The caller reads a batch's counters after enqueuing it; at the first zero the
 *               reconstruction is complete and X and Y are equal.  `planes_per_mask`: plane q has mask plane q / planes_per_mask.
 *               With a marker above its mask, or NaN, the result is unspecified; nothing is read or written out of range and
 *               every loop ends.
 *   stack       out [H][W][C] fp32, C = K + 2 n P: for each p < P the bands phi_{r_n}, .., phi_{r_1}, f, gamma_{r_1}, .., gamma_{r_n}
 *               (f canonicalised), then the components P .. K - 1 of the scores bit for bit.  `planes` = X or Y after the end.
 *   workspace   dmf_morph_workspace_bytes(H, W, P, n) = the bytes of mask, X, Y (each plane H W floats, in that order) and the
 *               state of 2 n P planes; -1 for an argument out of range.  Nothing allocates.
 * No float atomics (the counters are int32 atomic adds).  All report by code, without a launch (and so with every output as it
 * was): 1 a NULL pointer; 2 H or W < 1, or H W >= DMF_MORPH_PIXELS_MAX; 3 K outside 1..64 or P outside 1..K (reconstruct: planes
 * outside 1..DMF_MORPH_PLANES_MAX, or not a multiple of planes_per_mask >= 1); 4 n outside 1..DMF_MORPH_NMAX, or radii that are not
 * strictly increasing in 1..DMF_MORPH_RMAX; 5 pitch < K; 6 a pointer not 4-byte aligned; 7 two of the plane sets (or out and an
 * input) are the same memory; 8 more workgroups than a grid holds, or H W pitch beyond 64-bit byte offsets; 9 a launch itself
 * failed; 10 first_round or rounds out of range.  (They do not set the text of dmf_last_error.) */
#define DMF_MORPH_RMAX 32
#define DMF_MORPH_NMAX 8
#define DMF_MORPH_TILE 32
#define DMF_MORPH_BATCH 8
#define DMF_MORPH_PLANES_MAX 1024               /* 2 DMF_MORPH_NMAX 64 */
#define DMF_MORPH_PIXELS_MAX 2147483648LL       /* 2^31 */
int64_t dmf_morph_workspace_bytes(int32_t H, int32_t W, int32_t P, int32_t n);
int64_t dmf_morph_state_bytes(int32_t H, int32_t W, int32_t planes);
int32_t dmf_morph_markers(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P,
                          const int32_t* radii /* host [n] */, int32_t n, float* mask /* [2 P][H][W] */,
                          float* markers /* [2 n P][H][W] */, float* scratch /* [2 n P][H][W] */, void* stream);
int32_t dmf_morph_reconstruct(const float* mask, float* X, float* Y, int32_t H, int32_t W, int32_t planes, int32_t planes_per_mask,
                              int32_t first_round, int32_t rounds, void* state, void* stream);
int32_t dmf_morph_stack(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P, int32_t n, const float* mask,
                        const float* planes /* [2 n P][H][W] */, float* out /* [H][W][K + 2 n P] */, void* stream);

/* ---- attribute profiles of the reduced bands, `band_profile: area`: area openings and closings of the first P
 * components of the scores that dmf_band_project leaves, at a ladder of n area thresholds.  New symbols at an unchanged
 * DMF_VERSION: detect them by name.  From the quantiser on everything is integer, so no order of execution can change a bit.
 *   input       scores [H][W] pixels of K fp32 components, `pitch` floats apart (pitch >= K), finite (the caller refuses
 *               anything else).  Every value read is canonicalised once as x + 0.0f: -0 becomes +0.
 *   range       per component f: lo = min f, hi = max f over the plane, exact (integer atomics on the order-preserving unsigned
 *               image of the float; no float atomics).  range [P][2] = {lo, hi}.
 *   quantise    in double, the operations in this order (no multiply is followed by an add: nothing contracts):
 *                 d = (double)f - (double)lo;  m = d (double)L;  v = m / ((double)hi - (double)lo);  q = min(L - 1, (int)floor(v))
 *               and q = 0 everywhere where hi == lo.  L = the number of levels, 2..DMF_ATTR_LEVELS_MAX.
 *   opening     on the integer plane q, 4-connectivity, threshold a >= 1:
 *                 gamma_a(q)(x) = the largest t in 0..q(x) such that the 4-connected component of {q >= t} that holds x has at
 *                 least a pixels (level 0 always counts) = the number of levels t in 1..q(x) whose component qualifies: the sets
 *                 {q >= t} are nested, so the component's size falls as t rises.
 *   closing     phi_a(q) = (L - 1) - gamma_a((L - 1) - q)
 *   value       value(c) = (float)((double)lo + ((double)c ((double)hi - (double)lo)) / (double)L): multiply, divide, add.
 *   planes      q [2 P][H][W] uint8: plane p < P holds q of component p, plane P + p holds L - 1 - q.
 *               count [2 P][n][H][W] uint8: count[s][i] = gamma_{a_i} of plane s.
 *   levels      dmf_attr_area_levels takes the levels first_level .. first_level + levels - 1 of all 2 P planes (1 <= levels <= T,
 *               1 <= first_level, the last level <= L - 1; T = the level planes the workspace was sized for, 1..DMF_ATTR_BATCH_MAX):
 *               four launches, nothing is read back, there is no convergence loop.  Per (plane, level): the components of {q >= t}
 *               (a 16 x 16 tile's union-find in LDS, the tile's q staged once per call; atomicMin links across tile borders; every
 *               pixel's root), the size of every root (integer atomicAdd, one per run of equal roots in a wave), and the pixel's
 *               owner adds to count the levels at which size >= a_i.  The call with first_level 1 STORES count, every later call
 *               adds: enqueue the levels 1 .. L - 1 in ascending batches on one stream.  areas: HOST memory, n strictly increasing
 *               values >= 1 (int32: < 2^31).
 *   stack       out [H][W][C] fp32, C = K + 2 n P: for each p < P the bands value(phi_{a_n}), .., value(phi_{a_1}), f
 *               (canonicalised, not quantised), value(gamma_{a_1}), .., value(gamma_{a_n}), then the components P .. K - 1 of the
 *               scores bit for bit.
 *   workspace   dmf_attr_workspace_bytes(H, W, P, n, T) = up16(2 P uint32: the min / max keys of dmf_attr_quantise) + parent
 *               [2 P][T][H W] int32 + size [2 P][T][H W] int32, each of the two rounded up to 16 bytes, in that order; -1 for an
 *               argument out of range.  16-byte aligned, any contents.  dmf_attr_quantise uses (and asks for) the keys alone.
 *               Nothing allocates.
 * Limits: H W < DMF_ATTR_PIXELS_MAX (raster indices are int32; offsets are 64-bit).  All report by code, without a launch (and so
 * with every output as it was): 1 a NULL pointer; 2 H or W < 1, or H W >= DMF_ATTR_PIXELS_MAX; 3 K outside 1..64 or P outside 1..K
 * (area_levels: P outside 1..64); 4 n outside 1..DMF_ATTR_NMAX, or areas that are not strictly increasing and >= 1; 5 pitch < K;
 * 6 a misaligned pointer (fp32: 4 bytes, the workspace: 16); 7 an output overlaps an input or another output; 8 more workgroups
 * than a grid holds, or H W pitch beyond 64-bit byte offsets; 9 a launch itself failed; 10 first_level, levels or T out of range;
 * 11 L outside 2..DMF_ATTR_LEVELS_MAX; 12 the workspace is too small.  (They do not set the text of dmf_last_error.) */
#define DMF_ATTR_NMAX 8
#define DMF_ATTR_BATCH_MAX 16
#define DMF_ATTR_LEVELS_MAX 256
#define DMF_ATTR_PIXELS_MAX 2147483648LL        /* 2^31 */
int64_t dmf_attr_workspace_bytes(int32_t H, int32_t W, int32_t P, int32_t n, int32_t T);
int32_t dmf_attr_quantise(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P, int32_t L,
                          uint8_t* q /* [2 P][H][W] */, float* range /* [P][2] */, void* workspace, int64_t workspace_bytes,
                          void* stream);
int32_t dmf_attr_area_levels(const uint8_t* q, int32_t H, int32_t W, int32_t P, const int32_t* areas /* host [n] */, int32_t n,
                             int32_t L, int32_t first_level, int32_t levels, int32_t T, uint8_t* count /* [2 P][n][H][W] */,
                             void* workspace, int64_t workspace_bytes, void* stream);
int32_t dmf_attr_stack(const float* scores, int32_t H, int32_t W, int32_t K, int64_t pitch, int32_t P, int32_t n, int32_t L,
                       const uint8_t* count, const float* range /* [P][2] */, float* out /* [H][W][K + 2 n P] */, void* stream);

/* ---- several attributes over the same components: `band_profile: area` with `band_profile_diagonals` and / or
 * `band_profile_stds`.  New symbols at an unchanged DMF_VERSION: detect them by name.  Range, quantiser, closing and value() are
 * those above; dmf_attr_quantise and dmf_attr_stack serve unchanged with n = the length of the threshold list.
 *   thresholds  T = areas ++ diagonals ++ stds, n = n_area + n_diag + n_std <= DMF_ATTR_NMAX, HOST memory.  n_area >= 1; each of
 *               the three parts strictly increasing and >= 1 (int32: < 2^31); stds <= L - 1, in quantisation-level units.
 *   opening     for a threshold tau of attribute A, gamma_{A,tau}(q)(x) = the number of levels t in 1..q(x) at which the
 *               4-connected component S of {q >= t} that holds x satisfies crit_A(S, tau):
 *                 area       |S| >= tau                                                        (the criterion above)
 *                 diagonal   w^2 + h^2 >= tau^2, w and h the side lengths in pixels of S's bounding box
 *                 std        |S| sum q^2 - (sum q)^2 >= tau^2 |S|^2, the sums over the pixels of S of THAT PLANE's q (the closing
 *                            planes hold L - 1 - q: the closing side is the dual); the population variance is >= tau^2
 *               all in unsigned 64-bit without a division (csrc/dmf_attr_criteria.h states the functions and why nothing
 *               overflows).  Area and diagonal grow with S, the qualifying levels are 1 .. some t, and the count is the largest
 *               of them (the max rule).  The standard deviation does not grow with S: the count is the subtractive rule of
 *               attribute profiles and in general differs from the largest qualifying level.
 *   count       [2 P][n][H][W] uint8: count[s][i] = gamma_{T_i} of plane s.  The stack's band order per profiled component is
 *               therefore the closings at T_n .. T_1, f, the openings at T_1 .. T_n.
 *   levels      dmf_attr_multi_levels follows dmf_attr_area_levels' batch protocol (first_level 1 STORES count, later calls add;
 *               ascending batches on one stream) with five launches per call (four with n_diag = n_std = 0: there is no identity to
 *               write), nothing read back: the local labelling and the
 *               border links of dmf_attr_area_levels, the identities of the accumulators at the root cells, the root pass
 *               (per run of equal roots in a wave one integer atomic per accumulator: atomicAdd int32, atomicMin / atomicMax
 *               int32, atomicAdd uint64), and the count pass, which evaluates the n criteria at the root's cell.
 *   workspace   dmf_attr_multi_workspace_bytes(H, W, P, n_diag, n_std, T) = dmf_attr_workspace_bytes' layout (keys, parent, size);
 *               then, if n_diag > 0, four int32 planes [2 P][T][H W] (column min, column max, row min, row max); then, if
 *               n_std > 0, two uint64 planes [2 P][T][H W] (sum q, sum q^2); each plane rounded up to 16 bytes.  -1 for an
 *               argument out of range.  With n_diag = n_std = 0 it equals dmf_attr_workspace_bytes.  16-byte aligned, any
 *               contents; a plane set that was not asked for is neither part of it nor touched.
 * Limits and codes as above, and: 4 n_area outside 1..DMF_ATTR_NMAX or areas not strictly increasing and >= 1; 13 n_std > 0 with
 * H W > DMF_ATTR_STD_PIXELS_MAX (the 64-bit products of the std criterion); 14 n_diag or n_std < 0, n > DMF_ATTR_NMAX, diagonals or
 * stds that are not strictly increasing and >= 1, or a std > L - 1.  Every code leaves every output as it was. */
#define DMF_ATTR_STD_PIXELS_MAX 4194304LL       /* 2^22 */
int64_t dmf_attr_multi_workspace_bytes(int32_t H, int32_t W, int32_t P, int32_t n_diag, int32_t n_std, int32_t T);
int32_t dmf_attr_multi_levels(const uint8_t* q, int32_t H, int32_t W, int32_t P, const int32_t* thresholds /* host [n] */,
                              int32_t n_area, int32_t n_diag, int32_t n_std, int32_t L, int32_t first_level, int32_t levels,
                              int32_t T, uint8_t* count /* [2 P][n][H][W] */, void* workspace, int64_t workspace_bytes,
                              void* stream);

/* Replaces image_convert/IHS.py:14-19 `pan2ms` (2x2 mean pool + 2x2 polyphase split) for out [H, W, 4]
 * from pan [>=4H, >=4W] with row pitch `pitch` floats; computed in fp64 like the reference. */
int32_t dmf_pan2ms(const double* pan, int32_t pitch, int32_t H, int32_t W, double* out, void* stream);

/* ---- scene preparation: replaces `to_tensor` + the reflect padding of `data_padding` (function/function.py:99-124) and the
 * float32 / float16 conversions of the resident scene, for a raw scene uploaded in the dtype the readers deliver. */
#define DMF_RAW_U8  0
#define DMF_RAW_U16 1
#define DMF_RAW_I16 2
#define DMF_RAW_I32 3
#define DMF_RAW_F32 4
#define DMF_RAW_F64 5
/* minmax[0..2) <- {min, max} of raw[0..n), in the raw dtype (device memory).  Two launches, the result does not depend on
 * the order of the partial results; a NaN of a float scene propagates as np.min / np.max propagate it.  The partial results
 * live in library-owned device memory: do not run two of these calls at the same time on different streams. */
int32_t dmf_scene_minmax(const void* raw, int32_t dtype, int64_t n, void* minmax, void* stream);
/* out [H + pad, W + pad, C] (fp32, or fp16 when half != 0) <- (raw - min) / (max - min), padded at the bottom and the right by
 * reflection without the edge (BORDER_REFLECT_101 / numpy 'reflect': row i >= H reads row 2 (H - 1) - i; needs pad <= H - 1 and
 * pad <= W - 1).  raw [H, W, C] (C = 1 for a 2-D scene) and minmax as dmf_scene_minmax leaves them.  Bit for bit numpy's
 * result: integer types subtract in the raw type (the caller rules out a max - min that wraps) and divide as float64, f32
 * in float32, f64 in float64; one rounding to fp32, then for half a second one to fp16.  out needs no 16-byte alignment. */
int32_t dmf_scene_prepare(const void* raw, int32_t dtype, int32_t H, int32_t W, int32_t C, const void* minmax, int32_t pad,
                          int32_t half, void* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMF_H */
