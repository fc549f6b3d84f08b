/* C-ABI of libmmnn_sts.so -- the MI355X (gfx950) native compute path of the MMNN_STS multimodal-fusion
 * training step.  Plain C types only: device pointers, sizes, a HIP stream passed as void*.
 *
 * The reference (DigITs-AIML/MMNN_STS) has no FFI of its own: its hot path is the PyTorch module tree
 *   models/densenet.py:151-271  (DenseNet.backbone / .features),  models/mlp.py:7-63,
 *   models/multimodal.py:9-90,  losses/GradientBlender.py:181-205,  losses/losses.py:6-9, utils/utils.py:24-29
 * driven by main.py:460-469 (`model(inputs)`, `computeLoss`, `loss.backward()`).  Each entry point below names the
 * reference code whose arithmetic it replaces; the Python mirror in mmnn_sts_amd/ binds them with ctypes
 * (see INTEGRATION.md for the binding a maintainer of the reference would add).
 *
 * Conventions
 *   - every function returns 0 on success; on failure a non-zero status and mmnn_last_error() (thread-local text).
 *     1 = invalid argument / shape (-> ValueError), 2 = HIP runtime error (-> RuntimeError).  Never aborts.
 *   - the caller (PyTorch) owns every device buffer; the library never allocates, frees or retains device memory.
 *     Workspace sizes come from pure query functions.  All tensors are contiguous fp32, NCDHW.
 *   - threading: the library keeps no mutable state of its own besides the thread-local error text and per-device
 *     "kernel attribute already set" flags (idempotent; written with the value every writer would write).  A PLAN, however, is
 *     a stateful object: it owns host-side job tables (pinned staging buffers) and optional timers; its forward and backward
 *     enqueue every kernel on the caller's stream.  One plan must therefore not be used from two threads at once, and it
 *     belongs to the device that was current when its first forward ran.  Sequential use from different threads is fine
 *     (autograd calls backward from another thread than forward).  Different plans are independent of each other.
 */
#ifndef MMNN_STS_H
#define MMNN_STS_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

int mmnn_version(void);
const char* mmnn_last_error(void);

/* ---- 3-D DenseNet backbone: models/densenet.py:196-231 (conv0 .. norm5) ------------------------------------------ */
typedef struct {
  int32_t in_channels;      /* models/densenet.py:176 */
  int32_t init_features;    /* :179  (<= 64)  */
  int32_t growth_rate;      /* :180  (<= 32)  */
  int32_t bn_size;          /* :182 */
  int32_t num_blocks;       /* len(block_config), :181 */
  int32_t block_config[8];
  float eps;                /* BatchNorm eps (1e-5) */
  float momentum;           /* BatchNorm momentum (0.1) */
  float dropout_prob;       /* :185, nn.Dropout3d after conv2 (:84-85) */
} mmnn_densenet_config;

/* A plan fixes (config, batch, input extent); it owns host-side tables only.  NULL on error. */
void* mmnn_densenet_plan_create(const mmnn_densenet_config* cfg, int32_t n, int32_t d, int32_t h, int32_t w);
void mmnn_densenet_plan_destroy(void* plan);
int64_t mmnn_densenet_param_count(const void* plan);      /* floats in the flat parameter buffer, PyTorch
                                                             named_parameters() order of `backbone` */
int64_t mmnn_densenet_runstat_count(const void* plan);    /* floats in the flat running-stat buffer:
                                                             (running_mean, running_var) per BN in module order */
int64_t mmnn_densenet_workspace_bytes(const void* plan);
int mmnn_densenet_out_shape(const void* plan, int32_t* c, int32_t* d, int32_t* h, int32_t* w);

/* backbone(x): replaces DenseNet.backbone.forward (models/densenet.py:267-268).  training != 0: batch statistics,
 * running-stat update (momentum), channel dropout keyed by `seed`; training == 0: running statistics, no dropout.
 * out: [n][C][d'][h'][w'] = norm5 output. */
int mmnn_densenet_forward(void* plan, const float* params, float* runstats, const float* x, void* workspace, float* out,
                          int32_t training, uint64_t seed, void* stream);
/* autograd adjoint of the above wrt every backbone parameter (main.py:469); needs the workspace of the matching
 * training forward untouched.  grad_params: flat, same layout as params; accumulate != 0 adds into it. */
int mmnn_densenet_backward(void* plan, const float* params, const float* x, void* workspace, const float* grad_out,
                           float* grad_params, int32_t accumulate, uint64_t seed, void* stream);
/* The same backward cut at dense-block boundaries, for data parallelism (there is no counterpart upstream: main.py:336 is single
 * process; the accumulate-then-step rule it implements is main.py:403-407,478-481): runs dense blocks hi_block, hi_block-1, ...,
 * lo_block (0-based).  Calls must walk the blocks downwards without gaps, the first one starting at the last block; the call with
 * lo_block == 0 also runs the stem.  When a call has completed in stream order, the gradients of every parameter of the blocks it
 * covered (and of the transition / norm5 behind each, and of the stem when lo_block == 0) are final in grad_params, so their SUM
 * all-reduce can run while the next call's kernels execute.  mmnn_densenet_backward == one call with (num_blocks-1, 0). */
int mmnn_densenet_backward_range(void* plan, const float* params, const float* x, void* workspace, const float* grad_out,
                                 float* grad_params, int32_t accumulate, uint64_t seed, int32_t hi_block, int32_t lo_block, void* stream);
/* [begin, end) of the flat parameter / gradient buffer owned by dense block `block` (its layers + the transition or norm5 that
 * follows it); block -1: the stem (conv0, norm0).  The ranges tile [0, param_count) in the order stem, block 0, block 1, ... */
int mmnn_densenet_block_param_range(const void* plan, int32_t block, int64_t* begin, int64_t* end);
/* introspection: the ReLU decisions (a*x+b > 0, uint8 [n][C][V]) of one BN+ReLU site of the last training forward.
 * kind 0: relu0 (models/densenet.py:201); 1: denselayer relu1 (:77); 2: relu2 (:81); 3: transition relu (:146).
 * Used by the gradient parity tests (ReLU is not differentiable at 0: a reference must take the same branch). */
int mmnn_densenet_relu_mask(void* plan, const float* params, void* workspace, int32_t kind, int32_t block, int32_t layer,
                            uint8_t* out, void* stream);
/* measurement: time every launch of one kernel class (-1: of every class) with HIP events recorded on the launch stream.
 * kernel_class 0 none, 1 conv2 fwd, 2 conv2 dgrad, 3 conv2 wgrad, 4 conv1 fwd, 5 conv1 dgrad, 6 conv1 wgrad, 7 stem conv,
 * 8 stem wgrad, 9 reserved (accepted, but no launch records it); block >= 0 restricts to one dense block (0-based).  read_timer
 * synchronises the recorded events and returns the accumulated device time and launch count since set_timer (read_timer: all
 * recorded classes and blocks together; read_timer_class: one class (0: all) of one dense block (< 0: all)). */
int mmnn_densenet_set_timer(void* plan, int32_t kernel_class, int32_t block);
int mmnn_densenet_read_timer(void* plan, double* total_ms, int64_t* launches);
int mmnn_densenet_read_timer_class(void* plan, int32_t kernel_class, int32_t block, double* total_ms, int64_t* launches);
/* plan options.  "no_kz" (0/1): never split the channel axis of a small-extent convolution over several workgroups (the tests' reference
 * for the cross-workgroup hand-off).  "single_stream" (any value): accepted and ignored -- the backward always runs on the caller's
 * stream (it once selected between that and side streams for the weight gradients).  "params_version" (any non-zero
 * number the caller changes whenever it changed a parameter; 0 = unknown, the default): the forward re-packs the weights only
 * when the version, the parameter buffer or the workspace differs from the last packed one.  "conv1_dgrad_resident" (0 / 1 / 2, default 1):
 * which dense-layer conv1 data gradients run on the resident-operand kernel (csrc/conv1_dgrad.hip) instead of the general convolution
 * template -- 0 none, 1 the launches where it measured faster (bottleneck width 128, voxel count a multiple of 4, at least 512 voxels per
 * sample in at most 512 tiles of 64 voxels per batch), 2 every launch the kernel can run (tests, measurements). */
int mmnn_densenet_set_option(void* plan, const char* name, int64_t value);
/* nn.BatchNorm3d.num_batches_tracked of every BN of the backbone (module order, int64 [runstat_count / 2 channels ... one per BN]): when set
 * (non-NULL device pointer to `bn_count` int64 values), every training forward adds 1 to each of them in its running-statistics kernel;
 * NULL (the default) leaves the counters to the caller. */
int mmnn_densenet_set_batch_counters(void* plan, int64_t* num_batches_tracked, int32_t bn_count);
/* byte offset of a named workspace region (tests / GradCAM): "x","g","t1","conv0","st_x",... ; -1 if unknown.  Names that start with '#'
 * are counters, not offsets: e.g. "#conv1_dgrad_resident" with i = dense block returns how many layers of that block take the
 * resident-operand conv1 data gradient under the current "conv1_dgrad_resident" option. */
int64_t mmnn_densenet_ws_offset(const void* plan, const char* name, int32_t i, int32_t j);

/* ---- DenseNet.features: ReLU -> AdaptiveAvgPool3d(1) -> flatten -> Linear -> Dropout (models/densenet.py:234-247) ---- */
/* h [n][c][v] (norm5 output), w [f][c], b [f] -> out [n][f]; pooled [n][c] is saved for the backward. */
int mmnn_gap_linear_forward(int32_t n, int32_t c, int32_t v, int32_t f, const float* h, const float* w, const float* b,
                            float* pooled, float* out, float dropout_prob, uint64_t seed, int32_t training, void* stream);
int mmnn_gap_linear_backward(int32_t n, int32_t c, int32_t v, int32_t f, const float* h, const float* w, const float* pooled,
                             const float* dout, float* dw, float* db, float* dh, float dropout_prob, uint64_t seed,
                             int32_t training, int32_t accumulate, void* stream);

/* ---- [Linear -> BatchNorm1d -> ReLU / Dropout1d] stacks: MLP.backbone, MLP.features (models/mlp.py:19-51) ---------- */
#define MMNN_MLP_MAX_LAYERS 8
typedef struct {
  int32_t n;                                  /* batch rows */
  int32_t num_layers;
  int32_t in_dim[MMNN_MLP_MAX_LAYERS];
  int32_t out_dim[MMNN_MLP_MAX_LAYERS];
  int32_t relu_first[MMNN_MLP_MAX_LAYERS];    /* 1: dense-bn-relu-drop (mlp.py:21-24); 0: dense-bn-drop-relu (:25-49) */
  float dropout_prob;                         /* nn.Dropout1d on a 2-D input: whole ROWS are dropped */
  float eps, momentum;
  uint64_t seed;
  int32_t training;
  int32_t first_layer_id;                     /* dropout stream id of layer 0 of this stack */
} mmnn_mlp_desc;
typedef struct {
  const float* weight[MMNN_MLP_MAX_LAYERS];   /* [out][in] */
  const float* bias[MMNN_MLP_MAX_LAYERS];
  const float* gamma[MMNN_MLP_MAX_LAYERS];
  const float* beta[MMNN_MLP_MAX_LAYERS];
  float* running_mean[MMNN_MLP_MAX_LAYERS];
  float* running_var[MMNN_MLP_MAX_LAYERS];
  float* grad_weight[MMNN_MLP_MAX_LAYERS];    /* backward only */
  float* grad_bias[MMNN_MLP_MAX_LAYERS];
  float* grad_gamma[MMNN_MLP_MAX_LAYERS];
  float* grad_beta[MMNN_MLP_MAX_LAYERS];
  int64_t* num_batches_tracked[MMNN_MLP_MAX_LAYERS];   /* optional (NULL: not maintained): nn.BatchNorm1d's step counter, +1 per training forward */
} mmnn_mlp_params;
int64_t mmnn_mlp_saved_floats(const mmnn_mlp_desc* d);      /* size of `saved` */
int mmnn_mlp_forward(const mmnn_mlp_desc* d, const mmnn_mlp_params* p, const float* x, float* out, float* saved, void* stream);
/* scratch: 2 * n * max(dim) floats; dx may be NULL.  The BatchNorm adjoint follows d->training, which must be the flag of the forward
   that wrote `saved`: 1 -- batch statistics, dz = gamma rstd (g - mean_n g - xhat mean_n(g xhat)); 0 -- running statistics, constants
   of the pass, dz = gamma rstd g.  Either way dgamma = sum_n g xhat, dbeta = sum_n g (xhat and rstd as the forward saved them). */
int mmnn_mlp_backward(const mmnn_mlp_desc* d, const mmnn_mlp_params* p, const float* x, const float* saved, const float* dy,
                      float* dx, float* scratch, int32_t accumulate, void* stream);

/* ---- fusion heads (models/multimodal.py:62-77): out[0] = cat(fi,fc) Wf^T + bf; blend: out[1] = image head, out[2] = clinical */
int mmnn_fusion_heads_forward(int32_t n, int32_t f, int32_t c, int32_t blend, const float* fi, const float* fc, const float* wf,
                              const float* bf, const float* wi, const float* bi, const float* wc, const float* bc, float* out,
                              void* stream);
int mmnn_fusion_heads_backward(int32_t n, int32_t f, int32_t c, int32_t blend, const float* fi, const float* fc, const float* wf,
                               const float* wi, const float* wc, const float* dout, float* dfi, float* dfc, float* dwf, float* dbf,
                               float* dwi, float* dbi, float* dwc, float* dbc, int32_t accumulate, void* stream);

/* ---- small dense layer y = x W^T + b: class_layers.out (models/densenet.py:250-256), MLP.output_head (mlp.py:53-57) - */
int mmnn_linear_forward(int32_t n, int32_t d, int32_t o, const float* x, const float* w, const float* b, float* y, void* stream);
int mmnn_linear_backward(int32_t n, int32_t d, int32_t o, const float* x, const float* w, const float* dy, float* dx, float* dw,
                         float* db, int32_t accumulate, void* stream);

/* ---- Cox partial likelihood summed over targets and blended over heads (losses/losses.py:6-9 -> pycox CoxPHLoss,
 * utils/utils.py:24-29, losses/GradientBlender.py:197-205).  preds [heads][n][c]; sort_key / weight [n][c] fp64: pycox's
 * `durations` / `events` arguments (the reference passes events / durations there, in that order; its datasets build them as
 * int64 or float32 tensors, data/ImageDatasets.py:462 -- both are exact in fp64, fractional durations included).  Stable
 * descending sort.
 * Writes loss = sum_h head_weights[h] * head_losses[h] (head_weights NULL: all 1), head_losses[h] = sum_c cox(h, c), and
 * grad_preds = d loss / d preds.  scratch: 4 * n floats. */
int mmnn_cox_blend_loss(int32_t heads, int32_t n, int32_t c, const float* preds, const double* sort_key, const double* weight,
                        const float* head_weights, float* loss, float* head_losses, float* grad_preds, float* scratch, void* stream);

/* The same with sort_key / weight in the element type the caller's tensors already have (the reference's datasets produce int64 and
 * float32, data/ImageDatasets.py:462): no conversion pass.  Every supported type is exact in the kernel's fp64 arithmetic. */
#define MMNN_DT_F64 0
#define MMNN_DT_F32 1
#define MMNN_DT_I64 2
#define MMNN_DT_I32 3
#define MMNN_DT_U8 4
int mmnn_cox_blend_loss_typed(int32_t heads, int32_t n, int32_t c, const float* preds, const void* sort_key, int32_t sort_key_dtype,
                              const void* weight, int32_t weight_dtype, const float* head_weights, float* loss, float* head_losses,
                              float* grad_preds, float* scratch, void* stream);
/* autograd adjoint of (loss, head_losses) wrt preds (main.py:469): grad_preds = grad_saved * dloss[0] + grad_saved[h] * dheads[h] /
 * head_weights[h], where grad_saved is what mmnn_cox_blend_loss wrote.  dloss (1 float) / dheads ([heads]) are device pointers, either may
 * be NULL (that output took no part in the graph). */
int mmnn_cox_blend_backward(int32_t heads, int32_t n, int32_t c, const float* grad_saved, const float* head_weights, const float* dloss,
                            const float* dheads, float* grad_preds, void* stream);

/* ---- element-wise binary cross entropy on logits with per-class positive weights: nn.BCEWithLogitsLoss(pos_weight=...,
 * reduction='none') of the classification trainer (main.py:147-153), the loss behind `criterion` (utils/utils.py:20-22) and
 * GradientBlender.computeLossClassification (losses/GradientBlender.py:150-179).  logits / targets / loss / dloss_dlogits hold
 * `total` floats whose fastest axis is the class axis of length c; pos_weight [c] or NULL; dloss_dlogits may be NULL. */
int mmnn_bce_logits(int64_t total, int32_t c, const float* logits, const float* targets, const float* pos_weight, float* loss,
                    float* dloss_dlogits, void* stream);

/* ---- 3-D ResNet-18 variant (models/resnet.py:5-227).  Generic direct kernels: the net is 8 / 16 channels wide. ---------------- */
typedef struct {
  int32_t n, c_in, d, h, w;      /* input  [n][c_in][d][h][w]  */
  int32_t c_out;                 /* weight [c_out][c_in][kernel...], no bias (Conv3DSimple :95-112, BasicStem :9-11, downsample :176-178) */
  int32_t kernel[3], stride[3], padding[3];
} mmnn_conv3d_desc;
int mmnn_conv3d_out_shape(const mmnn_conv3d_desc* d, int32_t* od, int32_t* oh, int32_t* ow);
int mmnn_conv3d_forward(const mmnn_conv3d_desc* d, const float* x, const float* w, float* y, void* stream);
/* autograd adjoints (main.py:469): dx [n][c_in][d][h][w];  dw [c_out][c_in][kernel...] (accumulate != 0: added to);
 * workspace for the deterministic partial-sum slabs: mmnn_conv3d_wgrad_workspace_bytes(d) bytes */
int mmnn_conv3d_backward_data(const mmnn_conv3d_desc* d, const float* dy, const float* w, float* dx, void* stream);
int64_t mmnn_conv3d_wgrad_workspace_bytes(const mmnn_conv3d_desc* d);
int mmnn_conv3d_backward_weight(const mmnn_conv3d_desc* d, const float* x, const float* dy, float* dw, void* workspace, int32_t accumulate,
                                void* stream);
/* nn.BatchNorm3d [+ residual add] [+ ReLU] [+ element-wise nn.Dropout]: the tail of BasicStem (:12-13), of both halves of a BasicBlock
 * (:74-77, :89-91: `out += residual; out = relu(out)`), of a downsample branch (:179) and the dropout after each stage (:159-166).
 * x / residual / out [n][c][v]; save [2][c] (mean, rstd) and stat_ws (2*c doubles) are caller-provided scratch; training != 0: batch
 * statistics + running-stat update (unbiased variance), training == 0: running statistics, no dropout. */
int mmnn_bn3d_forward(int32_t n, int32_t c, int64_t v, const float* x, const float* gamma, const float* beta, float* running_mean,
                      float* running_var, float momentum, float eps, int32_t training, int32_t relu, const float* residual,
                      float dropout_prob, uint64_t seed, float* out, float* save, double* stat_ws, void* stream);
/* adjoint: dx wrt the BN input, dresidual (may be NULL) wrt the added tensor, dgamma / dbeta [c] (overwritten) */
int mmnn_bn3d_backward(int32_t n, int32_t c, int64_t v, const float* x, const float* out, const float* dout, const float* gamma,
                       const float* save, int32_t training, int32_t relu, float dropout_prob, uint64_t seed, float* dx, float* dresidual,
                       float* dgamma, float* dbeta, double* stat_ws, void* stream);
/* AdaptiveAvgPool3d(1) -> flatten -> Linear(c, o) -> sigmoid (models/resnet.py:152-167); pooled [n][c] is kept for the backward */
int mmnn_gap_fc_sigmoid_forward(int32_t n, int32_t c, int64_t v, int32_t o, const float* x, const float* w, const float* b, float* pooled,
                                float* y, void* stream);
int mmnn_gap_fc_sigmoid_backward(int32_t n, int32_t c, int64_t v, int32_t o, const float* w, const float* pooled, const float* y, const float* dy,
                                 float* dw, float* db, float* dx, void* stream);

/* ---- optimizer step over a flat buffer: torch.optim.SGD(momentum, nesterov, weight_decay) as main.py:410-413 uses it.
 * d = g + wd*p; buf = first_step ? d : momentum*buf + d; p -= lr * (nesterov ? d + momentum*buf : buf) */
int mmnn_sgd_step(float* params, const float* grads, float* momentum_buf, int64_t n, float lr, float momentum, float weight_decay,
                  int32_t nesterov, int32_t first_step, void* stream);

/* The same update for a LIST of small tensors (the ~30 parameter tensors of the MLP, the feature layer and the heads) in ONE launch.
 * momentum_buf is one flat buffer; tensor i owns [flat_offset, flat_offset + count).  first_step is per tensor (torch creates a
 * parameter's momentum buffer at its first step WITH a gradient; tensors without gradient are simply not listed). */
#define MMNN_MULTI_MAX 64
typedef struct {
  float* param;            /* may be NULL for mmnn_multi_copy */
  const float* grad;
  int64_t count;
  int64_t flat_offset;     /* position of this tensor inside the flat momentum / bucket buffer (floats) */
  int32_t first_step;
  int32_t reserved;
} mmnn_tensor_ref;
int mmnn_sgd_step_multi(const mmnn_tensor_ref* refs, int32_t n, float* momentum_buf, float lr, float momentum, float weight_decay,
                        int32_t nesterov, void* stream);
/* scatter == 0: flat[flat_offset + i] = grad[i] (gather the small gradients into ONE all-reduce bucket); scatter != 0: the way back */
int mmnn_multi_copy(const mmnn_tensor_ref* refs, int32_t n, float* flat, int32_t scatter, void* stream);

/* ---- learning-rate range test (upstream utils/find_lr.py: torch-lr-finder's LRFinder.range_test with nn.CrossEntropyLoss) --------
 * nn.CrossEntropyLoss(ignore_index, reduction) over logits [n][c] (1 <= c <= 1024).  target_kind 0: int64 class indices [n] (rows equal
 * to ignore_index are left out; the mean divides by the rows kept, NaN if none); 1: fp32 class probabilities [n][c] (the mean divides
 * by n).  An index outside [0, c) gives a NaN row (loss and gradient) instead of a fault.  reduction 0 none (loss [n]), 1 sum, 2 mean
 * (loss [1]).  dlogits_saved [n][c] (may be NULL): softmax * sum(y) - y, divided by the mean's divisor.  Deterministic: one block,
 * rows reduced in a fixed order.  Backward: dlogits = dlogits_saved * dloss, dloss a device pointer to 1 float (sum / mean) or n
 * (none). */
int mmnn_cross_entropy(int32_t n, int32_t c, const float* logits, const void* target, int32_t target_kind, int64_t ignore_index,
                       int32_t reduction, float* loss, float* dlogits_saved, void* stream);
int mmnn_cross_entropy_backward(int32_t n, int32_t c, int32_t reduction, const float* dlogits_saved, const float* dloss, float* dlogits,
                                void* stream);
/* The sweep's state (mmnn_lr_range_state_bytes(num_iter) bytes, 8-byte aligned): float total @0, int32 live @4, stop_iter @8 (-1: no
 * stop), iters_done @12, num_iter @16; double best @24, prev @32, hist[num_iter] @40.  accumulate: total = (first ? 0 : total) +
 * loss[0] / steps_or_1 in fp32.  update(iter): raw = (double)total; iter 0: best = s = raw; else s = smooth_f * raw +
 * one_minus_smooth_f * prev (raw when smooth_f == 0), best = min(best, s); hist[iter] = s; s > diverge_th * best stops the sweep
 * (live = 0, stop_iter = iter).  Once stopped, accumulate and update change nothing. */
int64_t mmnn_lr_range_state_bytes(int32_t num_iter);
int mmnn_lr_range_init(void* state, int32_t num_iter, void* stream);
int mmnn_lr_range_accumulate(void* state, const float* loss, float steps_or_1, int32_t first, void* stream);
int mmnn_lr_range_update(void* state, int32_t iter, double smooth_f, double one_minus_smooth_f, double diverge_th, void* stream);
/* mmnn_sgd_step / mmnn_sgd_step_multi with the learning rate read from device memory (*lr) and a device switch: *live == 0 leaves
 * params and momentum untouched.  Same per-element code, so a given lr gives bit-identical results. */
int mmnn_sgd_step_dev(float* params, const float* grads, float* momentum_buf, int64_t n, const float* lr, const int32_t* live, float momentum,
                      float weight_decay, int32_t nesterov, int32_t first_step, void* stream);
int mmnn_sgd_step_multi_dev(const mmnn_tensor_ref* refs, int32_t n, float* momentum_buf, const float* lr, const int32_t* live, float momentum,
                            float weight_decay, int32_t nesterov, void* stream);

/* ---- Grad-CAM of the fusion model on the last Conv3d of the image backbone: MultiModalGradCAM.forward after its model forward
 * (utils/utils.py:293-344), batch size 1 (:334).  Per class, in order: d out[0,cls] / d act in closed form (fused head -> feature_layer ->
 * average pool -> ReLU mask -> eval-mode norm5 scale, restricted to the captured layer = the LAST `growth` channels of the concat),
 * channel-pooled gradient (:308-311), the activations weighted by it IN PLACE and therefore cumulatively across classes (:313-314),
 * channel mean, min-max normalisation (:316-323), trilinear up-sampling to the input extent (:339, align_corners = False). */
typedef struct {
  int32_t c_total;          /* channels of the norm5 output */
  int32_t growth;           /* channels of the captured layer (<= 64) */
  int32_t d, h, w;          /* extent of the captured activations */
  int32_t classes;          /* rows of the fused head = Grad-CAM targets (<= 16) */
  int32_t features;         /* width of DenseNet.features' output = the image half of the fused head's input */
  int32_t head_ld;          /* row stride (floats) of the fused head weight (2 * features in the fusion model) */
  int32_t out_d, out_h, out_w;   /* extent of the attention maps = of the input volume */
  float eps;                /* norm5 eps */
} mmnn_gradcam_desc;
/* h5 [c_total][v]: eval-mode norm5 output; act_in [growth][v]: output of the last conv2 (the last channels of the block buffer);
 * w_head [classes][head_ld]; w_feat [features][c_total]; gamma5 / running_var5 [c_total].
 * Writes act [growth][v] (the weighted activations after the last class = `.features`), grads [growth][v] (the gradient of the last class
 * = `.grads`; may be NULL), heat [classes][v] (the normalised low-resolution maps) and maps [classes][out_d][out_h][out_w]. */
int mmnn_gradcam(const mmnn_gradcam_desc* d, const float* h5, const float* act_in, const float* w_head, const float* w_feat,
                 const float* gamma5, const float* running_var5, float* act, float* grads, float* heat, float* maps, void* stream);

/* ---- batched Grad-CAM of an image-only model (what upstream gets from medcam.inject(backend='gcam'), utils/utils.py:451-455;
 * semantics pinned in INTEGRATION.md).  The captured layer A [n][channels][v] is the last Conv3d of the encoder; per sample b and a
 * target t_b (a sum of, one of, or the argmax of the sample's outputs):  d t_b / d A[b][c][v] = s[b][c] * mask[b][c][v] / v  in closed form
 * (no autograd, no weight gradients), alpha[b][c] = mean over v of that gradient, heat[b][v] = ReLU(sum_c alpha[b][c] * A[b][c][v]),
 * min-max normalised per sample (an all-equal map, the all-zero map included, becomes 0, never NaN), trilinear up-sampling to the input
 * extent (align_corners = False).  Samples are independent.  Head families:
 *   MMNN_GC_HEAD_DENSENET  class_layers.out . features.feature_layer . GAP . ReLU . norm5 (eval), A = the last dense layer's conv2 =
 *                          channels [chan_off, chan_off + channels) of the concat buffer; mask = norm5 output > 0 on those channels
 *   MMNN_GC_HEAD_SIGMOID   sigmoid . fc . GAP . ReLU(BN(A) + residual) of r3d_18's last BasicBlock; mask = the block's output > 0 */
#define MMNN_GC_HEAD_DENSENET 0
#define MMNN_GC_HEAD_SIGMOID  1
#define MMNN_GC_LABEL_SUM     (-1)      /* target = sum of the sample's outputs (medcam's default) */
#define MMNN_GC_LABEL_BEST    (-2)      /* target = argmax of the sample's outputs, chosen on the device */
typedef struct {
  int32_t n;                /* samples */
  int32_t channels;         /* channels of the captured layer (<= 64) */
  int32_t d, h, w;          /* extent of the captured layer */
  int32_t out_d, out_h, out_w;   /* extent of the attention maps = of the input volume */
  int32_t classes;          /* model outputs per sample */
  int32_t label;            /* 0 <= label < classes, MMNN_GC_LABEL_SUM or MMNN_GC_LABEL_BEST */
  int64_t act_ns;           /* sample stride (floats) of act: channels * v for a plain tensor, c_total * v inside a concat buffer */
  int64_t mask_ns;          /* sample stride (floats) of mask_src */
} mmnn_gradcam_unimodal_desc;
typedef struct {
  int32_t kind;             /* MMNN_GC_HEAD_* */
  int32_t features;         /* DENSENET: rows of w_feat (width of features.feature_layer); SIGMOID: unused */
  int32_t w_feat_ld;        /* DENSENET: row stride of w_feat (= c_total); SIGMOID: unused */
  int32_t chan_off;         /* first captured channel in w_feat's columns and in gamma / running_var (DENSENET: c_total - growth) */
  const float* w_out;       /* DENSENET: class_layers.out.weight [classes][features]; SIGMOID: fc.weight [classes][channels] */
  const float* w_feat;      /* DENSENET: features.feature_layer.weight [features][w_feat_ld]; SIGMOID: NULL */
  const float* gamma;       /* weight / running_var of the BN after the captured layer (norm5; layer4[-1].conv2[1]) */
  const float* running_var;
  const float* outputs;     /* [n][classes] model outputs (sigmoid probabilities for SIGMOID): the argmax of LABEL_BEST, sigma' */
  float eps;                /* eps of that BN */
} mmnn_gradcam_head;
/* bytes of device scratch mmnn_gradcam_unimodal needs (per-sample gradient scales, per-block partial counts and extrema) */
int64_t mmnn_gradcam_unimodal_workspace_bytes(const mmnn_gradcam_unimodal_desc* d);
/* act: A of sample 0, channel 0 (sample b at act + b * act_ns, channel c at + c * v); mask_src: the mask's source laid out alike.
 * Writes grads [n][channels][v] (d t_b / d A; may be NULL), heat [n][v] (normalised low-resolution maps) and maps [n][out_d][out_h][out_w].
 * Four launches plus the up-sampling, no host synchronisation. */
int mmnn_gradcam_unimodal(const mmnn_gradcam_unimodal_desc* d, const mmnn_gradcam_head* head, const float* act, const float* mask_src,
                          float* grads, float* heat, float* maps, void* ws, int64_t ws_bytes, void* stream);

/* ---- input transforms: upstream's train_transforms / val_transforms (main.py:64-92) on a batch of (C, D, H, W) fp32 volumes
 * (csrc/transforms.hip).  The semantics are pinned by the table in DESIGN §11, not by monai.  `stages` lists the transforms present,
 * in upstream's order; a random stage fires for sample i when its bit is set in per_sample[i].fire.  Every random draw is made by
 * the caller (mmnn_sts_amd/transforms.py); the taps and zoom geometry arrive precomputed.  No host synchronisation. */
#define MMNN_TF_NORMALIZE  (1 << 0)
#define MMNN_TF_SCALE      (1 << 1)
#define MMNN_TF_ROTATE     (1 << 2)
#define MMNN_TF_FLIP       (1 << 3)
#define MMNN_TF_ZOOM       (1 << 4)
#define MMNN_TF_RESIZE     (1 << 5)
#define MMNN_TF_SHIFT      (1 << 6)
#define MMNN_TF_CONTRAST   (1 << 7)
#define MMNN_TF_SMOOTH     (1 << 8)
#define MMNN_TF_SHARPEN    (1 << 9)
#define MMNN_TF_HIST       (1 << 10)
#define MMNN_TF_NOISE      (1 << 11)
#define MMNN_TF_MAX_TAPS   13     /* 2 * radius + 1 for sigma <= 1.5 */
typedef struct {
  int32_t n, c, d, h, w;          /* batch and input extent */
  int32_t out_d, out_h, out_w;    /* Resize target (= d, h, w without MMNN_TF_RESIZE) */
  int32_t stages;                 /* MMNN_TF_* bits */
  float norm_mean, norm_std;      /* Normalize */
} mmnn_transform_desc;
typedef struct {
  int32_t fire;                   /* MMNN_TF_* bits of the random stages that apply to this sample */
  int32_t flip_axis;              /* 0, 1, 2 = D, H, W */
  double theta;                   /* rotation in the (H, W) plane, radians */
  uint64_t noise_seed;            /* noise stream of this sample (keyed further by its batch index and the voxel) */
  int32_t zoom_m[3];              /* zoom: intermediate extent floor(n * z) per axis */
  int32_t zoom_off[3];            /* zoom: output index o reads intermediate index clamp(o + off, 0, m - 1) */
  float shift, gamma, alpha, noise_std;
  float hist_fl[10];              /* histogram-shift control points (reference points: linspace(0, 1, 10)) */
  int32_t smooth_r[3], sharp1_r[3], sharp2_r[3];          /* tap radius per axis D, H, W */
  float smooth_k[3][MMNN_TF_MAX_TAPS];                    /* taps k[-r..r] per axis */
  float sharp1_k[3][MMNN_TF_MAX_TAPS], sharp2_k[3][MMNN_TF_MAX_TAPS];
} mmnn_transform_params;
int64_t mmnn_transform_workspace_bytes(const mmnn_transform_desc* d);
/* in [n][c][d][h][w], out [n][c][out_d][out_h][out_w]; in and out must not overlap; ws >= mmnn_transform_workspace_bytes */
int mmnn_transform_volumes(const mmnn_transform_desc* d, const mmnn_transform_params* per_sample, const float* in, float* out, void* ws,
                           int64_t ws_bytes, void* stream);

/* ---- scan ingest: what upstream's NIfTI datasets do per patient and modality (data/ImageDatasets.py:431-470, :599-637) -- image * mask,
 * removal of every all-zero slice along each axis, Resize((64,64,64)) (area) -- from the file's voxels in their on-disk type to one
 * 64^3 fp32 channel plane (csrc/ingest.hip).  With v(x,y,z) = (slope raw + inter) (mslope mraw + minter), formed in fp64 with a rounded
 * multiply and a rounded add: slice i of an axis is kept when any of its voxels has !(v == 0) (NaN counts as non-zero); the plane is
 * the adaptive average pooling of the compacted volume to 64^3, window sums in fp64, one rounding to fp32.  Tensor axes D, H, W are the
 * array axes x, y, z; the raw buffers are read as stored (x fastest).  A slope of 0, NaN or +-inf means "no scaling" (inter ignored
 * too); a non-finite inter counts as 0.  When the mask leaves nothing (an extent of 0) the plane is written as zeros.
 * Four launches (one of them a memset), no host synchronisation, no floating-point atomics: repeated calls are bit-identical. */
#define MMNN_INGEST_SIZE      64   /* output extent per axis where the caller names none (upstream's Resize target) */
#define MMNN_INGEST_MAX_SIZE  128  /* largest output extent of the _sized calls (16 maps of 128^3 fill a workgroup's 64 KiB of LDS on the way back) */
#define MMNN_INGEST_MAX_X  2048   /* largest x extent (one fp64 column sum per x and wave lives in LDS) */
typedef struct {
  int32_t x, y, z;                /* NIfTI dim[1..3] */
  int32_t scan_type, mask_type;   /* NIfTI datatype codes: 2 uint8, 4 int16, 8 int32, 16 float32, 64 float64, 256 int8, 512 uint16, 768 uint32 */
  float scan_slope, scan_inter;   /* scl_slope / scl_inter of the scan's header */
  float mask_slope, mask_inter;   /* ... of the mask's header */
} mmnn_ingest_desc;
/* bytes of device scratch for a scan of x * y * z voxels (occupancy flags, kept-index lists, extents); -1 on a bad extent.  Needs no GPU. */
int64_t mmnn_ingest_workspace_bytes(int32_t x, int32_t y, int32_t z);
/* scan, mask: device buffers of x*y*z voxels of the given types, aligned to their element size; out_plane: 64^3 floats (a channel of an
 * (N, C, 64, 64, 64) tensor; nothing else is written); extents: 3 int32 on the device = kept slices along x, y, z, valid once the
 * stream has run the call.  ws: once the stream has run the call it holds the kept-index lists and extents of this scan, and stays
 * valid as the `ingest_ws` of mmnn_maps_to_scan (below) until it is reused for another ingest. */
int mmnn_ingest_volume(const mmnn_ingest_desc* d, const void* scan, const void* mask, float* out_plane, int32_t* extents, void* ws,
                       void* stream);
/* The same ingest with the output extent `size` per axis in place of 64: out_plane is size^3 floats (a channel of an
 * (N, C, size, size, size) tensor), the plane is the adaptive average pooling of the compacted volume to size^3, and everything else --
 * the kept slices, `extents`, what `ws` holds afterwards, the launches, the bit-identical repeats -- is as above;
 * mmnn_ingest_volume(d, ...) is mmnn_ingest_volume_sized(d, MMNN_INGEST_SIZE, ...).  The workspace does not depend on `size`.
 * Refused (status 1, mmnn_last_error): what mmnn_ingest_volume refuses, and a size outside 1..MMNN_INGEST_MAX_SIZE. */
int mmnn_ingest_volume_sized(const mmnn_ingest_desc* d, int32_t size, const void* scan, const void* mask, float* out_plane,
                             int32_t* extents, void* ws, void* stream);

/* ---- a mask drawn on another grid -> the scan's grid: what upstream's DICOM datasets do before masking (data/ImageDatasets.py:145-152,
 * :246-257) -- `sitk.Resample(mask, image)` with its defaults (identity transform, linear interpolator, default pixel value 0), then the
 * rebinarisation `mask > 128` -- as one byte per scan voxel (csrc/ingest.hip).  T = index_map takes a scan voxel index to a continuous
 * mask index: inverse(mask affine) * (scan affine), formed by the caller in fp64.  For scan voxel (i, j, k), all in fp64:
 *   coordinates    c_r = T[r][0] i + T[r][1] j + T[r][2] k + T[r][3], r = 0..2.
 *   outside test   the byte is 0 unless -0.5 <= c_r < m_r - 0.5 on all three axes (ITK's buffer test on a continuous index).
 *   interpolation  f_r = floor(c_r), w_r = c_r - f_r; the eight neighbour indices f_r, f_r + 1 are clamped to [0, m_r - 1]; m is the
 *                  trilinear blend (weights 1 - w_r, w_r) of the scaled mask voxels slope raw + inter (the "no scaling" rules of the
 *                  ingest above: a slope of 0, NaN or +-inf switches scaling off, a non-finite inter counts as 0).
 *   binarisation   the byte is 1 when m > threshold, else 0.  A NaN mask voxel therefore gives 0 over its whole neighbourhood -- unlike
 *                  the same-grid ingest above, where a NaN mask voxel counts as non-zero and keeps its slices.
 * Differences from SimpleITK: sitk.Resample casts the interpolated value to the mask's integer pixel type before upstream compares it
 * with 128; here the fp64 value is compared.  `out` holds x*y*z bytes, x fastest, and every byte is written (nothing else is).  One
 * launch, no atomics, no host synchronisation: repeated calls are bit-identical.  The ingest then runs on (scan, out) with mask_type 2,
 * slope 1, inter 0.  Refused (status 1): a non-positive extent, x*y*z or mx*my*mz >= 2^31, an unknown type code, a non-finite
 * index_map entry or threshold, a mask buffer not aligned to its element size. */
typedef struct {
  int32_t x, y, z;                /* scan grid = output grid, NIfTI dim[1..3] */
  int32_t mx, my, mz;             /* mask grid */
  int32_t mask_type;              /* NIfTI datatype code, same set as mmnn_ingest_desc */
  float mask_slope, mask_inter;   /* scl_slope / scl_inter of the mask's header */
  double index_map[12];           /* rows of the 3x4 matrix T */
  double threshold;
} mmnn_resample_mask_desc;
int mmnn_resample_mask(const mmnn_resample_mask_desc* d, const void* mask, uint8_t* out, void* stream);

/* ---- the way back: 64^3 model-space maps (Grad-CAM attention maps) -> fp32 volumes on the scan's voxel grid, so that they overlay the
 * scan once written with its affine (csrc/ingest.hip).  The kept slices are the ingest's own: `ingest_ws` is the workspace a completed
 * mmnn_ingest_volume call for this scan left behind; it is read, never written, and neither the scan nor the mask is read again (so a
 * resampled-mask ingest is inverted by the slices it kept).  With S = 64 and M_r the extent kept along axis r:
 *   dropped voxels a scan voxel whose x, y or z index is not in the kept list of its axis gets exactly 0.0f.
 *   coordinate     otherwise p_r is the rank of its index in the kept list, 0 <= p_r < M_r, and per axis, in fp64:
 *                  s = max((p + 0.5) S / M - 0.5, 0), i0 = min(floor(s), S - 1), i1 = min(i0 + 1, S - 1), w = s - i0.
 *   value          the trilinear blend of the eight map entries (weights 1 - w, w per axis), formed in fp64 and rounded once to fp32:
 *                  F.interpolate(map, size=(Mx, My, Mz), mode='trilinear', align_corners=False) scattered to the kept positions, the
 *                  convention of the Grad-CAM up-sampling (mmnn_gradcam).
 *   empty mask     an extent of 0 gives an all-zero `out`.
 * maps: [n_maps][64][64][64] fp32, tensor axes D, H, W = array axes x, y, z as the ingest writes its plane; out: [n_maps][z][y][x]
 * fp32, x fastest (NIfTI order); every element of it is written and nothing else is.  Two launches (the per-axis tap table, then the
 * pass), no atomics, no host synchronisation: repeated calls are bit-identical.  Refused (status 1): a non-positive extent,
 * x > MMNN_INGEST_MAX_X, x*y*z >= 2^31, n_maps outside 1..MMNN_MAPS_TO_SCAN_MAX_MAPS, a null pointer, a workspace not aligned to 256
 * bytes, maps / out not aligned to 4. */
#define MMNN_MAPS_TO_SCAN_MAX_MAPS 16
typedef struct {
  int32_t x, y, z;                /* the scan's grid = the output grid, NIfTI dim[1..3] */
  int32_t n_maps;                 /* 1..MMNN_MAPS_TO_SCAN_MAX_MAPS */
} mmnn_maps_to_scan_desc;
/* bytes of device scratch (the tap tables of the three axes); -1 on a bad extent.  Needs no GPU. */
int64_t mmnn_maps_to_scan_workspace_bytes(int32_t x, int32_t y, int32_t z);
int mmnn_maps_to_scan(const mmnn_maps_to_scan_desc* d, const void* ingest_ws, const float* maps, float* out, void* ws, void* stream);
/* The same way back for maps of extent `size` per axis: maps is [n_maps][size][size][size] fp32 and S = size in the coordinate rule
 * above; out, the workspace, the launches and the refusals are as above, and mmnn_maps_to_scan(d, ...) is
 * mmnn_maps_to_scan_sized(d, MMNN_INGEST_SIZE, ...).  `ingest_ws` holds the scan's kept slices and nothing of the extent its ingest
 * resized them to, so `size` need not be that ingest's.  Also refused (status 1): a size outside 1..MMNN_INGEST_MAX_SIZE. */
int mmnn_maps_to_scan_sized(const mmnn_maps_to_scan_desc* d, int32_t size, const void* ingest_ws, const float* maps, float* out, void* ws,
                            void* stream);

/* ---- DICOM slice decode: the PixelData bytes of an uncompressed single-frame series, sorted by position -> the raw voxel volume that
 * mmnn_ingest_volume / mmnn_resample_mask take (csrc/dicom.hip).  `pixels` holds the z slices back to back, x (the column) fastest,
 * little-endian words of bits_allocated bits.  Per voxel:
 *   stored value   u = (word >> (high_bit + 1 - bits_stored)) & (2^bits_stored - 1): whatever sits in the unused bits is dropped.
 *   signedness     v = u, or, for is_signed (PixelRepresentation 1), u sign-extended from bit bits_stored - 1.
 *   integer output out_type is the NIfTI code of the (bits_allocated, is_signed) integer type -- 8: 2 / 256, 16: 512 / 4, 32: 768 / 8
 *                  (unsigned / signed) -- and v is stored in that type; slice_scale must be NULL.  A series whose slices share one
 *                  RescaleSlope / RescaleIntercept is decoded this way and the pair handed to the ingest like a NIfTI scl_slope.
 *   float64 output out_type 64: slice k stores (double)v * slice_scale[2k] + slice_scale[2k + 1], a rounded multiply and a rounded add,
 *                  never an FMA (the ingest's rule).  slice_scale: device pointer to [z][2] doubles (RescaleSlope, RescaleIntercept).
 * `out` holds x*y*z elements, x fastest; every element of it is written and nothing else is.  One launch, no atomics, no host
 * synchronisation: repeated calls are bit-identical.  Refused (status 1) before any launch: a null pointer, a non-positive extent,
 * x*y*z >= 2^31, bits_allocated outside {8, 16, 32}, bits_stored outside 1..bits_allocated, high_bit outside bits_stored-1..
 * bits_allocated-1, is_signed outside {0, 1}, an out_type that is neither 64 nor the integer type above, slice_scale inconsistent with
 * out_type, pixels / out not aligned to their element size, overlapping pixels and out. */
typedef struct {
  int32_t x, y, z;                /* Columns, Rows, slices */
  int32_t bits_allocated;         /* 8, 16, 32 */
  int32_t bits_stored;            /* 1..bits_allocated */
  int32_t high_bit;               /* bits_stored-1 .. bits_allocated-1 */
  int32_t is_signed;              /* PixelRepresentation */
  int32_t out_type;               /* NIfTI code of the (bits_allocated, is_signed) integer type, or 64 = float64 */
} mmnn_decode_slices_desc;
int mmnn_decode_slices(const mmnn_decode_slices_desc* d, const void* pixels, const double* slice_scale, void* out, void* stream);

/* ---- DICOM RLE Lossless expansion: the fragments of a sorted single-frame series in transfer syntax 1.2.840.10008.1.2.5 (PS3.5
 * Annex G, PackBits over byte planes) -> exactly the bytes an uncompressed series would hold, i.e. the `pixels` of mmnn_decode_slices:
 * little-endian words of bits_allocated bits, x (the column) fastest, the z frames in order (csrc/dicom_rle.hip, csrc/rle_core.hpp).
 * `payload`: the z fragments back to back as the files hold them (64-byte header included), each start aligned to 16 bytes, payload_bytes
 * in all.  `segments`: DEVICE memory, [z][B][2] int64, B = bits_allocated / 8: the byte offset into `payload` and the byte length of
 * segment s of frame k.  The kernel trusts neither number: it clamps the offset into 0..payload_bytes and the length into what is left.
 *   planes         segment s of a frame holds byte B - 1 - s of every word (the most significant byte plane comes first); a plane has
 *                  exactly x*y bytes.
 *   control byte   n in 0..127 copies the next n + 1 bytes; n in 129..255 repeats the next byte 257 - n times; 128 does nothing.
 *                  Runs may cross row ends (encoders must not do that, decoders must cope).
 *   a full plane   decoding stops when the plane is full: a run that would overfill it is clipped, and whatever is left in the segment
 *                  is ignored, the zero byte that pads a segment to even length included.
 *   a short plane  a run whose bytes (the control byte, then n + 1 literal bytes or the one repeated byte) do not all lie inside the
 *                  segment is cut: it gives no output, even where clipping would have needed fewer bytes, and it ends the segment.  If
 *                  a segment ends, or a run is cut, before the plane is full, status[k] of that frame is 1 and the bytes of that plane
 *                  from there on are written as 0; the frame's other planes and every other frame are unaffected.
 * status[k] is 0 for a frame whose planes were all filled; every status word and every byte of `pixels` is written.  No read ever leaves
 * [payload, payload + payload_bytes) and no write ever leaves `pixels`, `status` or `workspace`, whatever the bytes hold.  `workspace`:
 * mmnn_rle_workspace_bytes bytes (the byte planes before they meet, and their status words); with bits_allocated 8 nothing is kept there.
 * One launch at 8 bits, two otherwise; no atomics, no host synchronisation: repeated calls are bit-identical.  A segment passes through
 * LDS in chunks of MMNN_RLE_CHUNK bytes.  Refused (status 1) before any launch: a null pointer, a non-positive extent, x*y*z >= 2^31,
 * bits_allocated outside {8, 16, 32}, payload_bytes < 1, payload or workspace not aligned to 16 bytes, segments not aligned to 8,
 * status not to 4, pixels not to its element size, pixels or status overlapping payload. */
#define MMNN_RLE_CHUNK 4096
typedef struct {
  int32_t x, y, z;                /* Columns, Rows, slices */
  int32_t bits_allocated;         /* 8, 16, 32 */
  int64_t payload_bytes;
} mmnn_rle_desc;
/* bytes of device scratch; grows with every extent and with bits_allocated; -1 on a bad extent or bits_allocated.  Needs no GPU. */
int64_t mmnn_rle_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t bits_allocated);
int mmnn_rle_expand(const mmnn_rle_desc* d, const void* payload, const int64_t* segments, void* pixels, int32_t* status, void* workspace,
                    void* stream);

/* ---- DICOM JPEG Lossless decode: the entropy-coded data of a sorted single-frame series in transfer syntax 1.2.840.10008.1.2.4.70
 * (T.81 Annex H: process 14, selection value 1) or 1.2.840.10008.1.2.4.57 with predictor 1 -> exactly the bytes an uncompressed series
 * would hold, i.e. the `pixels` of mmnn_decode_slices: little-endian words of bits_allocated bits, x (the column) fastest, the z frames
 * in order (csrc/dicom_jpegll.hip, csrc/jpegll_core.hpp).  `payload`: the z fragments back to back as the files hold them (marker
 * segments included), each start aligned to 16 bytes, payload_bytes in all.  `frames`: DEVICE memory, one record per frame: the byte
 * offset into `payload` and the byte length of what follows the SOS segment, the precision P, and the Huffman table SOS selects as its
 * 16 BITS counts and up to 17 HUFFVALs (unused ones 0).
 *   byte stuffing  inside the data FF 00 stands for the byte FF; FF followed by anything else, or FF as the last byte, ends the data
 *                  there.
 *   codes          canonical, built from BITS / HUFFVAL as T.81 Annex C builds them; the decoded value SSSS lies in 0..16.
 *   differences    (T.81 H.1.2.2, F.2.2.1) SSSS 0: 0.  SSSS 1..15: the next SSSS bits are v, most significant first; the difference is
 *                  v if v >= 2^(SSSS-1), else v - 2^SSSS + 1.  SSSS 16: 32768, and no further bits are read.
 *   prediction     all modulo 2^16: the first sample of the frame is predicted 2^(P-1), every other sample of the first row from its left
 *                  neighbour, the first sample of every later row from the sample above it, every other sample from its left neighbour.
 *                  The stored word is the low bits_allocated bits of prediction + difference.  So the x*y samples are two prefix sums of
 *                  the differences, one down column 0 and one along each row, and that is how they are computed.
 *   a full frame   decoding stops after x*y symbols; whatever follows (pad bits, EOI, trailing bytes) is ignored.
 *   a short frame  a symbol is cut when its code and extra bits do not all lie in front of the end of the data, when its first 16 bits,
 *                  padded with 1-bits behind the end, match no code, or when its decoded value exceeds 16.  A cut symbol gives no output
 *                  and ends the frame: status[k] is 1 and the missing differences count as 0.  Every other frame is unaffected.
 *   trust          nothing in `frames` or `payload` is trusted: offset and length are clamped into the payload, P into 2..16, the BITS
 *                  counts so that they sum to at most 17, and a HUFFVAL above 16 cuts the symbol that decodes to it.  What a table
 *                  that the host reader refuses (over-subscribed, repeated values) decodes to is bounded but otherwise unspecified.
 * status[k] is 0 for a frame that was filled; every status word and every byte of `pixels` is written.  No read ever leaves
 * [payload, payload + payload_bytes) and no write ever leaves `pixels`, `status` or `workspace`, whatever the bytes hold.  `workspace`:
 * mmnn_jpegll_workspace_bytes bytes (the differences as 16-bit words, and every row's first sample).  Two launches; no atomics, no host
 * synchronisation: repeated calls are bit-identical.  A frame's data passes through LDS in chunks of MMNN_JPEGLL_CHUNK bytes as the file
 * holds them (stuffed zeros included).  Refused (status 1) before any launch: a null pointer, a non-positive extent, x*y*z >= 2^31,
 * bits_allocated outside {8, 16}, payload_bytes < 1, payload or workspace not aligned to 16 bytes, frames not aligned to 8, status not
 * to 4, pixels not to its element size, pixels or status overlapping payload. */
#define MMNN_JPEGLL_CHUNK 1024
typedef struct {
  int32_t x, y, z;                /* Columns, Rows, slices */
  int32_t bits_allocated;         /* 8, 16 */
  int64_t payload_bytes;
} mmnn_jpegll_desc;
typedef struct {
  int64_t offset, length;         /* of the entropy-coded data, in `payload` */
  int32_t precision;              /* P of SOF3 */
  uint8_t bits[16];               /* BITS: the number of codes of each length 1..16 */
  uint8_t huffval[17];            /* HUFFVAL: the values in code order */
  uint8_t reserved[3];
} mmnn_jpegll_frame;              /* 56 bytes */
/* bytes of device scratch; grows with every extent; -1 on a bad extent or bits_allocated.  Needs no GPU. */
int64_t mmnn_jpegll_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t bits_allocated);
int mmnn_jpegll_decode(const mmnn_jpegll_desc* d, const void* payload, const mmnn_jpegll_frame* frames, void* pixels, int32_t* status,
                       void* workspace, void* stream);

/* ---- RTSTRUCT contours -> a mask on the scan's grid: the planar polygons of one ROI of an RT Structure Set, already mapped by the host
 * into the scan's continuous voxel index space (a voxel centre sits at the integer index) and assigned to slices, filled into one byte
 * per scan voxel (csrc/rtstruct.hip).  `points`: n_points pairs (px, py) in fp64; `contours`: n_contours pairs (first point, point
 * count), sorted by slice; `slice_first`: z + 1 entries, the contours of slice k are [slice_first[k], slice_first[k + 1]).  Each contour
 * is closed from its last point back to its first.  Voxel (i, j, k) is 1 if and only if an odd number of edges of slice k count for it
 * (the even-odd rule), else 0.  Edge (x0, y0) -> (x1, y1) counts for the voxel when both hold, in fp64:
 *   row test       (y0 <= j && j < y1) || (y1 <= j && j < y0): half open, so a vertex on a row counts once and a horizontal edge never.
 *   side test      i < x0 + (j - y0) * (x1 - x0) / (y1 - y0), every operation rounded on its own (a subtraction, a multiply, a division
 *                  and an addition in that order, never an FMA); a comparison with NaN is false.
 * Contours may leave the grid on any side (they are clipped by construction), may have any orientation and may repeat points; the
 * result does not depend on the order of the contours or of their edges.  `out` holds x*y*z bytes, x fastest -- a mask of NIfTI type 2
 * for mmnn_ingest_volume, slope 1, inter 0 -- and every byte of it is written by the kernel (a slice without contours as zeros, no
 * separate memset); nothing else is.  A contour record that does not lie inside `points`, and a slice range that does not lie inside
 * `contours`, is ignored.  One launch, no atomics on global memory, no host synchronisation: repeated calls are bit-identical.  There
 * is no cap on the points of a slice: its edges pass through LDS in chunks of MMNN_RASTERIZE_CHUNK_EDGES.  n_contours == 0 is legal
 * (an all-zero mask; points and contours may then be null).  Refused (status 1) before any launch: a null descriptor, a non-positive
 * extent, x > MMNN_INGEST_MAX_X, a negative n_contours or n_points, a null slice_first / out, null points / contours with
 * n_contours > 0, a pointer not aligned to its element size. */
#define MMNN_RASTERIZE_CHUNK_EDGES 1024
typedef struct {
  int32_t x, y, z;                /* the scan's grid = the output grid, NIfTI dim[1..3] */
  int32_t n_contours;
  int64_t n_points;
} mmnn_rasterize_desc;
int mmnn_rasterize_contours(const mmnn_rasterize_desc* d, const double* points, const int32_t* contours, const int32_t* slice_first,
                            uint8_t* out, void* stream);

/* ---- DICOM SEG frames -> a byte mask: the PixelData value of a BINARY Segmentation object (PS3.3 C.8.20, one bit per pixel, PS3.5 bit
 * order) unpacked into one byte per voxel of an x * y * z grid (csrc/seg.hip).  `bits` holds the value as the file holds it: pixel
 * p = j*x + i of frame f is bit number (int64)f*x*y + p of the stream, and bit b of the stream is bit b & 7 of byte b >> 3, counted from
 * the least significant.  The frames follow each other WITHOUT byte alignment; the stream holds ceil(n_frames*x*y / 8) bytes, and the
 * padding bits behind the last frame are never read as pixels.  `refs`: n_refs frame indices; `slice_first`: z + 1 entries, the frames
 * of output slice k are refs[slice_first[k] .. slice_first[k + 1]) (the layout mmnn_rasterize_contours uses for its contours).  Voxel
 * (i, j, k) of `out` is `one` if a frame f listed for slice k, with 0 <= f < n_frames, has its bit set, else 0: several frames on one
 * slice are OR-ed, a frame may be listed for several slices, frames need no order, and frames that no slice lists (another segment's)
 * are not read.  A frame index outside 0..n_frames-1 is ignored; so is a slice range that does not lie inside `refs` (not
 * 0 <= first <= last <= n_refs), as a whole.  `out` holds x*y*z bytes, x fastest -- a mask of NIfTI type 2 for mmnn_ingest_volume
 * (one = 1) or mmnn_resample_mask (one = 255) -- and every byte of it is written by the kernel (a slice without frames as zeros, no
 * separate memset); nothing else is.  `bits` and `out` may have any byte alignment; the stream is read in aligned 32-bit words, so the
 * 4-byte cells around its first and last byte are read whole.  One launch, no atomics on global memory, no host synchronisation:
 * repeated calls are bit-identical.  n_refs == 0 is legal (an all-zero mask; bits and refs may then be null).  Refused (status 1)
 * before any launch: a null descriptor, a non-positive extent, x*y*z >= 2^31, a negative n_frames or n_refs, `one` outside 1..255, a
 * null slice_first / out, null bits / refs with n_refs > 0, refs / slice_first not aligned to 4 bytes, overlapping bits and out. */
typedef struct {
  int32_t x, y, z;                /* output grid: Columns, Rows, slices */
  int32_t n_frames;               /* frames held by `bits` */
  int32_t n_refs;                 /* entries of `refs` */
  int32_t one;                    /* byte written for a set voxel, 1..255 */
} mmnn_unpack_frames_desc;
int mmnn_unpack_frames(const mmnn_unpack_frames_desc* d, const uint8_t* bits, const int32_t* refs, const int32_t* slice_first, uint8_t* out,
                       void* stream);

/* ---- row gather: a batch assembled from a table of rows that stays on the device (csrc/gather.hip) -- the ingested planes and kept
 * extents of the patients that the volume cache holds (mmnn_sts_amd/data/cache.py).
 * out row i = table row slots[i], i < n, copied as bit patterns (NaN payloads and -0.0 survive).  table: n_rows rows of row_bytes
 * bytes on the device; slots: n int32 ON THE HOST, read and checked before the launch and passed to the kernel by value; out:
 * n * row_bytes bytes on the device.  Every byte of out is written and nothing else is.  One launch, no atomics, no host
 * synchronisation.  All byte offsets are 64-bit: n_rows * row_bytes may exceed 2^32.  16-byte loads and stores when row_bytes % 16 == 0
 * and table and out are aligned to 16 bytes, dwords otherwise.  The same slot may appear several times.
 * Refused (status 1, mmnn_last_error names the argument) before any launch: a null pointer, n_rows < 1, row_bytes < 4 or not a multiple
 * of 4, n outside 1..MMNN_GATHER_MAX_ROWS, a slot outside 0..n_rows-1, table or out not aligned to 4 bytes, out overlapping the table. */
#define MMNN_GATHER_MAX_ROWS 256
int mmnn_gather_rows(const void* table, int64_t n_rows, int64_t row_bytes, const int32_t* slots, int32_t n, void* out, void* stream);

/* ---- occlusion sensitivity: blank a box of the input, run the model, record how far each output moved; slide the box over the volume
 * and average the moves over the boxes that cover a voxel (csrc/occlusion.hip).  The library builds the occluded batches and assembles
 * the map; the forwards in between are the caller's.
 *   window grid    along an axis of length L with window w and stride s, 1 <= s <= w <= L: n = ceil((L - w) / s) + 1 windows, window i
 *                  starts at o_i = min(i * s, L - w).  The last window is clamped to the edge, so every voxel is covered by at least one
 *                  window, and the windows that cover a voxel form a contiguous index range lo..hi.  Windows are numbered d-major:
 *                  index = (a * n_h + b) * n_w + c; Wn = n_d * n_h * n_w.  s > w would leave holes and is refused.
 * mmnn_occlusion_window_count returns Wn and fills the per-axis counts n_out[3] (d, h, w order; may be null); -1 on a bad descriptor.
 * Needs no GPU.
 * mmnn_occlude_windows: x is (c, d, h, w) fp32, `fill` c floats on the device, out (count, c, d, h, w).  Sample b is a copy of x in
 * which every voxel inside window min(first + b, Wn - 1) is replaced by fill[channel], in all channels; values are copied as bit patterns
 * (NaN payloads and -0.0 survive).  The clamp pads a last short batch with repeats of the last window, so the shape the model sees never
 * changes.  Every element of `out` is written and nothing else is.  One launch, no atomics, no host synchronisation.  16-byte loads and
 * stores when w % 4 == 0 and x and out are aligned to 16 bytes, dwords otherwise.
 * mmnn_occlusion_map: `base` is k floats (the model's outputs on the unoccluded input), `scores` (Wn, k), out (k, d, h, w).  For class j
 * and voxel v, out = (float)( sum((double)base[j] - (double)scores[win][j]) / count ) over the `count` windows that cover v, added in
 * fp64 in ascending (a, b, c) order starting from 0.0, divided in fp64 and rounded to fp32 once: positive where hiding the voxel
 * lowers the output.  One launch, no atomics: repeated calls are bit-identical, and (the library is built without FMA contraction) equal
 * the same statement in numpy.
 * mmnn_channel_means: x is (c, n) fp32, out c floats: each channel's mean, summed in fp64 in a fixed order that depends on n only (two
 * stages: MMNN_CHANNEL_MEANS_PARTS partial sums per channel in `ws`, then their sum), divided by n in fp64 and rounded once.  No atomics:
 * repeated calls are bit-identical.  ws: c * MMNN_CHANNEL_MEANS_PARTS doubles of device scratch.
 * Refused (status 1; the count returns -1) before any launch, with mmnn_last_error() naming the field: a null pointer or descriptor, a
 * non-positive extent, c*d*h*w*count >= 2^31 (for the map d*h*w*k and Wn*k), win outside 1..L, stride outside 1..win, first outside
 * 0..Wn-1, count < 1, k outside 1..MMNN_OCCLUSION_MAX_OUTPUTS, a float pointer not aligned to 4 bytes or a workspace not aligned to 8,
 * x and out overlapping (for the map: out overlapping scores or base). */
#define MMNN_OCCLUSION_MAX_OUTPUTS 16
#define MMNN_CHANNEL_MEANS_PARTS 64
typedef struct {
  int32_t c, d, h, w;             /* the model's input, one sample */
  int32_t win[3];                 /* window per axis, d, h, w order: 1..extent */
  int32_t stride[3];              /* stride per axis, d, h, w order: 1..win */
} mmnn_occlusion_desc;
int64_t mmnn_occlusion_window_count(const mmnn_occlusion_desc* d, int32_t n_out[3]);
int mmnn_occlude_windows(const mmnn_occlusion_desc* d, const float* x, const float* fill, int32_t first, int32_t count, float* out,
                         void* stream);
int mmnn_occlusion_map(const mmnn_occlusion_desc* d, int32_t k, const float* base, const float* scores, float* out, void* stream);
int mmnn_channel_means(const float* x, int32_t c, int64_t n, float* out, void* ws, void* stream);

/* ---- radiomic features of one (scan, mask) pair: first order, the intensity histogram, exact order statistics and the 13 grey-level
 * co-occurrence matrices with 23 features (csrc/radiomics.hip).  Scan and mask hold x*y*z elements, x fastest, in NIfTI types scan_type /
 * mask_type (the codes of mmnn_ingest_desc); a voxel's value is raw * slope + inter in fp64, two roundings, and a slope of 0 or a
 * non-finite slope switches the scaling off, as in the ingest.  The ROI is the voxels whose scaled mask value is not 0.  Everything is
 * in voxel index space: distance 1, no resampling.
 *   discretisation  low = floor(min / bw) * bw;  bin(v) = floor((v - low) / bw) + 1 in fp64, held at 1 from below;  Ng = bin(max).
 *   hist            [max_bins] counts of bin - 1.           glcm  [13][max_bins][max_bins]: direction d (offsets (dz, dy, dx) with the first
 *                   non-zero component positive, in lexicographic order: (0,0,1), (0,1,-1), (0,1,0), (0,1,1), (1,-1,-1), ... (1,1,1)), then
 *                   [a - 1][b - 1]: for every ROI voxel with bin a whose neighbour at the offset lies in the volume and in the ROI with bin
 *                   b, one count at [a][b] and one at [b][a].  Both buffers are the accumulation targets; the call zeroes them first.
 *   result          the block below.  order[2i], order[2i + 1]: the values of rank floor(h), ceil(h), h = (n - 1) * p / 100, for
 *                   p = 10, 25, 50, 75, 90, bitwise the elements of the sorted ROI values (-0.0 counts and is returned as +0.0).
 *                   firstorder: Energy, Minimum, Maximum, Range, Mean, Variance, Skewness, Kurtosis, MeanAbsoluteDeviation,
 *                   RootMeanSquared, 10Percentile, 90Percentile, Median, InterquartileRange, RobustMeanAbsoluteDeviation, Entropy,
 *                   Uniformity (PyRadiomics' definitions, shift 0; RobustMeanAbsoluteDeviation is NaN when no value lies in [p10, p90]).
 *                   glcm: Autocorrelation, JointAverage, ClusterProminence, ClusterShade, ClusterTendency, Contrast, Correlation,
 *                   DifferenceAverage, DifferenceEntropy, DifferenceVariance, JointEnergy, JointEntropy, Imc1, Imc2, Idm, Idmn, Id, Idn,
 *                   InverseVariance, MaximumProbability, SumAverage, SumEntropy, SumSquares: per direction, averaged over the directions
 *                   whose matrix is not empty, NaN when all are.
 *   flags           overflow (Ng > max_bins; n_bins still holds Ng), nonfinite (a NaN / Inf value in the ROI), empty (n = 0).  With a flag
 *                   set every fp64 entry of the result is NaN, hist and glcm are zero, and n, the bounding box and the moments are still
 *                   valid (lo = hi = 0 when empty).
 * The integers are accumulated exactly (uint32 / uint64 atomics, in LDS where the matrix fits); every fp64 sum runs over a partition and
 * in an order that depend on the extents only, without floating-point atomics: repeated calls are bit-identical.  No host wait.
 * ws: mmnn_radiomics_workspace_bytes bytes, aligned to 256.  Refused (status 1; the size returns -1) before any launch: a null pointer, a
 * non-positive extent, x*y*z >= 2^31, max_bins outside 1..MMNN_RADIOMICS_MAX_BINS, an unsupported type code, a bin_width that is not
 * finite and positive, a buffer not aligned to its element size. */
#define MMNN_RADIOMICS_DIRECTIONS 13
#define MMNN_RADIOMICS_FIRSTORDER 17
#define MMNN_RADIOMICS_GLCM 23
#define MMNN_RADIOMICS_MAX_BINS 1024
typedef struct {
  int32_t x, y, z;
  int32_t scan_type, mask_type;   /* NIfTI datatype codes */
  double scan_slope, scan_inter, mask_slope, mask_inter;
  double bin_width;
  int32_t max_bins;
} mmnn_radiomics_desc;
typedef struct {
  int64_t n;
  int64_t lo[3], hi[3];           /* bounding box of the ROI, inclusive, x y z */
  int64_t moments[9];             /* sums over the ROI of x, y, z, xx, yy, zz, xy, xz, yz */
  int64_t n_bins;                 /* Ng */
  int64_t overflow, nonfinite, empty;
  double order[10];
  double firstorder[MMNN_RADIOMICS_FIRSTORDER];
  double glcm[MMNN_RADIOMICS_GLCM];
} mmnn_radiomics_result;
int64_t mmnn_radiomics_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins);
int mmnn_radiomics(const mmnn_radiomics_desc* d, const void* scan, const void* mask, mmnn_radiomics_result* result, uint32_t* hist,
                   uint32_t* glcm, void* ws, void* stream);

/* ---- three more texture classes of the same pair: the grey-level run-length matrix (GLRLM), the grey-level dependence matrix (GLDM)
 * and the neighbouring grey-tone difference matrix (NGTDM) (csrc/radiomics_texture.hip).  The call runs after mmnn_radiomics on the same
 * stream: `ws` and `result` are the workspace and the device result block that a mmnn_radiomics call with the same descriptor has filled
 * earlier on `stream`.  The bin volume (uint16, 0 outside the ROI), Ng, n and the flags are read from the workspace ON THE DEVICE: no
 * host wait, no read-back (`result` is checked like the other pointers and names the call this one belongs to).  Distance 1, the 26
 * neighbours, alpha = 0, levels i = 1..Ng, lengths / dependences j from 1, eps = 2^-52.  L = max(x, y, z).
 *   glrlm    [13][max_bins][L] uint32, the directions of mmnn_radiomics in its order.  A run is a maximal set of consecutive voxels along
 *            the direction that all lie in the volume and in the ROI and share one bin; one count at [d][bin - 1][length - 1].  Every ROI
 *            voxel is in exactly one run per direction: sum_j j P(i, j) = hist[i].
 *   gldm     [max_bins][27] uint32: an ROI voxel of bin i counts at [i - 1][k], k the number of its 26 neighbours in the volume and in the
 *            ROI with the same bin; the dependence is j = k + 1.
 *   ngtdm_n  [max_bins][27] uint32, ngtdm_s [max_bins][27] uint64: an ROI voxel of bin i with c of its 26 neighbours in the volume and in
 *            the ROI, their bins summing to B, adds 1 at n[i - 1][c] and |i c - B| at s[i - 1][c].  So n_i = sum_{c=1..26} n[i][c] and
 *            s_i = sum_{c=1..26} s[i][c] / c, exact up to that division; column 0 (no neighbour) is counted and enters no feature.
 *   The four tables are the accumulation targets; the call zeroes them first, and they are exact.
 *   out.glrlm  per direction, averaged over the 13 (none is empty when n > 0).  P(i, j) the count, Nr = sum P, p = P / Nr, pg(i) = sum_j P,
 *            pr(j) = sum_i P, Np = n, mu_g = sum i pg / Nr, mu_r = sum j pr / Nr:
 *            ShortRunEmphasis sum pr / j^2 / Nr; LongRunEmphasis sum pr j^2 / Nr; GrayLevelNonUniformity sum pg^2 / Nr;
 *            GrayLevelNonUniformityNormalized sum pg^2 / Nr^2; RunLengthNonUniformity sum pr^2 / Nr; RunLengthNonUniformityNormalized
 *            sum pr^2 / Nr^2; RunPercentage Nr / Np; GrayLevelVariance sum (pg / Nr)(i - mu_g)^2; RunVariance sum (pr / Nr)(j - mu_r)^2;
 *            RunEntropy -sum sum p log2(p + eps); LowGrayLevelRunEmphasis sum pg / i^2 / Nr; HighGrayLevelRunEmphasis sum pg i^2 / Nr;
 *            ShortRunLowGrayLevelEmphasis sum sum P / (i^2 j^2) / Nr; ShortRunHighGrayLevelEmphasis sum sum P i^2 / j^2 / Nr;
 *            LongRunLowGrayLevelEmphasis sum sum P j^2 / i^2 / Nr; LongRunHighGrayLevelEmphasis sum sum P i^2 j^2 / Nr.
 *   out.gldm   one matrix, Nz = sum P = n, pg and pd the marginals, p = P / Nz: SmallDependenceEmphasis sum pd / j^2 / Nz;
 *            LargeDependenceEmphasis sum pd j^2 / Nz; GrayLevelNonUniformity sum pg^2 / Nz; DependenceNonUniformity sum pd^2 / Nz;
 *            DependenceNonUniformityNormalized sum pd^2 / Nz^2; GrayLevelVariance; DependenceVariance; DependenceEntropy
 *            -sum sum p log2(p + eps); LowGrayLevelEmphasis sum pg / i^2 / Nz; HighGrayLevelEmphasis sum pg i^2 / Nz;
 *            SmallDependenceLowGrayLevelEmphasis sum sum P / (i^2 j^2) / Nz; SmallDependenceHighGrayLevelEmphasis sum sum P i^2 / j^2 / Nz;
 *            LargeDependenceLowGrayLevelEmphasis sum sum P j^2 / i^2 / Nz; LargeDependenceHighGrayLevelEmphasis sum sum P i^2 j^2 / Nz.
 *   out.ngtdm  Nvp = sum n_i, p_i = n_i / Nvp, Ngp = #{i: n_i > 0}, double sums over the pairs with n_i > 0 and n_j > 0:
 *            Coarseness 1 / sum p_i s_i (10^6 when that sum is 0); Contrast [sum sum p_i p_j (i - j)^2 / (Ngp (Ngp - 1))] [sum s_i / Nvp]
 *            (0 when Ngp = 1); Busyness sum p_i s_i / sum sum |i p_i - j p_j| (0 when the denominator is 0); Complexity
 *            sum sum |i - j| (p_i s_i + p_j s_j) / (p_i + p_j) / Nvp; Strength sum sum (p_i + p_j)(i - j)^2 / sum s_i (0 when sum s_i = 0).
 *            All five are NaN when Nvp = 0 (a single voxel, isolated voxels only).
 *   flags    with overflow, nonfinite or empty set by mmnn_radiomics every fp64 of `out` is NaN and the four tables are zero.
 * Where the tables live while they are counted: the run-length matrix of a direction in LDS when Ng * L <= 16384 (64 KiB), the three
 * neighbourhood tables in LDS when Ng <= 128 (54 KiB); uint32 / uint64 atomics on global memory beyond.  Every fp64 sum runs over a
 * partition and in an order fixed by the extents and Ng alone, without floating-point atomics: repeated calls are bit-identical.
 * ws2: mmnn_radiomics_texture_workspace_bytes bytes, aligned to 256.  Refused as mmnn_radiomics refuses (status 1; the size returns -1),
 * before any launch: a null pointer, a bad extent, max_bins, type code or bin_width, a buffer not aligned to its element size.
 * The size-zone matrix and the mesh-based shape features are the calls below; the GLCM's MCC is not computed. */
#define MMNN_RADIOMICS_GLRLM 16
#define MMNN_RADIOMICS_GLDM 14
#define MMNN_RADIOMICS_NGTDM 5
#define MMNN_RADIOMICS_NEIGHBOURS 27
typedef struct {
  double glrlm[MMNN_RADIOMICS_GLRLM];
  double gldm[MMNN_RADIOMICS_GLDM];
  double ngtdm[MMNN_RADIOMICS_NGTDM];
} mmnn_radiomics_texture_result;
int64_t mmnn_radiomics_texture_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins);
int mmnn_radiomics_texture(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws,
                           mmnn_radiomics_texture_result* out, uint32_t* glrlm, uint32_t* gldm, uint32_t* ngtdm_n, uint64_t* ngtdm_s,
                           void* ws2, void* stream);

/* ---- the grey-level size-zone matrix (GLSZM) of the same pair, from a connected-component labelling on the device
 * (csrc/radiomics_zones.hip).  The call runs after mmnn_radiomics on the same stream, like mmnn_radiomics_texture: `ws` and `result` are
 * the workspace and the device result block that a mmnn_radiomics call with the same descriptor has filled earlier on `stream`.  The bin
 * volume (uint16, 0 outside the ROI), Ng, n and the flags are read from the workspace ON THE DEVICE: no host wait, no read-back.
 *   zones    a zone is a maximal set of ROI voxels that share one bin and are connected through the 26 neighbours inside the volume
 *            (PyRadiomics' default in 3-D: the 13 directions at distance 1).  The neighbour test is made on (x, y, z): the last voxel of a
 *            row or slice never connects to the first of the next.
 *   labels   [x*y*z] uint32 in the scan's layout: 0 outside the ROI, otherwise 1 + the smallest linear index among the voxels of the
 *            voxel's zone.  The label is canonical: it does not depend on the order in which the zones were merged.
 *   sizes    [x*y*z] uint32: the zone's voxel count at its smallest-index voxel, 0 everywhere else.  sum sizes = n.
 *   levels   [max_bins] uint32: pg(i), the number of zones of bin i + 1.
 *   The three tables are the accumulation targets; the call zeroes them first, and they are exact.
 *   out      P(i, j) the number of zones of level i and size j, Nz = sum P, Np = n, pg(i) = sum_j P, ps(j) = sum_i P, p = P / Nz,
 *            mu_i = sum i pg / Nz, mu_j = sum j ps / Nz = n / Nz, eps = 2^-52.  The six integers, exact (all below 2^62: n < 2^31,
 *            sum ps^2 <= Nz^2, sum over zones of size^2 <= n^2): nz = Nz; n_keys, the number of distinct (i, j) with P > 0; max_size;
 *            sum_pg2 = sum_i pg^2; sum_ps2 = sum_j ps^2; sum_j2 = sum over zones of size^2 = sum_j ps j^2.  glszm, in this order:
 *            SmallAreaEmphasis sum ps / j^2 / Nz; LargeAreaEmphasis sum ps j^2 / Nz; GrayLevelNonUniformity sum pg^2 / Nz;
 *            GrayLevelNonUniformityNormalized sum pg^2 / Nz^2; SizeZoneNonUniformity sum ps^2 / Nz; SizeZoneNonUniformityNormalized
 *            sum ps^2 / Nz^2; ZonePercentage Nz / Np; GrayLevelVariance sum (pg / Nz)(i - mu_i)^2; ZoneVariance sum (ps / Nz)(j - mu_j)^2;
 *            ZoneEntropy -sum sum p log2(p + eps); LowGrayLevelZoneEmphasis sum pg / i^2 / Nz; HighGrayLevelZoneEmphasis sum pg i^2 / Nz;
 *            SmallAreaLowGrayLevelEmphasis sum sum P / (i^2 j^2) / Nz; SmallAreaHighGrayLevelEmphasis sum sum P i^2 / j^2 / Nz;
 *            LargeAreaLowGrayLevelEmphasis sum sum P j^2 / i^2 / Nz; LargeAreaHighGrayLevelEmphasis sum sum P i^2 j^2 / Nz.
 *            One matrix: nothing is averaged over directions, and no feature degenerates while n > 0.
 *   flags    with overflow, nonfinite or empty set by mmnn_radiomics the 16 doubles are NaN, the six integers and the three tables zero.
 * How it is built: union-find on a parent array in ws3 (every write is an atomic minimum with a smaller index, so parent[v] <= v always
 * holds, every walk and retry is bounded and the final root is the zone's smallest index); P never exists densely: the distinct (i, j)
 * are at most sqrt(2 n Ng) <= sqrt(2 x y z max_bins), and they are counted in an open-addressing table in ws3 of the next power of two
 * above twice that bound, which therefore never fills; a second table keyed by j holds ps.  Both live in global memory at every Ng.
 * The integers are accumulated exactly (uint32 / uint64 atomic add, minimum and maximum); every fp64 sum runs over the distinct keys in a
 * partition and an order fixed by the extents, Ng and the exact integer tables alone, without floating-point atomics: repeated calls are
 * bit-identical.  ws3: mmnn_radiomics_zones_workspace_bytes bytes, aligned to 256.  Refused as mmnn_radiomics_texture refuses (status 1;
 * the size returns -1), before any launch: a null pointer, a bad extent, max_bins, type code or bin_width, a buffer not aligned to its
 * element size.  Zones per slice (2-D), other distances and the GLCM's MCC are not computed; the mesh-based shape features are the
 * call below. */
#define MMNN_RADIOMICS_GLSZM 16
typedef struct {
  int64_t nz;        /* number of zones = sum P */
  int64_t n_keys;    /* number of distinct (level, size) pairs */
  int64_t max_size;  /* largest zone */
  int64_t sum_pg2;   /* sum_i pg(i)^2 */
  int64_t sum_ps2;   /* sum_j ps(j)^2 */
  int64_t sum_j2;    /* sum over zones of size^2 */
  double glszm[MMNN_RADIOMICS_GLSZM];
} mmnn_radiomics_zones_result;
int64_t mmnn_radiomics_zones_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins);
int mmnn_radiomics_zones(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws,
                         mmnn_radiomics_zones_result* out, uint32_t* labels, uint32_t* sizes, uint32_t* levels,
                         void* ws3, void* stream);

/* ---- the surface mesh of the same ROI and what the eight mesh-based shape features need from it (csrc/radiomics_mesh.hip).  The call
 * runs after mmnn_radiomics on the same stream, like the two above: `ws` and `result` are the workspace and the device result block that
 * a mmnn_radiomics call with the same descriptor has filled earlier on `stream`.  The bin volume (uint16, 0 outside the ROI), the flags and
 * the ROI's bounding box are read ON THE DEVICE: no host wait, no read-back, and no triangle is ever stored.
 *   mesh     The ROI (bin != 0) is padded with one layer of empty voxels on every side, in thought only: a corner outside the volume
 *            reads as empty and nothing is allocated for it.  A cell is a 2 x 2 x 2 block of corners with origin o in -1 .. extent - 1
 *            per axis; corner k of a cell is o + (k & 1, k >> 1 & 1, k >> 2 & 1) in (x, y, z), and bit k of the cell's configuration
 *            says whether that corner is in the ROI.  Coordinates are DOUBLED voxel indices (voxel i at 2 i).
 *            vertices: every cell edge whose two corners differ carries one vertex at its midpoint, an integer triple.  Edge
 *            4 a + p + 2 q runs along axis a (x 0, y 1, z 2) at the position (p, q) of the two other axes in ascending order.
 *            segments: on each of the six faces the four corners are visited counter-clockwise as seen from outside the cell; every
 *            maximal run of set corners is cut off by one directed segment from the crossing where the run starts to the crossing
 *            where it ends (two diagonally opposite set corners get two segments that separate them).
 *            loops: every vertex ends one segment and starts another, so the segments form disjoint closed loops.
 *            triangles: a loop is rotated to start at its lowest-numbered edge v0 and cut into the fan (v0, v_i, v_i+1); a cell's loops
 *            are taken in the order of their lowest edge.  At most 5 triangles per cell.
 *            orientation: as directed above the normals (b - a) x (c - a) point out of the ROI; the signed volume is positive.
 *            A face's segments depend on that face's four corners alone, so neighbouring cells agree and the mesh is closed: every
 *            directed edge occurs as often as its reverse (an undirected edge can be used more than twice, where two sheets touch).
 *            The table is generated from this rule (tools/gen_mesh_table.py -> csrc/mesh_table.hpp); mmnn_radiomics_mesh_table returns
 *            the copy the library was built with, on the host: tri [256][16] (edge numbers, -1 behind the last triangle, the triangle
 *            count in [15]), l48 [256] and nsum [256][3] (below).
 *   cfg      [256] uint64: the number of cells per configuration, all (x + 1)(y + 1)(z + 1) cells counted.  The accumulation target;
 *            the call zeroes it first.  Exact.
 *   out      n_vertices; n_triangles = sum_c cfg[c] T_c; volume48 = sum over the triangles of a . (b x c) in doubled coordinates
 *            = 48 x the mesh volume in voxels.  All exact.  With l48[c] = sum a . (b x c) and nsum[c] = sum (b - a) x (c - a) over the
 *            triangles of configuration c in coordinates relative to the cell, a cell at origin o adds l48[c] + 2 o . nsum[c]; o is
 *            taken relative to the ROI's bounding box (the mesh is closed, so the sum does not depend on the origin) and the sum runs
 *            modulo 2^64, which cannot touch a value of at most 48 n.
 *            area = sum_c cfg[c] A_c in index order c = 0 .. 255, A_c = sum over the triangles of c in table order of |cof(L) n| / 8,
 *            n = (b - a) x (c - a) the integer normal, cof(L) the cofactor matrix of `linear` ((L a) x (L b) = cof(L) (a x b)), each
 *            row applied as (C0 nx + C1 ny) + C2 nz, the norm as sqrt((w0^2 + w1^2) + w2^2).  In the squared units of `linear`.
 *            q[4]: squared diameters in doubled units.  Every vertex v is mapped to t_r = (L[r][0] vx + L[r][1] vy) + L[r][2] vz; a pair
 *            scores q = ((dt0)^2 + (dt1)^2) + (dt2)^2.  q[0] is the largest q over all unordered vertex pairs, self-pairs included (so a
 *            class with no other pair gives 0, never NaN); q[1], q[2], q[3] over the pairs whose integer z, y and x coordinate agrees:
 *            Maximum2DDiameterSlice, Column and Row in the (x, y, z) order of the scan's array -- Slice holds z fixed, Column y, Row x.
 *            (PyRadiomics names its axes after its own array order; that naming is not checked here.)  A diameter is sqrt(q) / 2.
 *            The four are maxima, the file is built without contraction: they are bit-identical to the restatement's and from call
 *            to call, although the order of the vertex list in ws4 is not fixed.
 *            (Specified while every t_r is finite: a `linear` so large that L v overflows is the caller's error.)
 *   flags    with overflow, nonfinite or empty set by mmnn_radiomics the five doubles are NaN, the three integers and cfg zero.
 * linear: 9 doubles ON THE HOST, row-major, the 3 x 3 linear part of the voxel index -> mm affine; read during the call.
 * Integers by uint32 / uint64 atomic add and maximum (the maxima on the bit patterns of non-negative doubles); no floating-point atomics.
 * ws4: mmnn_radiomics_mesh_workspace_bytes bytes, aligned to 256: the vertex list, three uint32 per vertex for 3 (x + 1)(y + 1)(z + 1)
 * vertices, the most a volume can have.  Refused as mmnn_radiomics_zones refuses (status 1; the size returns -1), before any launch: a
 * null pointer, a bad extent, max_bins, type code or bin_width, a buffer not aligned to its element size; and a null or non-finite
 * `linear`.  Pruning the pair search to hull-extreme vertices is not done.  The GLCM's MCC is not computed. */
typedef struct {
  int64_t n_vertices;
  int64_t n_triangles;
  int64_t volume48;  /* 48 x the mesh volume in voxels */
  double area;       /* in the squared units of `linear` */
  double q[4];       /* squared diameters, doubled units: all pairs, z fixed (Slice), y fixed (Column), x fixed (Row) */
} mmnn_radiomics_mesh_result;
int64_t mmnn_radiomics_mesh_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t max_bins);
int mmnn_radiomics_mesh(const mmnn_radiomics_desc* d, const mmnn_radiomics_result* result, const void* ws, const double* linear,
                        mmnn_radiomics_mesh_result* out, uint64_t* cfg, void* ws4, void* stream);
int mmnn_radiomics_mesh_table(int8_t* tri, int32_t* l48, int32_t* nsum);

/* ---- the Laplacian-of-Gaussian image type of the radiomics path: a separable 3-D FIR with spacing-dependent taps, fp64 accumulation and
 * edge replication (csrc/radiomics_filter.hip).  `scan` holds x*y*z elements, x fastest, in NIfTI type scan_type; a voxel's value v is
 * raw * scan_slope + scan_inter in fp64, the type codes and the rule exactly those of mmnn_radiomics_desc (a slope of 0 switches the
 * scaling off).  `out` is [z][y][x] float32, x fastest, every element written: it is a scan of type 16 with slope 0 for mmnn_radiomics.
 *   taps     a device buffer of fp64: for each axis a = x, y, z in turn g_a[2 r_a + 1] (the smoothing taps) and then h_a[2 r_a + 1] (the
 *            second-derivative taps), r_a = radius[a].  The caller computes them; the library never calls exp.
 *   weight   w_x, w_y, w_z: what each axis' second derivative is multiplied by (sigma^2 / spacing_a^2 for the scale-normalised mm
 *            Laplacian).
 *   arithmetic  all fp64, product then sum with no contraction; every sum runs over the taps t = -r .. +r in ascending order, starting
 *            from +0.0, and a source index outside the volume is clamped to it (edge replication):
 *              x pass   A0 = sum g_x[t] v(x + t)                       A2 = sum h_x[t] v(x + t)
 *              y pass   B0 = sum g_y[t] A0(y + t)                      C  = (sum g_y[t] A2(y + t)) w_x + (sum h_y[t] A0(y + t)) w_y
 *              z pass   out = (float)( sum g_z[t] C(z + t) + (sum h_z[t] B0(z + t)) w_z )
 *            The intermediates are fp64 and the result is rounded to fp32 once.  A non-finite voxel propagates to every output within
 *            its radii.  A radius may exceed the extent of its axis.
 * One lane per output and no atomics: repeated calls are bit-identical, and so is a restatement that follows the order above.  No host
 * wait.  ws: mmnn_log_filter_workspace_bytes bytes, aligned to 256: the four fp64 intermediates.  Refused (status 1; the size returns -1)
 * before any launch: a null pointer, a non-positive extent, x*y*z >= 2^31, an unsupported type code, a radius outside
 * 1..MMNN_LOG_FILTER_MAX_RADIUS, a non-finite weight, a scan not aligned to its element size, taps not aligned to 8, out not to 4, ws
 * not to 256.  The largest radius is what the y / z tile with its two halos takes of the LDS: 62.8 KiB of a CU's 160. */
#define MMNN_LOG_FILTER_MAX_RADIUS 88
typedef struct {
  int32_t x, y, z;
  int32_t scan_type;              /* NIfTI datatype code */
  double scan_slope, scan_inter;
  int32_t radius[3];              /* x, y, z */
  double weight[3];               /* x, y, z */
} mmnn_log_filter_desc;
int64_t mmnn_log_filter_workspace_bytes(int32_t x, int32_t y, int32_t z);
int mmnn_log_filter(const mmnn_log_filter_desc* d, const void* scan, const double* taps, float* out, void* ws, void* stream);

/* ---- the two optional pre-steps of the radiomics path, in PyRadiomics' order: normalise the scan's intensities, then resample the
 * (scan, mask) pair to a stated voxel spacing (csrc/radiomics_resample.hip).  Each returns a new scan of type 16 with slope 0 (and the
 * second a byte mask) that mmnn_radiomics, its follow-on calls and mmnn_log_filter take like any other.  **Parity with PyRadiomics is
 * unpinned**: no test compares with it; its B-spline is ITK's, and it crops the resampled grid to the ROI's bounding
 * box plus padding, where this resamples the whole scan.
 *
 * mmnn_normalize_scan.  `scan` holds x*y*z elements, x fastest, in NIfTI type scan_type; a voxel's value v is raw * scan_slope +
 * scan_inter in fp64 under the rule of mmnn_radiomics_desc (a slope of 0 switches the scaling off).  The statistics are those of the
 * WHOLE scan (n = x*y*z), not of an ROI, as PyRadiomics takes them:
 *   mean = (sum v) / n;   sd = sqrt(sum (v - mean)^2 / (n - 1)), a second pass over the scan with the first one's mean.  (The n - 1
 *   divisor is believed to be what ITK's statistics filter uses; that belief is unpinned.)
 *   out = (float)(((v - mean) / sd) * scale), one rounding to fp32; with outliers = k > 0 the fp64 value is clamped to
 *   [-k scale, +k scale] before that rounding (a NaN stays a NaN).  `out` is [z][y][x] float32, every element written.
 *   result (on the device, nothing is read back): n, mean, sd, and nonfinite = 1 when any voxel is NaN or infinite.
 * A non-finite voxel makes mean or sd NaN and with them EVERY output; so does a scan of one voxel (0 / 0) and a constant scan whose sums
 * are exact (sd = 0, 0 / 0: integer types; a constant whose fp64 mean rounds leaves a tiny non-zero sd and finite, meaningless outputs,
 * which nothing detects).  mmnn_radiomics then finds non-finite values inside the mask and sets its nonfinite flag.
 * The two fp64 sums: workgroup p of P = min(256, ceil(n / 256)) adds the voxels p 256 + t + k P 256 (lane t, k ascending) per lane,
 * folds the workgroup by block_reduce (csrc/reduce.hpp: the lanes of each wave by the xor butterfly, then the waves in index order), and
 * the P partial sums, part p in lane p, are folded by one more block_reduce: a partition and an order fixed by the extents alone, no floating-point atomics, repeated calls are bit-identical.  No host wait.
 * ws: mmnn_normalize_scan_workspace_bytes bytes, aligned to 256.  Refused (status 1, nothing written; the size returns -1) before any
 * launch: a null pointer, a non-positive extent, x*y*z >= 2^31, an unsupported type code, a scale that is not finite and positive, an
 * outliers that is negative or not finite, a scan not aligned to its element size, out not to 4, result not to 8, ws not to 256. */
typedef struct {
  int32_t x, y, z;
  int32_t scan_type;              /* NIfTI datatype code */
  double scan_slope, scan_inter;
  double scale;                   /* what the z-score is multiplied by */
  double outliers;                /* 0: no clamp; k > 0: clamp to [-k scale, +k scale] */
} mmnn_normalize_desc;
typedef struct {
  int64_t n;
  double mean, sd;
  int64_t nonfinite;
} mmnn_normalize_result;
int64_t mmnn_normalize_scan_workspace_bytes(int32_t x, int32_t y, int32_t z);
int mmnn_normalize_scan(const mmnn_normalize_desc* d, const void* scan, float* out, mmnn_normalize_result* result, void* ws, void* stream);

/* mmnn_resample_pair.  `scan` and `mask` hold x*y*z elements each, as above; `out` is [mz][my][mx] float32 and `out_mask` [mz][my][mx]
 * bytes, every element of both written.  The caller decides the output grid and states it in per-axis tables; the library calls
 * neither floor on a coordinate nor any power.
 *   tables   mx + my + mz entries of mmnn_resample_entry (56 bytes each, no padding): those of the x axis, then y, then z.  Entry j of
 *            an axis of source extent n whose output sample j sits at the continuous source index c: with f = floor(c), t = c - f,
 *              i[k]     mirror(f - 1 + k), k = 0..3: the whole-sample symmetric reflection, period 2 n - 2 (0 when n = 1)
 *              w[k]     the cubic B-spline weights (1-t)^3/6, 2/3 - t^2 (2-t)/2, 2/3 - (1-t)^2 (1+t)/2, t^3/6
 *              nearest  clamp(floor(c + 0.5), 0, n - 1): where the mask is read
 *              inside   0 when c < -0.5 or c >= n - 0.5 (ITK's buffer test), otherwise 1
 *            `tables` is the copy on the device, which the kernels read; `tables_host` the same bytes on the host, read during the call
 *            to refuse an index outside its axis before anything is launched.
 *   prefilter  the scan becomes cubic B-spline coefficients in fp64, one volume in ws, by the recursion below along every line of x,
 *            then of y, then of z; an axis of extent 1 is left as it is.  z = pole (sqrt(3) - 2), pole_gain = z / (z^2 - 1), gain = 6,
 *            pole_power[k] = z^k, k = 0 .. H - 1, H = MMNN_RESAMPLE_HORIZON: all from the descriptor.  |z|^40 = 1.3e-23 is below fp64
 *            resolution, so one horizon serves every axis length.  Every product is rounded before its sum, no contraction:
 *              s[k]     = gain v[k]
 *              c+[0]    = sum_{k = 0 .. H-1, ascending from +0.0} pole_power[k] s[mirror(k)]
 *              c+[k]    = s[k] + z c+[k-1]                         k = 1 .. n-1
 *              c-[n-1]  = pole_gain (c+[n-1] + z c+[n-2])
 *              c-[k]    = z (c-[k+1] - c+[k])                      k = n-2 .. 0
 *   evaluation  out[jx, jy, jz] = (float)( sum_kz wz[jz][kz] ( sum_ky wy[jy][ky] ( sum_kx wx[jx][kx]
 *            coef[ix[jx][kx], iy[jy][ky], iz[jz][kz]] ) ) ), each sum over k = 0..3 ascending from +0.0, product then sum; computed as
 *            three passes x, y, z over fp64 intermediates in ws (the inner sums depend on (jx, y, z) and (jx, jy, z) alone: the same
 *            bits as the nested form).  Where any axis is outside, out is 0.0f (ITK's default pixel value).
 *   mask     out_mask is 1 where all three axes are inside and the mask voxel at the three nearest indices, raw * mask_slope +
 *            mask_inter, is not 0 (a NaN counts as not 0: the ROI rule of mmnn_radiomics); otherwise 0.
 * A non-finite scan voxel propagates through the recursion: it reaches the whole of its x line, then every y line that crosses that,
 * then every z line -- in practice the whole volume.  One lane per output, no atomics: repeated calls are bit-identical, and so is a
 * restatement that follows the order above.  No host wait.  ws: mmnn_resample_pair_workspace_bytes bytes, aligned to 256: the
 * coefficients and the two intermediates, 8 (x y z + mx y z + mx my z) bytes.  Refused (status 1, nothing written; the size returns -1)
 * before any launch: a null pointer, a non-positive extent on either grid, 2^31 elements or more on either grid or in an intermediate,
 * an unsupported type code, a non-finite prefilter constant, a scan or mask not aligned to its element size, tables not to 8, out not to
 * 4, ws not to 256, a table index outside its source axis, a non-finite weight. */
#define MMNN_RESAMPLE_HORIZON 40
typedef struct {
  double w[4];
  int32_t i[4];
  int32_t nearest;
  int32_t inside;
} mmnn_resample_entry;
typedef struct {
  int32_t x, y, z;                /* the source grid */
  int32_t mx, my, mz;             /* the output grid */
  int32_t scan_type, mask_type;   /* NIfTI datatype codes */
  double scan_slope, scan_inter, mask_slope, mask_inter;
  double pole, pole_gain, gain;
  double pole_power[MMNN_RESAMPLE_HORIZON];
} mmnn_resample_desc;
int64_t mmnn_resample_pair_workspace_bytes(int32_t x, int32_t y, int32_t z, int32_t mx, int32_t my, int32_t mz);
int mmnn_resample_pair(const mmnn_resample_desc* d, const void* scan, const void* mask, const mmnn_resample_entry* tables_host,
                       const mmnn_resample_entry* tables, float* out, uint8_t* out_mask, void* ws, void* stream);

/* ---- the margin step behind the mask routes: widen a mask by a radius in mm on the scan's grid (csrc/mask_margin.hip).  An exact,
 * bounded Euclidean distance to the mask under the scan's voxel spacing, thresholded at the radius.  `mask` holds x*y*z elements, x
 * fastest, in NIfTI type mask_type.
 *   set voxels   a mask voxel q is set when !(m == 0), m the scaled mask value formed as the ingest forms it: raw * mask_slope +
 *            mask_inter in fp64, two roundings.  A NaN counts as set.  A slope of 0, NaN or +-inf means no scaling.
 *   per-axis term  t_a(k) = fl(fl(k s_a) fl(k s_a)) for an index distance k >= 0 along axis a with spacing s_a = spacing[a]: fp64, every
 *            operation rounded on its own, never an FMA.
 *   distance  D(p) = min over set q of fl(fl(t_x(|p_x - q_x|) + t_y(|p_y - q_y|)) + t_z(|p_z - q_z|)); +inf for an empty mask.
 *   radius   R2 = fl(radius radius).
 *   modes    MMNN_MARGIN_DILATE writes out = 1 where D <= R2, else 0.  MMNN_MARGIN_SHELL writes out = 1 where 0 < D <= R2, else 0: the
 *            dilated set without the mask itself.
 *   outputs  `out` is one byte per scan voxel, x fastest; every byte is written and nothing else is.  It is a type-2 mask with slope 1
 *            and inter 0 for mmnn_ingest_volume and mmnn_radiomics.  An optional `dist2` (fp64, may be null) receives D where D <= R2
 *            and +inf elsewhere.
 *   reach    reach_a is the largest k with t_a(k) <= R2; the library computes it on the host from `spacing` and `radius`.  No q farther
 *            than that along an axis can matter, so the search is bounded.  mmnn_mask_margin_reach is that computation as a host query
 *            that needs no GPU (status 1 for a null pointer, a spacing or radius that is not finite and > 0, a reach above the cap).
 * The index axes are taken as orthogonal.  Computed as three passes x, y, z (a rounded addition is monotone, so the minimum commutes with
 * adding the next axis' term: the same bits as the brute-force minimum above); every loop bound comes from the descriptor, no walk
 * depends on the data.  Everything is enqueued on the caller's stream; one lane per output, no atomics, no host synchronisation:
 * repeated calls are bit-identical.  ws: mmnn_mask_margin_workspace_bytes bytes (no GPU needed), aligned to 256: one byte and one fp64
 * per voxel.  Refused (status 1, nothing written; the size returns -1) before any launch: a null descriptor, mask, out or workspace; a
 * non-positive extent, or x*y*z >= 2^31; an unknown type code; a spacing or radius that is not finite and > 0; a mode outside the two; a
 * reach above MMNN_MARGIN_MAX_REACH; `mask` overlapping `out`; a mask not aligned to its element size, dist2 not to 8, ws not to 256.
 * The cap: 30 mm at 0.4 mm in-plane is 75 voxels; at 128 the y / z tile with its two halos takes 52.1 KiB of the 64 KiB of LDS a launch
 * gets, and an index distance still fits the byte the x pass stores. */
#define MMNN_MARGIN_MAX_REACH 128
#define MMNN_MARGIN_DILATE 0
#define MMNN_MARGIN_SHELL 1
typedef struct {
  int32_t x, y, z;
  int32_t mask_type;              /* NIfTI datatype code */
  double mask_slope, mask_inter;
  double spacing[3];              /* x, y, z, in mm */
  double radius;                  /* in mm */
  int32_t mode;                   /* MMNN_MARGIN_DILATE, MMNN_MARGIN_SHELL */
} mmnn_mask_margin_desc;
int mmnn_mask_margin_reach(const double spacing[3], double radius, int32_t reach[3]);
int64_t mmnn_mask_margin_workspace_bytes(int32_t x, int32_t y, int32_t z);
int mmnn_mask_margin(const mmnn_mask_margin_desc* d, const void* mask, uint8_t* out, double* dist2, void* ws, void* stream);

/* ---- measurement aid (bench.py): MHz the chip sustains under a chip-wide v_mfma_f32_32x32x2_f32 load (one wave per SIMD, every CU), from
 * the known cycle count of an MFMA loop and HIP events around it.  Synchronises the stream.  scratch: >= 1 float of device memory. */
int mmnn_measure_mfma_clock(double* mhz, float* scratch, void* stream);

#ifdef __cplusplus
}
#endif
#endif
