/* rvlm.h - C ABI of librvlm.so, the MI355X (gfx950) adversarial inner loop for RobustVLM.
 *
 * Drop-in boundary.  Everything the reference's Python hot path does on
 * the device goes through these entry points; the Python shim in robustvlm_amd/ binds them with
 * ctypes (INTEGRATION.md shows the stub a reference maintainer would add).
 *
 * Conventions
 *   - extern "C", plain pointers and sizes, no torch / C++ types.
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in _host.
 *   - every function takes the hipStream_t to enqueue on (as void*), never synchronises the device
 *     (except *_create / *_destroy / *_get_profile), starts no threads and allocates nothing after
 *     rvlm_vit_create.
 *   - return value: 0 = RVLM_OK, otherwise an rvlm_status; rvlm_last_error() gives the message of
 *     the last failure on the calling thread.  No exceptions cross the ABI.
 *   - images are NCHW fp32 in [0,1] (un-normalised: the CLIP mean/std Normalize lives inside the
 *     encoder, train/adversarial_training_clip.py:105-108,254), targets are int64.
 */
#ifndef RVLM_H
#define RVLM_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RVLM_VERSION 109
/* Additions made without a version step are announced by a feature macro (a binding can also probe the symbol):
 * RVLM_HAS_TEXT: the rvlm_text_* entry points and RVLM_FLAG_TOKEN_RANGE / RVLM_FLAG_EOT_ACTIVE */
#define RVLM_HAS_TEXT 1
/* RVLM_HAS_FAB: the rvlm_fab_* entry points (FAB / FAB-T, L-inf), RVLM_LOSS_LOGIT_DIFF and RVLM_FLAG_FAB_NONFINITE */
#define RVLM_HAS_FAB 1
/* RVLM_HAS_INPUT_RESIZE: rvlm_vit_set_input_size (bicubic up-sampling as part of the model), rvlm_resize_bicubic(_adjoint),
 * rvlm_resize_taps */
#define RVLM_HAS_INPUT_RESIZE 1
/* RVLM_HAS_TOKENS: token-level outputs of the encoder and their input gradient - rvlm_vit_forward_tokens,
 * rvlm_vit_backward_input_tokens, rvlm_tokens_l2_loss_grad, rvlm_vit_tokens_fwd_inputgrad, rvlm_pgd_run_tokens,
 * RVLM_TOKENS_ALL / RVLM_TOKENS_PATCH and RVLM_FLAG_TOKENS_NONFINITE */
#define RVLM_HAS_TOKENS 1
/* RVLM_HAS_VLM_ATTACKS: the per-iteration kernels of vlm_eval/attacks/pgd.py / apgd.py on a [B, n_img, P] tensor with a per-image
 * mask - rvlm_mask_grad, rvlm_pgd_masked_update, rvlm_apgd_masked_step, rvlm_apgd_masked_bookkeeping */
#define RVLM_HAS_VLM_ATTACKS 1
/* RVLM_HAS_SQUARE_L2: rvlm_square_l2_propose (one query of the L2 Square Attack) and RVLM_FLAG_SQUARE_NONFINITE */
#define RVLM_HAS_SQUARE_L2 1
/* RVLM_HAS_SGD: rvlm_sgd_step (torch.optim.SGD with momentum, the trainer's --opt sgd) */
#define RVLM_HAS_SGD 1
/* RVLM_HAS_TOKEN_TRAINING: weight gradients through the token door - rvlm_vit_forward_tokens(save = 2),
 * rvlm_vit_backward_params_tokens(_stages), rvlm_tokens_cosine */
#define RVLM_HAS_TOKEN_TRAINING 1
/* RVLM_HAS_TOKEN_APGD: rvlm_apgd_run_tokens - vlm_eval/attacks/apgd.py's loop on the per-image token loss, batched, device resident */
#define RVLM_HAS_TOKEN_APGD 1

typedef void* rvlm_stream_t; /* hipStream_t */
typedef struct rvlm_vit rvlm_vit;

typedef enum {
    RVLM_OK = 0,
    RVLM_ERR_ARG = 1,         /* bad argument (null pointer, shape out of range, unknown enum) */
    RVLM_ERR_HIP = 2,         /* a HIP runtime call failed */
    RVLM_ERR_STATE = 3,       /* call order violated (e.g. backward without a saved forward) */
    RVLM_ERR_UNSUPPORTED = 4  /* configuration the kernels do not cover */
} rvlm_status;

/* GEMM / attention operand precision.  RVLM_PREC_F32X3 (ABI 108): fp32 storage and fp32 LayerNorm / softmax / attention products
 * like RVLM_PREC_F32, the encoder's linears as split-bf16 products (a_hi w_hi + a_hi w_lo + a_lo w_hi, fp32 accumulate) on the
 * bf16 matrix pipe: ~16 mantissa bits at 3 bf16 MFMAs per product (robustvlm_amd/csrc/x3_kernels.hip); attack / inference only */
enum { RVLM_PREC_F32 = 0, RVLM_PREC_BF16 = 1, RVLM_PREC_F32X3 = 2 };
enum { RVLM_ACT_QUICK_GELU = 0, RVLM_ACT_GELU = 1 };  /* open_clip QuickGELU / exact erf GELU */
enum { RVLM_LOSS_L2 = 0, RVLM_LOSS_CE = 1,             /* FARE l2 / TeCoA ce (…clip.py:495-528) */
       RVLM_LOSS_DLR = 2, RVLM_LOSS_DLR_TARGETED = 3,   /* AutoAttack DLR losses (autopgd_base.py:195-201, 613-618) */
       RVLM_LOSS_LOGIT_DIFF = 4 };                      /* FAB-T's logit difference (fab_pt.py:100-114), RVLM_HAS_FAB */
enum { RVLM_RED_MEAN = 0, RVLM_RED_NONE = 1 };        /* reduction='mean' | 'none' (grad of sum) */

/* bits of the device-side flag word written by the attack kernels (replaces the reference's
 * per-iteration host asserts, train/pgd_train.py:24,40,60-63) */
enum {
    RVLM_FLAG_INPUT_RANGE = 1, /* data_clean outside [0,1] (+-1e-6)          pgd_train.py:24    */
    RVLM_FLAG_NAN_GRAD = 2,    /* NaN in the gradient (zeroed, not an error) pgd_train.py:40-42 */
    RVLM_FLAG_NAN_DELTA = 4,   /* NaN in the perturbation                    pgd_train.py:60    */
    RVLM_FLAG_ADV_RANGE = 8,   /* x+delta left [0,1] (+-1e-6)                pgd_train.py:61-63 */
    /* rvlm_text_encode (RVLM_HAS_TEXT); where the reference would fault inside nn.Embedding or pool the wrong row */
    RVLM_FLAG_TOKEN_RANGE = 16, /* a token id outside [0, vocab)                                  */
    RVLM_FLAG_EOT_ACTIVE = 32,  /* a prompt's EOT position (argmax of its ids) is >= active_len   */
    /* rvlm_fab_projection_linf / rvlm_fab_linf_step (RVLM_HAS_FAB) */
    RVLM_FLAG_FAB_NONFINITE = 64, /* NaN / Inf in a row's w, t or b: that row gets lambda = 0 (no move) */
    /* rvlm_tokens_l2_loss_grad and the loops built on it (RVLM_HAS_TOKENS) */
    RVLM_FLAG_TOKENS_NONFINITE = 128, /* NaN / Inf in an image's token loss (its tokens or their reference) */
    /* rvlm_square_l2_propose (RVLM_HAS_SQUARE_L2) */
    RVLM_FLAG_SQUARE_NONFINITE = 256 /* NaN / Inf in a candidate (square.py:416-417): that row of x_new = x_best */
};

/* ---------------------------------------------------------------------------------------------
 * Encoder: open_clip VisionTransformer forward + input-gradient.
 * Replaces `ClipVisionModel.forward` (train/adversarial_training_clip.py:253-257) and the autograd
 * backward `torch.autograd.grad(loss, perturbation)` (train/pgd_train.py:38, apgd_train.py:185,295).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t image_size; /* 224 */
    int32_t patch;      /* 14 (ViT-L/14), 32 (ViT-B/32) */
    int32_t width;      /* 1024 / 768; heads * 64 */
    int32_t layers;     /* 24 / 12 */
    int32_t heads;      /* 16 / 12 (head_dim must be 64) */
    int32_t out_dim;    /* 768 / 512 */
    int32_t act;        /* RVLM_ACT_* */
    int32_t precision;  /* RVLM_PREC_* */
    int32_t max_batch;  /* workspace is sized for this many images */
    float mean[3];      /* Normalize constants, …clip.py:116 */
    float std[3];
    int32_t trainable;  /* > 0: also keep what the weight-gradient backward needs (rvlm_vit_backward_params);
                           -1: inference only (frozen model_orig copy): no per-layer activation storage;
                           -2 (ABI 109, fp32-storage precisions): forward PROVIDER of a bf16 handle - its saving forwards are all
                           rvlm_vit_forward_for / rvlm_pgd_run_mixed_fwd: per-block residual stream and statistics only, no
                           backward scratch, no probabilities (51 -> 13 GiB at ViT-L/14, B = 128); on a bf16 handle -2 means -1 */
} rvlm_vit_config;

/* fp32 device pointers in `visual.state_dict()` layout (…clip.py:239,470; Appendix B key list). */
typedef struct {
    const float* ln_1_weight;          /* [W]      */
    const float* ln_1_bias;            /* [W]      */
    const float* attn_in_proj_weight;  /* [3W, W]  */
    const float* attn_in_proj_bias;    /* [3W]     */
    const float* attn_out_proj_weight; /* [W, W]   */
    const float* attn_out_proj_bias;   /* [W]      */
    const float* ln_2_weight;          /* [W]      */
    const float* ln_2_bias;            /* [W]      */
    const float* mlp_c_fc_weight;      /* [4W, W]  */
    const float* mlp_c_fc_bias;        /* [4W]     */
    const float* mlp_c_proj_weight;    /* [W, 4W]  */
    const float* mlp_c_proj_bias;      /* [W]      */
} rvlm_vit_block_weights;

typedef struct {
    const float* class_embedding;      /* [W]            */
    const float* positional_embedding; /* [tokens, W]    */
    const float* proj;                 /* [W, out_dim]   */
    const float* conv1_weight;         /* [W, 3, P, P]   */
    const float* ln_pre_weight;        /* [W] */
    const float* ln_pre_bias;
    const float* ln_post_weight;
    const float* ln_post_bias;
    const rvlm_vit_block_weights* blocks_host; /* HOST array of `layers` structs of device ptrs */
} rvlm_vit_weights;

/* Allocates the workspace, converts/transposes the weights into the engine's layout. */
int rvlm_vit_create(const rvlm_vit_config* cfg, const rvlm_vit_weights* weights,
                    rvlm_stream_t stream, rvlm_vit** out);
int rvlm_vit_destroy(rvlm_vit* h);
/* Re-import weights (after an optimizer step of the outer trainer). */
int rvlm_vit_load_weights(rvlm_vit* h, const rvlm_vit_weights* weights, rvlm_stream_t stream);
/* Bytes of device memory the handle owns. */
size_t rvlm_vit_workspace_bytes(const rvlm_vit* h);

/* emb[B,out_dim] = visual(Normalize(x + delta)) (delta may be NULL), L2-normalised iff
 * output_normalize.  save_for_backward: 0 = inference, 1 = keep what rvlm_vit_backward_input needs,
 * 2 = additionally keep the linear-layer inputs for rvlm_vit_backward_params (trainable handles). */
int rvlm_vit_forward(rvlm_vit* h, const float* x, const float* delta, int B, int output_normalize,
                     int save_for_backward, float* out_emb, rvlm_stream_t stream);
/* grad_x[B,3,H,W] = d<d_emb, emb>/d(x+delta) for the last saved forward (dgrad only, no wgrad). */
int rvlm_vit_backward_input(rvlm_vit* h, const float* d_emb, int B, float* grad_x,
                            rvlm_stream_t stream);
/* The same for the forward saved on ANOTHER handle of the same model and max_batch (ABI 109): h_saved holds fp32 storage
 * (RVLM_PREC_F32 / RVLM_PREC_F32X3), h is a bf16 handle whose backward kernels evaluate the gradient - qkv, attention output and
 * act'(fc1) are exported to bf16, the fp32 residual stream / LayerNorm statistics are read in place.  For the first FARE iteration
 * (torch.autograd.grad(loss, perturbation), train/pgd_train.py:38): the forward difference needs the precision, the backward does
 * not.  Invalidates h's own saved forward. */
int rvlm_vit_backward_input_from(rvlm_vit* h, rvlm_vit* h_saved, const float* d_emb, int B, float* grad_x,
                                 rvlm_stream_t stream);
/* A saving forward on the fp32-storage handle h FOR `consumer`'s backward (ABI 109): like rvlm_vit_forward(save_for_backward = 1), but
 * the attention runs as the fp32 flash kernel (no probabilities kept - rvlm_vit_backward_input on h is refused for this pass) and the
 * bf16 tensors rvlm_vit_backward_input_from(consumer, h, ...) reads are written by the forward itself instead of by export passes. */
int rvlm_vit_forward_for(rvlm_vit* h, rvlm_vit* consumer, const float* x, const float* delta, int B, int output_normalize,
                         float* out_emb, rvlm_stream_t stream);
/* Non-saving forwards of an fp32-storage handle on the fp32 flash attention as well (default off: a handle's saving and non-saving
 * forwards agree bit for bit, which FARE's zero gradient at delta = 0 relies on; switch it on for the handle whose saving forwards
 * are all rvlm_vit_forward_for, so that its clean embedding and its first-iteration embedding share one arithmetic).  ABI 109. */
int rvlm_vit_set_flash_inference(rvlm_vit* h, int on);

/* ---------------------------------------------------------------------------------------------
 * Bicubic resize inside the model (RVLM_HAS_INPUT_RESIZE): ClassificationModel(..., resizer=Resize(224, BICUBIC,
 * antialias=False)) of CLIP_eval/clip_robustbench.py:60-68,104-114 - the attack's images, perturbation and eps ball live at the
 * dataset's own resolution and the input gradient comes back through the resize.
 * The operator is torch.nn.functional.interpolate(x, (out_h, out_w), mode='bicubic', align_corners=False, antialias=False) on
 * float tensors: Y = R_h X R_w^T with, per output index o, src = (in / out) (o + 0.5) - 0.5, i = floor(src), t = src - i, four taps
 * i-1 .. i+2 (index clamped to [0, in-1]), cubic-convolution weights with A = -0.75 (computed in double, rounded to fp32).  The result
 * is not clamped.
 * ------------------------------------------------------------------------------------------- */
/* Handle state.  (image_size, image_size) or (0, 0): the model's own resolution, the default.  Otherwise every entry that takes or
 * returns images (rvlm_vit_forward, rvlm_vit_backward_input, rvlm_vit_fwd_inputgrad, rvlm_pgd_run*, rvlm_apgd_run*) reads / writes
 * [B, 3, in_h, in_w]: x (+ delta) is resized to (image_size, image_size) inside the patch embedding, grad_x is the adjoint's.
 * 1 <= in_h, in_w <= image_size (up-sampling); larger, or a trainable handle: RVLM_ERR_UNSUPPORTED.  Changing the size invalidates a
 * saved forward (a backward then returns RVLM_ERR_STATE).  The two-handle entries (rvlm_pgd_run_mixed*, rvlm_vit_forward_for,
 * rvlm_vit_backward_input_from) need the same size on both handles, else RVLM_ERR_STATE.  First use of a size on a device builds
 * its tap tables (a synchronous copy of a few KB). */
int rvlm_vit_set_input_size(rvlm_vit* h, int in_h, int in_w);
/* Standalone: y [planes, out_h, out_w] <- x [planes, in_h, in_w] and the adjoint gx [planes, in_h, in_w] <- gy [planes, out_h, out_w]
 * (gx = R_h^T gy R_w), any pair of sizes in 1..32768.  The adjoint is a gather in a fixed order: no atomics, bit-reproducible. */
int rvlm_resize_bicubic(const float* x, long planes, int in_h, int in_w, int out_h, int out_w, float* y, rvlm_stream_t stream);
int rvlm_resize_bicubic_adjoint(const float* gy, long planes, int in_h, int in_w, int out_h, int out_w, float* gx,
                                rvlm_stream_t stream);
/* HOST: the tap table of one axis, idx [out, 4] (clamped) and w [out, 4]; needs no device. */
int rvlm_resize_taps(int in, int out, int32_t* idx, float* w);

/* Weight gradients of the outer training step (loss_total.backward(), …clip.py:361): for the last
 * forward run with save_for_backward == 2 on a `trainable` handle, writes (accumulate == 0) or adds
 * (accumulate != 0) d<d_emb, emb>/d(param) for EVERY parameter into the fp32 tensors `grads` points to
 * (same struct / shapes as the weights).  No input gradient is produced. */
int rvlm_vit_backward_params(rvlm_vit* h, const float* d_emb, int B, const rvlm_vit_weights* grads,
                             int accumulate, rvlm_stream_t stream);
/* The same pass cut into stages (execution order): 0 = head (proj, ln_post), 1 + j = transformer block layers-1-j,
 * layers + 1 = embeddings (ln_pre, positional / class embedding, conv1).  Runs stages [stage_begin, stage_end); the
 * stages of one backward must be run in order.  The host uses it to all-reduce a finished gradient bucket (RCCL,
 * side stream) while the remaining stages compute - the reference's DataParallel reduces inside backward as well
 * (…clip.py:184-191). */
int rvlm_vit_backward_params_stages(rvlm_vit* h, const float* d_emb, int B, const rvlm_vit_weights* grads,
                                    int accumulate, int stage_begin, int stage_end, rvlm_stream_t stream);
/* torch.optim.AdamW single-tensor step on flat fp32 buffers (optimizer.step(), …clip.py:196-197,362):
 * grads are multiplied by grad_scale first (1/world_size after a sum all-reduce). `step` counts from 1.  The
 * hyper-parameters are doubles (Python floats in torch): bias corrections and step size are formed in double and
 * rounded to fp32 where torch rounds them. */
int rvlm_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, size_t n,
                    double lr, double beta1, double beta2, double eps, double weight_decay, int step,
                    float grad_scale, rvlm_stream_t stream);
/* torch.optim.SGD single-tensor step (dampening 0, no Nesterov; --opt sgd, …clip.py:198-206) on flat fp32 buffers
 * (RVLM_HAS_SGD).  Per element, in fp32, the double hyper-parameters rounded to fp32 first:
 *     g = grads[i] * grad_scale;  d = g + weight_decay * p        (coupled weight decay, unlike AdamW's)
 *     buf = first ? d : momentum * buf + d;  p = p - lr * buf     (momentum == 0: no buffer, p -= lr * d)
 * `first` != 0 on the first step of a run (torch clones d into the buffer: it is written, not read).  momentum_buf may
 * be NULL only when momentum == 0 and is then neither read nor written.  NULL params / grads, momentum < 0 and a NULL
 * buffer with momentum > 0 are RVLM_ERR_ARG (nothing is launched); n == 0 is RVLM_OK without a launch.  Elements move in
 * 16-byte accesses when all live pointers are 16-byte aligned, one float at a time otherwise, with identical results. */
int rvlm_sgd_step(float* params, const float* grads, float* momentum_buf, size_t n, double lr, double momentum,
                  double weight_decay, int first, float grad_scale, rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Losses (replace compute_loss / l2 / ce, …clip.py:495-528) - loss value and d loss / d emb.
 *   L2:  ref = embedding_orig [B,D];  per_sample = sum_d (emb-ref)^2
 *   CE:  ref = text head T [D,C] (column-normalised); logits = emb @ (logit_scale*T)
 * reduction MEAN: *loss_scalar = mean_b, d_emb carries the 1/B; NONE: d_emb = grad of the sum.
 *   DLR / DLR_TARGETED (APGD-DLR, APGD-T): same logits; per_sample =
 *        -(z_y - max_{c != y} z_c) / (z_(1) - z_(3) + 1e-12)            resp.
 *        -(z_y - z_t) / (z_(1) - (z_(3) + z_(4)) / 2 + 1e-12),  t = y_target[b],  z_(k) = k-th largest logit
 * reduction MEAN: *loss_scalar = mean_b, d_emb carries the 1/B; NONE: d_emb = grad of the sum.
 *   LOGIT_DIFF (FAB-T, fab_pt.py:100-114; RVLM_HAS_FAB): same logits; per_sample = -(z_y - z_t), t = y_target[b];
 *        d_emb = logit_scale * (T[:, t] - T[:, y]): with reduction NONE one call gives FAB's df (per_sample) and, through
 *        rvlm_vit_fwd_inputgrad, dg (grad_x) without an autograd graph.
 * pred_eq (optional, u8[B]) = argmax_c(logits) == targets (head losses only).  scratch: the head losses need
 * B*C + D*C floats (may be NULL for L2).  y_target: DLR_TARGETED and LOGIT_DIFF (else NULL).
 * Caller's duty: every targets[b] and y_target[b] lies in [0, C).  The labels live on the device, so this call cannot
 * check them without a sync; a label outside the range makes the kernel read logits[b][label] outside the row.
 * (The Python callers check before they launch and raise IndexError, as F.cross_entropy does.)
 * ------------------------------------------------------------------------------------------- */
int rvlm_loss_grad(int loss_kind, int reduction, const float* emb, const float* ref,
                   const int64_t* targets, const int64_t* y_target, int B, int D, int C, float logit_scale,
                   float* loss_per_sample, float* loss_scalar, float* d_emb, uint8_t* pred_eq,
                   float* scratch, rvlm_stream_t stream);
/* ce() on given logits (…clip.py:523-528 = F.cross_entropy): per-sample loss, optional scalar (mean or sum per
 * `reduction`), d_logits [B,C] = d loss / d logits (MEAN carries the 1/B; may alias logits), optional pred_eq. */
int rvlm_ce_logits(const float* logits, const int64_t* targets, int B, int C, int reduction,
                   float* loss_per_sample, float* loss_scalar, float* d_logits, uint8_t* pred_eq,
                   rvlm_stream_t stream);
/* Zero-shot head of ClassificationModel.forward (CLIP_eval/clip_robustbench.py:66-68): logits[B,C] = (emb[B,D] @
 * T[D,C]) * scale, and its backward d_emb = (d_logits * scale) @ T^T. */
int rvlm_head_logits(const float* emb, const float* T, int B, int D, int C, float scale, float* logits,
                     rvlm_stream_t stream);
int rvlm_head_logits_bwd(const float* d_logits, const float* T, int B, int D, int C, float scale, float* d_emb,
                         rvlm_stream_t stream);
/* Logging metrics of the training step (…clip.py:368-387): out_per_row[b] = F.cosine_similarity(a[b], b[b]) (eps 1e-8),
 * optional *out_mean = their mean; F.normalize(e, dim=1) (eps 1e-12) with the reciprocal norms. */
int rvlm_cosine_rows(const float* a, const float* b, int B, int D, float* out_per_row, float* out_mean,
                     rvlm_stream_t stream);
int rvlm_l2_normalize_rows(const float* e, int B, int D, float* out, float* inv_norm, rvlm_stream_t stream);
/* out[b] = (argmax_j logits[b,j] == targets[b]); ties -> first index (…clip.py:490,
 * apgd_train.py:192,301). */
int rvlm_argmax_eq(const float* logits, const int64_t* targets, int B, int C, uint8_t* out,
                   rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * L-inf attack arithmetic (bit-exact with the reference).
 * ------------------------------------------------------------------------------------------- */
/* flags |= RVLM_FLAG_INPUT_RANGE if any x outside (-1e-6, 1+1e-6)   (pgd_train.py:24) */
int rvlm_check_image_range(const float* x, size_t n, int32_t* flags, rvlm_stream_t stream);
/* The standalone helpers of vlm_eval/attacks/utils.py as they are (robustvlm_amd/attack_utils.py):
 *   project_perturbation (:8-16): norm_kind 0 -> clamp(pert, -eps, eps); 2 -> torch.renorm(pert, p=2, dim=0, maxnorm=eps)
 *   normalize_grad (:19-26):      norm_kind 0 -> sign(grad);             2 -> F.normalize(grad.view(B, -1), p=2, dim=1)
 * over B samples of n_per_sample elements; out may alias the input. */
int rvlm_project_perturbation(const float* pert, size_t n_per_sample, int B, int norm_kind, float eps, float* out,
                              rvlm_stream_t stream);
int rvlm_normalize_grad(const float* grad, size_t n_per_sample, int B, int norm_kind, float* out, rvlm_stream_t stream);
/* One PGD step (pgd_train.py:38-63 + vlm_eval/attacks/utils.py:10,21), in place on delta/velocity:
 *   g=NaN->0; v=sign(mom*v+sign(g)); delta=clamp(delta +/- step*v, +-eps);
 *   delta=clamp(x+delta,0,1)-x.   x_adv_out (optional) = x + delta.
 * It is rvlm_pgd_masked_update without a mask (one row of n elements, image_space = 1): the same kernel.  A NaN in delta, x
 * or stepsize (or one that Inf - Inf makes of them) propagates as torch.clamp passes it on and raises RVLM_FLAG_NAN_DELTA
 * (pgd_train.py:60). */
int rvlm_pgd_linf_update(const float* x, const float* grad, float* delta, float* velocity,
                         size_t n, float eps, float stepsize, float momentum, int mode_max,
                         float* x_adv_out, int32_t* flags, rvlm_stream_t stream);
/* The L2 branch of the same block (norm in [2, 'l2', ...]; vlm_eval/attacks/utils.py:12-14,22-26), per sample b over
 * its n_per_sample pixels:  g = NaN->0; g /= max(|g|_2, 1e-12); v = mom*v + g; v /= max(|v|_2, 1e-12);
 * delta +/-= step*v; delta *= eps/(|delta|_2 + 1e-7) where |delta|_2 > eps (torch.renorm); delta = clamp(x+delta,0,1)-x.
 * The norms are deterministic fp32 sums in an order of their own: equal to the reference to fp32 rounding.
 * The kernel of rvlm_pgd_masked_update (L2) without a mask, in its scalar walk; NaN in delta / x propagates and raises
 * RVLM_FLAG_NAN_DELTA as in rvlm_pgd_linf_update. */
int rvlm_pgd_l2_update(const float* x, const float* grad, float* delta, float* velocity, size_t n_per_sample, int B,
                       float eps, float stepsize, float momentum, int mode_max, float* x_adv_out, int32_t* flags,
                       rvlm_stream_t stream);
/* One APGD step (apgd_train.py:205-229 == autopgd_base.py:328-341); step is per-sample [B].  The kernel of rvlm_apgd_masked_step
 * (L-inf) without a mask or a flag word: a NaN in x_adv, x_adv_old or step propagates as in torch.min / torch.max /
 * torch.clamp.  16-byte accesses when n_per_sample % 4 == 0 and the pointers are 16-byte aligned; n_per_sample > 0. */
int rvlm_apgd_linf_step(const float* x, float* x_adv, float* x_adv_old, const float* grad,
                        const float* step, float a, float eps, size_t n_per_sample, int B,
                        rvlm_stream_t stream);
/* The L2 branch of the same step (apgd_train.py:231-254): gradient step of length `step` along grad / |grad|_2, projection
 * onto the eps ball (L2) around x and the image range, momentum mix (a, 1 - a), projection again; per-sample norms are
 * deterministic fp32 sums in an order of their own (equal to the reference to fp32 rounding).  The kernel of rvlm_apgd_masked_step
 * (L2) without a mask, in its scalar walk: NaN propagates through the clamps as in torch. */
int rvlm_apgd_l2_step(const float* x, float* x_adv, float* x_adv_old, const float* grad, const float* step, float a,
                      float eps, size_t n_per_sample, int B, rvlm_stream_t stream);
/* Per-sample APGD bookkeeping for iteration i (apgd_train.py:301-305,320-355): k and do_check
 * follow the data-independent checkpoint schedule kept by the host. */
int rvlm_apgd_controller(int i, int B, int n_iter, int k, int do_check, const float* loss_i,
                         const uint8_t* pred, float* loss_steps, float* loss_best,
                         float* loss_best_last_check, float* reduced_last_check, float* step,
                         uint8_t* acc, uint8_t* f_notpred, uint8_t* f_improved,
                         uint8_t* f_reduced, rvlm_stream_t stream);
/* The same with the oscillation threshold as a parameter: `rho` of APGDAttack (autoattack/autopgd_base.py:111,137;
 * check_oscillation's k3, :170-175,415-416); rvlm_apgd_controller is rho = 0.75, the value apgd_train hard-codes
 * (train/apgd_train.py:117,334). */
int rvlm_apgd_controller_rho(int i, int B, int n_iter, int k, int do_check, double rho, const float* loss_i,
                             const uint8_t* pred, float* loss_steps, float* loss_best,
                             float* loss_best_last_check, float* reduced_last_check, float* step,
                             uint8_t* acc, uint8_t* f_notpred, uint8_t* f_improved,
                             uint8_t* f_reduced, rvlm_stream_t stream);
/* The index assignments of the same lines as one pass over the image tensors. */
int rvlm_apgd_select(float* x_adv, float* grad, float* x_best, float* grad_best,
                     float* x_best_adv, const uint8_t* f_notpred, const uint8_t* f_improved,
                     const uint8_t* f_reduced, size_t n_per_sample, int B, rvlm_stream_t stream);
/* APGDAttack random start (autopgd_base.py:210-214,180-183): x + eps * t / (max_b|t| + 1e-12). */
int rvlm_linf_random_start(const float* x, const float* t, float eps, size_t n_per_sample, int B,
                           float* x_adv, rvlm_stream_t stream);
/* Its L2 form (autopgd_base.py:184-185,215-218): x + eps * t / (|t|_2 + 1e-12), t ~ N(0, 1) drawn by the caller (the reference
 * draws it on the CPU generator); the norm is a deterministic fp32 sum in the kernel's own order. */
int rvlm_l2_random_start(const float* x, const float* t, float eps, size_t n_per_sample, int B, float* x_adv,
                         rvlm_stream_t stream);
/* Square Attack, L-inf: one query of SquareAttack.attack_single_run (autoattack/square.py:256-263).  Candidates of the
 * n_active still-robust images idx[a] (int64 indices into x / x_best [*, C, H, W]), written compactly to x_new
 * [n_active, C, H, W]:  clamp(min(max(x_best + window, x - eps), x + eps), 0, 1), window = 2*eps*sign[c] on rows
 * [vh, vh+s) x columns [vw, vw+s) and 0 elsewhere (one window per query for the whole batch).  sign: C floats. */
int rvlm_square_linf_propose(const float* x, const float* x_best, const int64_t* idx, int n_active, int C, int H,
                             int W, int vh, int vw, int s, float eps, const float* sign, float* x_new,
                             rvlm_stream_t stream);
/* square.py:288-291: x_best[idx[a]] = x_new[a] for the candidates with take[a] != 0 (loss improved or misclassified). */
int rvlm_square_accept(float* x_best, const float* x_new, const int64_t* idx, const float* take, int n_active,
                       size_t n_per_image, rvlm_stream_t stream);
/* Square Attack, L2 (RVLM_HAS_SQUARE_L2): one query of the L2 branch of SquareAttack.attack_single_run (autoattack/square.py:339-379)
 * in one launch, for the n_active still-robust images idx[a], written compactly to x_new [n_active, C, H, W] as above.  With
 * delta = x_best - x, window 1 = rows [vh, vh+s) x columns [vw, vw+s) and window 2 the same at (vh2, vw2), per image and channel c:
 *   new = eta * sign[a, c] + delta[win1] / (1e-12 + |delta[win1]|_c)
 *   new = new / (1e-12 + |new|_c) * sqrt(max(eps^2 - |delta|^2, 0) / C + |delta[win1 u win2]|_c^2)
 *   delta[win2] = 0, then delta[win1] = new;   x_new = clamp(x + eps * delta / (|delta| + 1e-12), 0, 1)
 * eta: [s, s] floats (the reference's eta(s), already transposed if its coin said so); sign: [n_active, C] floats.  delta and the
 * windows are never stored.  Every norm is a deterministic fp32 sum in the kernel's own fixed order (no atomics): the same bits on
 * every run, not the bits of torch's sum.  flags (optional device word) |= RVLM_FLAG_SQUARE_NONFINITE for an image whose sums hold
 * NaN / Inf (the reference's asserts, :416-417); its row of x_new is x_best.  Both windows must lie inside the image, eps finite and
 * > 0 (RVLM_ERR_ARG); C <= 16 (RVLM_ERR_UNSUPPORTED).  16-byte accesses when W % 4 == 0 and the pointers are 16-byte aligned, a scalar
 * path otherwise.  rvlm_square_accept is the accept step of both norms. */
int rvlm_square_l2_propose(const float* x, const float* x_best, const int64_t* idx, int n_active, int C, int H, int W, int vh,
                           int vw, int vh2, int vw2, int s, float eps, const float* eta, const float* sign, float* x_new,
                           int32_t* flags, rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * FAB / FAB-T, L-inf (RVLM_HAS_FAB): the device arithmetic of one iteration of FABAttack.attack_single_run
 * (autoattack/fab_base.py:160-254).  The loop itself is sequenced by the host (robustvlm_amd/fab.py) without a
 * synchronisation; scratch and state are the caller's tensors.  One workgroup per row / image, deterministic sums.
 * ------------------------------------------------------------------------------------------- */
/* projection_linf (autoattack/fab_projections.py:7-58) without the sort: for each of R rows, d [R, D] with the smallest
 * max|d_i| such that w.(t + d) = b and 0 <= t + d <= 1 - d_i = dir_i * min(lambda, room_i), dir_i = sign(b - w.t) sign(w_i),
 * room_i = distance of t_i to the box face in that direction (0 where w_i = 0), lambda the smallest fp32 with
 * sum_i |w_i| min(lambda, room_i) >= |b - w.t|; every coordinate to its face when the hyperplane misses the box.
 * lambda (optional, [R]) = max_i |d_i|.  flags (optional) |= RVLM_FLAG_FAB_NONFINITE for a row with NaN / Inf, whose d is 0.
 * The search is a fixed number of passes whatever the data. */
int rvlm_fab_projection_linf(const float* t, const float* w, const float* b, int R, size_t D, float* d, float* lambda,
                             int32_t* flags, rvlm_stream_t stream);
/* fab_base.py:166-226 for B images of n_per_sample pixels given the chosen class' df [B] and dg [B, n]: b = -df + dg.x1, the
 * projections d1 of x1 and d0 of x0 (the clean image) onto dg.z = b, alpha = min(max(a1 / (a1 + a0), 0), alpha_max) with
 * a = max(max|d|, 1e-8), and IN PLACE x1 = clamp((x1 + eta d1) (1 - alpha) + (x0 + eta d0) alpha, 0, 1); d1 / d0 are never
 * stored.  lambda (optional, [B, 2]) = max|d1|, max|d0|. */
int rvlm_fab_linf_step(float* x1, const float* x0, const float* dg, const float* df, int B, size_t n_per_sample,
                       float alpha_max, float eta, float* lambda, int32_t* flags, rvlm_stream_t stream);
/* fab_base.py:228-252 after the prediction forward: for the images with pred_eq[b] == 0 (x1 is misclassified),
 * t = max|x1 - x0|; t < res2[b] -> adv[b] = x1[b], res2[b] = t; then the backward step x1 = x0 + (x1 - x0) * beta. */
int rvlm_fab_track_best(float* x1, const float* x0, float* adv, float* res2, const uint8_t* pred_eq, float beta, int B,
                        size_t n_per_sample, rvlm_stream_t stream);
/* Untargeted FAB, class k of the Jacobian streamed class by class instead of the [K, B, D] tensor of fab_pt.py:76-98:
 * w = g_k - g_y, dist = |df_k| / (1e-12 + |w|_1) (fab_base.py:166-170); where y[b] != k and dist < best_dist[b] (strictly:
 * the first minimum wins like min(dim=1)[1], :181) -> best_dist[b] = dist, best_df[b] = df_k[b], best_w[b] = w.  The caller
 * starts best_dist at +inf and calls k = 0 .. K-1 in order. */
int rvlm_fab_jacobian_argmin(const float* g_k, const float* g_y, const float* df_k, const int64_t* y, int k, int B,
                             size_t n_per_sample, float* best_dist, float* best_df, float* best_w, rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Whole loops, device resident (no host sync inside): replace
 *   pgd()        train/pgd_train.py:5-68          -> rvlm_pgd_run
 *   apgd_train() train/apgd_train.py:125-373      -> rvlm_apgd_run (train_variant = 1)
 *   APGDAttack.attack_single_run autopgd_base.py:205-451 -> rvlm_apgd_run (train_variant = 0)
 *   apgd()       vlm_eval/attacks/apgd.py:163-368 on the token loss, per image -> rvlm_apgd_run_tokens (RVLM_HAS_TOKEN_APGD)
 * with the FARE / TeCoA losses bound (ComputeLossWrapper, …clip.py:260-274).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t loss_kind;        /* RVLM_LOSS_* */
    int32_t reduction;        /* pgd: MEAN (trainer) ; apgd: NONE */
    int32_t output_normalize; /* F.normalize the embedding */
    int32_t n_classes;        /* C for CE (columns of ref) */
    float logit_scale;        /* 100. */
    const float* ref;         /* L2: embedding_orig [B,D];  CE: T [D,C] */
    const int64_t* targets;   /* [B] (CE, and the argmax test of apgd); may be NULL for pgd+L2 */
    const int64_t* y_target;  /* [B] target classes, RVLM_LOSS_DLR_TARGETED / RVLM_LOSS_LOGIT_DIFF (else NULL) */
} rvlm_loss_spec;

/* x_adv_out = pgd(...) ; delta0 may be NULL (zeros).  flags: see RVLM_FLAG_*.
 * loss_trace (optional, [iterations]) receives the scalar loss of every iteration. */
int rvlm_pgd_run(rvlm_vit* h, const float* x, const float* delta0, int B,
                 const rvlm_loss_spec* loss, float eps, int iterations, float stepsize,
                 float momentum, int mode_max, float* x_adv_out, float* loss_trace,
                 int32_t* flags, rvlm_stream_t stream);

/* pgd() with the norm as a parameter: norm_kind 0 = L-inf (rvlm_pgd_run), 2 = L2 (rvlm_pgd_l2_update per iteration). */
int rvlm_pgd_run_norm(rvlm_vit* h, const float* x, const float* delta0, int B, const rvlm_loss_spec* loss, int norm_kind,
                      float eps, int iterations, float stepsize, float momentum, int mode_max, float* x_adv_out,
                      float* loss_trace, int32_t* flags, rvlm_stream_t stream);

/* pgd() in two precisions: iterations [0, n_first) evaluate forward + loss + input gradient on h_first, a second handle of
 * the SAME model (its fp32 mode: the reference's own precision, train/pgd_train.py:30-38), the rest on h; the attack state
 * lives in h.  loss->ref should be the h_first-precision embedding (FARE's first cotangent is a difference of nearly equal
 * embeddings).  Both handles need max_batch >= B. */
int rvlm_pgd_run_mixed(rvlm_vit* h, rvlm_vit* h_first, int n_first, const float* x, const float* delta0, int B,
                       const rvlm_loss_spec* loss, int norm_kind, float eps, int iterations, float stepsize, float momentum,
                       int mode_max, float* x_adv_out, float* loss_trace, int32_t* flags, rvlm_stream_t stream);

/* rvlm_pgd_run_mixed with the handoff (ABI 109): iterations [0, n_first) evaluate forward + loss on h_first (fp32 storage) and the
 * input gradient on h's bf16 kernels from h_first's saved forward (rvlm_vit_backward_input_from).  Same max_batch on both. */
int rvlm_pgd_run_mixed_fwd(rvlm_vit* h, rvlm_vit* h_first, int n_first, const float* x, const float* delta0, int B,
                           const rvlm_loss_spec* loss, int norm_kind, float eps, int iterations, float stepsize, float momentum,
                           int mode_max, float* x_adv_out, float* loss_trace, int32_t* flags, rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Token-level outputs and their input gradient (RVLM_HAS_TOKENS): what a VLM reads from the tower.
 *   LLaVA        llava/model/multimodal_encoder/clip_encoder.py:55-65, 77-90: select_layer = -2 (the last resblock dropped),
 *                output_tokens, proj = None, feature_select takes the patch tokens [:, 1:]      -> depth = layers - 1
 *   OpenFlamingo open_flamingo/src/factory.py:41, flamingo.py:217,242: visual.output_tokens = True, vision_encoder(x)[1]
 *                                                                                             -> depth = layers
 *   vlm_eval/attacks/pgd.py, apgd.py differentiate the VLM's loss through those tokens down to the pixels.
 * depth in 1..layers = resblocks run; tokens = the fp32 residual stream after block depth - 1, all S rows [B, S, W] (class row
 * first: the caller slices).  Plain RVLM_PREC_BF16 / F32 / F32X3 handles; a forward-provider (trainable = -2) or inference-only
 * handle is refused where activations would be kept.  The class-token tail of the bf16 handle is bypassed for a token pass (its last
 * block runs on every row); pooled passes before and after are unchanged.
 * ------------------------------------------------------------------------------------------- */
enum { RVLM_TOKENS_ALL = 0, RVLM_TOKENS_PATCH = 1 };   /* rows of the token loss: all S, or the S - 1 patch rows ([:, 1:]) */

/* out_tokens [B, S, W] fp32.  ln_post = 1: ln_post applied to every row first (releases of open_clip that normalise the tokens
 * they return); 0: the raw residual stream.  out_emb (optional, depth == layers only): the pooled embedding [B, D], un-normalised,
 * the bits rvlm_vit_forward gives on an fp32-storage handle.  save = 1 keeps the activations for rvlm_vit_backward_input_tokens
 * (the first ln_post pass of a handle allocates the row statistics it needs: 2 floats per token row).  save = 2
 * (RVLM_HAS_TOKEN_TRAINING; `trainable` handles, RVLM_ERR_ARG on any other) additionally keeps the inputs of every linear layer of
 * blocks 0 .. depth - 1 for rvlm_vit_backward_params_tokens; rvlm_vit_backward_input_tokens reads such a pass too. */
int rvlm_vit_forward_tokens(rvlm_vit* h, const float* x, const float* delta, int B, int depth, int ln_post, int save,
                            float* out_tokens, float* out_emb, rvlm_stream_t stream);

/* grad_x [B, 3, in_h, in_w] = d(<d_tokens, tokens> + <d_emb, emb>) / dx of the token pass saved last (vlm_eval/attacks/pgd.py:
 * torch.autograd.grad through CLIPVisionTower.forward).  d_tokens [B, S, W] fp32; d_emb [B, D] optional, depth == layers only.
 * RVLM_ERR_STATE: no saved token pass for this B (a pooled forward, any later forward, another batch size); the pooled backwards
 * (rvlm_vit_backward_input, _params, _input_from) return RVLM_ERR_STATE after a token forward. */
int rvlm_vit_backward_input_tokens(rvlm_vit* h, const float* d_tokens, const float* d_emb, int B, float* grad_x,
                                   rvlm_stream_t stream);

/* Weight gradients through the token door (RVLM_HAS_TOKEN_TRAINING): for the token pass saved last with save = 2 on a `trainable`
 * handle, writes (accumulate == 0) or adds (accumulate != 0) d(<d_tokens, tokens> + <d_emb, emb>) / d(param) into the fp32 tensors
 * `grads` points to.  d_tokens [B, S, W] fp32, required; d_emb [B, D] optional, depth == layers only (else RVLM_ERR_ARG).  The saved
 * pass's ln_post flag is honoured.  No input gradient is produced.  Parameters the cotangent cannot reach - proj unless d_emb is
 * given, ln_post.* unless the pass applied ln_post or d_emb is given, every block >= depth - are zero-filled when accumulate == 0
 * and left untouched otherwise.  RVLM_ERR_STATE: handle not trainable; the last saved forward is pooled, a token pass with
 * save != 2, or of another B.  The pooled backwards keep returning RVLM_ERR_STATE after any token forward. */
int rvlm_vit_backward_params_tokens(rvlm_vit* h, const float* d_tokens, const float* d_emb, int B, const rvlm_vit_weights* grads,
                                    int accumulate, rvlm_stream_t stream);
/* The same pass in the stages of rvlm_vit_backward_params_stages (same numbers, same in-order rule; stage 0 restarts).  Stage 0
 * seeds the residual-gradient stream from d_tokens (through ln_post's backward over every row where the pass applied it, plus the
 * pooled path's class rows when d_emb is given) and owns proj / ln_post; an unreached parameter is zero-filled by the stage that
 * owns it. */
int rvlm_vit_backward_params_tokens_stages(rvlm_vit* h, const float* d_tokens, const float* d_emb, int B,
                                           const rvlm_vit_weights* grads, int accumulate, int stage_begin, int stage_end,
                                           rvlm_stream_t stream);

/* Logging metric of the token training step, the token twin of rvlm_cosine_rows (RVLM_HAS_TOKEN_TRAINING): out_per_image[b] = the
 * mean over the selected rows of F.cosine_similarity(tokens[b, s], ref_tokens[b, s - select]) (eps 1e-8: a.b / sqrt(max(|a|^2 |b|^2,
 * 1e-16))); shapes and `select` as in rvlm_tokens_l2_loss_grad.  out_mean (optional) = their mean over b.  scratch: B * ceil(S / 8)
 * floats.  Fixed summation order (bit-reproducible), no atomics.  W % 8 == 0, 16-byte aligned pointers. */
int rvlm_tokens_cosine(const float* tokens, const float* ref_tokens, int B, int S, int W, int select, float* out_per_image,
                       float* out_mean, float* scratch, rvlm_stream_t stream);

/* FARE's embedding loss (train/adversarial_training_clip.py:509-521) over the tokens the VLM reads, fused with the start of the
 * backward: loss_per_sample[b] = sum over the selected rows and W of (tokens - ref_tokens)^2, ref_tokens [B, S - select, W];
 * d = 2 (tokens - ref) (x 1 / B for RVLM_RED_MEAN) written as fp32 (seed_f32) and / or bf16 (seed_bf16), [seed_rows, W] with
 * unselected rows and rows B S .. seed_rows - 1 zero (seed_rows = 0: B S); both NULL: loss only.  loss_scalar (optional) = mean
 * or sum of loss_per_sample.  scratch: B * ceil(S / 8) floats.  Fixed summation order (bit-reproducible).  flags (optional)
 * |= RVLM_FLAG_TOKENS_NONFINITE.  W % 8 == 0, 16-byte aligned pointers. */
int rvlm_tokens_l2_loss_grad(const float* tokens, const float* ref_tokens, int B, int S, int W, int select, int reduction,
                             float* seed_f32, uint16_t* seed_bf16, long seed_rows, float* loss_per_sample, float* loss_scalar,
                             float* scratch, int32_t* flags, rvlm_stream_t stream);

/* The token twin of rvlm_vit_fwd_inputgrad: forward to `depth` (activations kept), the token loss above against ref_tokens, input
 * gradient.  Every output pointer is optional (out_tokens [B, S, W], out_loss_per_sample [B], out_loss_scalar [1], out_grad_x). */
int rvlm_vit_tokens_fwd_inputgrad(rvlm_vit* h, const float* x, const float* delta, int B, int depth, int ln_post, int select,
                                  const float* ref_tokens, int reduction, float* out_tokens, float* out_loss_per_sample,
                                  float* out_loss_scalar, float* out_grad_x, rvlm_stream_t stream);

/* rvlm_pgd_run_norm (train/pgd_train.py:5-68; vlm_eval/attacks/pgd.py) with the token loss as the model step: the unsupervised
 * attack on what the VLM sees.  flags: RVLM_FLAG_* of the update kernels and RVLM_FLAG_TOKENS_NONFINITE. */
int rvlm_pgd_run_tokens(rvlm_vit* h, const float* x, const float* delta0, int B, int depth, int ln_post, int select,
                        const float* ref_tokens, int reduction, int norm_kind, float eps, int iterations, float stepsize,
                        float momentum, int mode_max, float* x_adv_out, float* loss_trace, int32_t* flags, rvlm_stream_t stream);

/* apgd() of vlm_eval/attacks/apgd.py:163-368 (L-inf and L2 branches, mask = None, maximising) with the token loss as the model, run
 * independently for every image of the batch (RVLM_HAS_TOKEN_APGD).  The per-image loss is the RVLM_RED_NONE form of
 * rvlm_tokens_l2_loss_grad - sum over the selected rows and W of (tokens - ref_tokens)^2, seed 2 (t - ref) without a 1 / B.
 * Start: clamp(x_init ? x_init : x, 0, 1), forward + backward.  Each of the n_iter (1..1024) iterations: rvlm_apgd_linf_step /
 * rvlm_apgd_l2_step (a = 1.0 at i == 0, else 0.75), forward + loss, backward unless i == n_iter - 1 (:300-304),
 * rvlm_apgd_controller_rho with an all-zero `pred` (as rvlm_apgd_masked_bookkeeping: x_best_adv follows the last iterate, :310) and
 * the oscillation threshold `rho` (the reference: 0.75), rvlm_apgd_select.  The checkpoint schedule is the host's; nothing is read
 * back or allocated, the state lives in the handle's attack buffers.  step0 = alpha * eps (the reference: alpha = 2).
 * Outputs: x_best_out [B, 3, in_h, in_w] (required) / loss_best_out [B] = the iterate of highest loss and that loss; x_last_out
 * (optional) = the reference's third return value x_best_adv; loss_trace_out (optional, [n_iter + 1, B]): row 0 the start point's
 * loss, row i + 1 the loss after iteration i; step_out (optional, [B]) the final step sizes.  flags (optional): RVLM_FLAG_NAN_GRAD
 * from the steps, RVLM_FLAG_TOKENS_NONFINITE from the loss.  norm_kind other than 0 / 2: RVLM_ERR_UNSUPPORTED; depth, select, B,
 * handle kind and scratch size are refused as by rvlm_pgd_run_tokens.  Leaves a saved token pass, like every token loop. */
int rvlm_apgd_run_tokens(rvlm_vit* h, const float* x, const float* x_init, int B, int depth, int ln_post, int select,
                         const float* ref_tokens, int norm_kind, float eps, int n_iter, float step0, float rho, float* x_best_out,
                         float* loss_best_out, float* x_last_out, float* loss_trace_out, float* step_out, int32_t* flags,
                         rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * VLM-side attacks (RVLM_HAS_VLM_ATTACKS): the arithmetic of one iteration of vlm_eval/attacks/pgd.py (class PGD) and apgd.py
 * (apgd) - everything but the model's forward and backward.  The attacked tensor is contiguous fp32 [B, n_img, P] (the reference's
 * [B, n_img, 1, 3, H, W]; P = elements of one image), `mask` is uint8 [n_img]: 1 = attacked, 0 = masked out (mask_out =
 * 'context' -> 0...01, 'query' -> 1...10, an int -> that entry 0); NULL = every image attacked.  A masked gradient is g * 0 as in
 * the reference (NaN / Inf stay NaN), masked images are stepped along that zero gradient and projected with their sample, not
 * skipped: they come out bit-identical to what went in for L-inf when they lie in the eps-ball and [0,1] (every output of these
 * calls does), for L2 when they equal x.  16-byte accesses when P % 4 == 0 and the pointers are 16-byte aligned.  B * n_img <= 65535.
 * norm_kind: 0 = L-inf, 2 = L2 (anything else: RVLM_ERR_UNSUPPORTED; the reference's L1 / L0 branches are not covered).  The L2 forms
 * run one workgroup per sample with fixed-order fp32 sums (bit-reproducible; equal to torch to fp32 rounding of the norms).
 * flags: optional device word, RVLM_FLAG_*.
 * ------------------------------------------------------------------------------------------- */
/* out = mask * grad (pgd.py:40, apgd.py:223-224,303-304); out may be grad.  flags |= RVLM_FLAG_NAN_GRAD if the product holds a
 * NaN (it is left in place: apgd keeps it; rvlm_pgd_masked_update zeroes it itself). */
int rvlm_mask_grad(const float* grad, const uint8_t* mask, int B, int n_img, size_t P, float* out, int32_t* flags,
                   rvlm_stream_t stream);
/* One iteration of PGD.perturb after the gradient (pgd.py:39-65): g = mask * grad, NaN -> 0 (RVLM_FLAG_NAN_GRAD), normalize_grad
 * (sign | g / max(|g|_2, 1e-12) per sample, the norm over the MASKED gradient), velocity = normalize(momentum * velocity + g),
 * delta -+= stepsize * velocity (mode_max = 0: minimise), project_perturbation (clamp to +-eps | torch.renorm to eps), and if
 * image_space: delta = clamp(x + delta, 0, 1) - x with RVLM_FLAG_ADV_RANGE where x + delta leaves (-1e-6, 1 + 1e-6) (:62-64).
 * RVLM_FLAG_NAN_DELTA: NaN in delta (:65).  grad is the RAW gradient.  x_adv_out (optional) = x + delta. */
int rvlm_pgd_masked_update(const float* x, const float* grad, float* delta, float* velocity, const uint8_t* mask, int B, int n_img,
                           size_t P, int norm_kind, float eps, float stepsize, float momentum, int mode_max, int image_space,
                           float* x_adv_out, int32_t* flags, rvlm_stream_t stream);
/* One gradient step of apgd (apgd.py:242-266): momentum step with a = 1.0 (first iteration) | 0.75, both projections, x_adv_old
 * <- x_adv, x_adv <- the new point; step [B] is read from device memory.  grad may be the raw or the already masked gradient (the
 * mask is applied here; mask * mask = mask).  flags |= RVLM_FLAG_NAN_GRAD for a NaN in mask * grad (not zeroed: the reference
 * does not). */
int rvlm_apgd_masked_step(const float* x, float* x_adv, float* x_adv_old, const float* grad, const uint8_t* mask, const float* step,
                          float a, float eps, int B, int n_img, size_t P, int norm_kind, int32_t* flags, rvlm_stream_t stream);
/* apgd.py:321-351 for iteration i with [B] losses: loss_steps[i] = loss_i, the best-loss select of x_best / grad_best / loss_best,
 * x_best_adv = x_adv (:310), and at a checkpoint (do_check; the host knows k and counter3, they do not depend on data) the
 * oscillation test, step halving and restart of x_adv / grad from x_best / grad_best.  It is rvlm_apgd_controller (rho = 0.75) +
 * rvlm_apgd_select with "never classified correctly" for every sample - their semantics equal this function's, no kernel of its
 * own.  scratch: 5 * B bytes, zeroed by the caller before the first iteration and not touched by it between iterations.
 * loss_steps [n_iter, B]; n_per_sample = n_img * P. */
int rvlm_apgd_masked_bookkeeping(int i, int B, int n_iter, int k, int do_check, const float* loss_i, float* loss_steps,
                                 float* loss_best, float* loss_best_last_check, float* reduced_last_check, float* step,
                                 float* x_adv, float* grad, float* x_best, float* grad_best, float* x_best_adv, uint8_t* scratch,
                                 size_t n_per_sample, rvlm_stream_t stream);

/* APGD L-inf.  x_init: NULL -> start from clamp(x,0,1) (apgd_train) or the caller-provided random
 * start (APGDAttack).  logits_from_head: 0 -> the `argmax(model output)==y` test runs on the
 * embedding (apgd_train quirk); 1 -> on emb @ (logit_scale*T) logits
 * (ClassificationModel, CLIP_eval/clip_robustbench.py:50-69).
 * Outputs (each optional): x_best_adv, x_best, loss_best [B], acc u8[B]. */
int rvlm_apgd_run(rvlm_vit* h, const float* x, const float* x_init, int B,
                  const rvlm_loss_spec* loss, float eps, int n_iter, float alpha,
                  int train_variant, int logits_from_head, float* x_best_adv, float* x_best,
                  float* loss_best, uint8_t* acc, rvlm_stream_t stream);

/* `rho` of APGDAttack for the following rvlm_apgd_run* calls WITH train_variant == 0 on this handle (default 0.75).
 * train/apgd_train.py has no such parameter: train_variant != 0 runs always use 0.75, whatever was set here.
 * Returns RVLM_ERR_ARG for NaN. */
int rvlm_vit_set_apgd_rho(rvlm_vit* h, double rho);

/* SURVEY.md section 8(b) `rvlm_vit_fwd_inputgrad`: ONE iteration's model work in one call - forward of x (+ delta,
 * may be NULL) with the activations kept, the bound FARE / TeCoA loss, and grad_x = d loss / d (x + delta)
 * (pgd_train.py:33-38: out = forward(...); loss = loss_fn(out, targets); autograd.grad(loss, perturbation)).
 * Outputs (each optional): out_emb [B,out_dim], out_loss_per_sample [B], out_loss_scalar [1] (per loss->reduction),
 * out_grad_x [B,3,H,W].  Equivalent to rvlm_vit_forward(save=1) + rvlm_loss_grad + rvlm_vit_backward_input. */
int rvlm_vit_fwd_inputgrad(rvlm_vit* h, const float* x, const float* delta, int B, const rvlm_loss_spec* loss,
                           float* out_emb, float* out_loss_per_sample, float* out_loss_scalar, float* out_grad_x,
                           rvlm_stream_t stream);

/* rvlm_apgd_run with the norm as a parameter: norm_kind 0 = L-inf, 2 = L2 (apgd_train(norm='l2'); train_variant only). */
int rvlm_apgd_run_norm(rvlm_vit* h, const float* x, const float* x_init, int B, const rvlm_loss_spec* loss, int norm_kind,
                       float eps, int n_iter, float alpha, int train_variant, int logits_from_head, float* x_best_adv,
                       float* x_best, float* loss_best, uint8_t* acc, rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Input front end: replaces Compose([Resize(size, bicubic), CenterCrop(size),
 * ToTensor()]) over a decoded RGB image (train/adversarial_training_clip.py:105-116; torchvision 0.15.2 over Pillow).
 * img_hwc: device uint8 [H, W, 3]; out_chw: device float32 [3, size, size] in [0,1] (NOT normalised).  Bit-exact with
 * Pillow's 8-bit bicubic resampler.  The taps of an input shape are computed on the host and cached in the object:
 * consecutive images of equal shape cost one kernel launch.  max_input_dim bounds the longer input edge.
 * ------------------------------------------------------------------------------------------- */
typedef struct rvlm_preproc rvlm_preproc;
int rvlm_preproc_create(int size, int max_input_dim, rvlm_preproc** out);
int rvlm_preproc_destroy(rvlm_preproc* p);
int rvlm_preproc_run(rvlm_preproc* p, const uint8_t* img_hwc, int H, int W, float* out_chw, rvlm_stream_t stream);
/* A batch of n decoded images of any mix of shapes in ONE kernel launch (the reference's DataLoader hands over batches of
 * 128, train/adversarial_training_clip.py:119-148): imgs_hwc / H / W are HOST arrays of n device pointers / heights /
 * widths; out: device float32 [n, 3, size, size].  Tables are staged through pinned memory and copied on `stream`; the call
 * does not synchronise the stream.  Same arithmetic as rvlm_preproc_run (bit-identical outputs). */
int rvlm_preproc_run_batch(rvlm_preproc* p, const uint8_t* const* imgs_hwc, const int* H, const int* W, int n, float* out,
                           rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Data-parallel trainer: gradient all-reduce over RCCL / xGMI, one process per GPU.
 * Replaces the reduction the reference gets from torch.nn.DataParallel (train/adversarial_training_clip.py:184-191).
 * Rendezvous: rank 0 calls rvlm_comm_unique_id and hands the 128 bytes to every rank by whatever channel the host has
 * (launcher environment, file, socket); every rank then calls rvlm_comm_create on its own GPU (collective call).
 * rvlm_allreduce_grads: in-place SUM of buf[0 .. count) (device pointer) over the ranks, asynchronous on `stream`; the
 * 1 / world factor goes into rvlm_adamw_step (grad_scale).  The attack entry points need none of this: every quantity of
 * pgd / apgd_train / APGDAttack is per sample.  librccl is loaded at the first rvlm_comm_* call (RVLM_ERR_UNSUPPORTED if
 * the host has none).
 * ------------------------------------------------------------------------------------------- */
#define RVLM_COMM_ID_BYTES 128
#define RVLM_DTYPE_F32 0
#define RVLM_DTYPE_BF16 1
typedef struct rvlm_comm rvlm_comm;
int rvlm_comm_unique_id(uint8_t* out_id /* [RVLM_COMM_ID_BYTES], host memory */);
int rvlm_comm_create(const uint8_t* id, int rank, int world, rvlm_comm** out);
int rvlm_comm_destroy(rvlm_comm* comm);
int rvlm_comm_info(const rvlm_comm* comm, int* rank, int* world);
int rvlm_allreduce_grads(rvlm_comm* comm, void* buf, size_t count, int dtype, rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Text tower: open_clip CLIP.encode_text, forward only (RVLM_HAS_TEXT).  Builds the zero-shot / TeCoA head
 * embedding_text_labels_norm = encode_text(tokenize(prompts), normalize=True).T that the reference
 * computes under no_grad on the frozen model (train/adversarial_training_clip.py:150-180,
 * CLIP_eval/eval_utils.py:63-85, 80-template ensemble CLIP_eval/clip_robustbench.py:186-224).
 * Tokenisation stays with the caller: tokens are what open_clip.tokenize returns.
 * ------------------------------------------------------------------------------------------- */
typedef struct rvlm_text rvlm_text;
typedef struct {
    int32_t vocab;     /* 49408 */
    int32_t context;   /* 77 (<= 96) */
    int32_t width;     /* = heads * 64 */
    int32_t layers;
    int32_t heads;
    int32_t out_dim;   /* multiple of 4 */
    int32_t act;       /* RVLM_ACT_* (QuickGELU for OpenAI weights) */
    int32_t precision; /* RVLM_PREC_* */
    int32_t max_batch; /* prompts per call; 0 -> 1024 */
} rvlm_text_config;
typedef struct {
    const float* token_embedding;      /* [vocab, W]   */
    const float* positional_embedding; /* [context, W] */
    const float* ln_final_weight;      /* [W] */
    const float* ln_final_bias;
    const float* text_projection;      /* [W, out_dim] */
    const rvlm_vit_block_weights* blocks_host; /* HOST array of `layers` structs of device ptrs: the vision tower's block layout */
} rvlm_text_weights;
/* model_orig = open_clip.create_model_and_transforms(...) (train/adversarial_training_clip.py:95-97): copies / converts the text
 * weights, allocates the workspace.  RVLM_ERR_UNSUPPORTED for RVLM_PREC_F32X3 with a max_batch whose fc2 split operand would pass
 * 2^31 bytes (about 1 500 prompts at width 768). */
int rvlm_text_create(const rvlm_text_config* cfg, const rvlm_text_weights* weights, rvlm_stream_t stream, rvlm_text** out);
int rvlm_text_destroy(rvlm_text* h);
size_t rvlm_text_workspace_bytes(const rvlm_text* h);
/* out_emb[N, out_dim] = model_orig.encode_text(tokens, normalize=normalize) (train/adversarial_training_clip.py:166-170,
 * CLIP_eval/eval_utils.py:74-78): tokens [N, context] int32 on the device, N <= max_batch.  active_len: only the first active_len
 * positions of every prompt are evaluated (the mask is causal: nothing behind a prompt's EOT reaches its EOT row); it must exceed
 * every prompt's EOT position; 0 = the full context.  flags: optional device word, |= RVLM_FLAG_TOKEN_RANGE / RVLM_FLAG_EOT_ACTIVE
 * (the call itself never faults on such input; the embeddings of that call are then meaningless). */
int rvlm_text_encode(rvlm_text* h, const int32_t* tokens, int N, int active_len, int normalize, float* out_emb, uint32_t* flags,
                     rvlm_stream_t stream);

/* ---------------------------------------------------------------------------------------------
 * Measurement support: per-kernel-class HIP-event timing on the engine's stream.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    char name[48];
    double total_ms;  /* sum of launch durations */
    double flops;     /* algorithmic FLOPs of those launches (2/MAC, GEMM-shaped work only) */
    double bytes;     /* algorithmic bytes (HBM-bound kernels) */
    int64_t launches;
} rvlm_profile_entry;
int rvlm_vit_set_profiling(rvlm_vit* h, int enabled);
/* Synchronises the device; writes up to *n entries, sets *n to the count. */
int rvlm_vit_get_profile(rvlm_vit* h, rvlm_profile_entry* out, int* n);
int rvlm_vit_reset_profile(rvlm_vit* h);

const char* rvlm_last_error(void);
int rvlm_version(void);   /* = RVLM_VERSION.  101: rvlm_loss_spec.y_target, rvlm_loss_grad(y_target), DLR losses;
                           * 102: square-attack kernels; 103: rvlm_vit_fwd_inputgrad, rvlm_vit_backward_params_stages,
                           * rvlm_ce_logits, rvlm_head_logits(_bwd), double hyper-parameters in rvlm_adamw_step,
                           * rvlm_pgd_l2_update, rvlm_pgd_run_norm, rvlm_apgd_l2_step, rvlm_apgd_run_norm,
                           * rvlm_project_perturbation, rvlm_normalize_grad; 104: rvlm_preproc_run_batch, rvlm_ce_logits takes B = 1,
                           * rvlm_vit_backward_params_stages refuses out-of-order stages; 105: rvlm_apgd_controller_rho,
                           * rvlm_vit_set_apgd_rho, rvlm_comm_* / rvlm_allreduce_grads; 106: rvlm_pgd_run_mixed, fp32 mode on v_mfma_f32_32x32x2_f32;
                           * 107: rvlm_l2_random_start; 108: RVLM_PREC_F32X3 (split-bf16 linears over fp32 storage);
                           * 109: rvlm_vit_backward_input_from, rvlm_vit_forward_for, rvlm_vit_set_flash_inference, rvlm_pgd_run_mixed_fwd (fp32-storage forward, bf16 backward);
                           * still 109, additions only: rvlm_text_* (CLIP text tower, forward only, announced by RVLM_HAS_TEXT);
                           * rvlm_fab_* (FAB / FAB-T L-inf), RVLM_LOSS_LOGIT_DIFF, RVLM_FLAG_FAB_NONFINITE (announced by RVLM_HAS_FAB);
                           * rvlm_vit_set_input_size, rvlm_resize_bicubic(_adjoint), rvlm_resize_taps (announced by RVLM_HAS_INPUT_RESIZE);
                           * rvlm_vit_forward_tokens, rvlm_vit_backward_input_tokens, rvlm_tokens_l2_loss_grad, rvlm_vit_tokens_fwd_inputgrad,
                           * rvlm_pgd_run_tokens, RVLM_FLAG_TOKENS_NONFINITE (announced by RVLM_HAS_TOKENS);
                           * rvlm_square_l2_propose, RVLM_FLAG_SQUARE_NONFINITE (announced by RVLM_HAS_SQUARE_L2);
                           * rvlm_sgd_step (announced by RVLM_HAS_SGD);
                           * rvlm_vit_forward_tokens(save = 2), rvlm_vit_backward_params_tokens(_stages), rvlm_tokens_cosine
                           * (announced by RVLM_HAS_TOKEN_TRAINING);
                           * rvlm_apgd_run_tokens (announced by RVLM_HAS_TOKEN_APGD) */

#ifdef __cplusplus
}
#endif
#endif /* RVLM_H */
