// The device-resident attack loops of the ViT engine (engine_internal.h): the fused forward + loss + input-gradient step and the
// PGD, mixed-precision / handoff, token and APGD loops built on it, with their entries of the C ABI.
#include <algorithm>

#include "engine_internal.h"

namespace rvlm {

__global__ void __launch_bounds__(256)
add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = a[i] + (b ? b[i] : 0.0f);
}
__global__ void __launch_bounds__(256)
clamp01_kernel(const float* __restrict__ a, float* __restrict__ out, size_t n) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = fminf(fmaxf(a[i], 0.0f), 1.0f);
}
__global__ void init_apgd_state_kernel(int B, const float* loss0, const uint8_t* pred0, float step0,
                                       float* loss_best, float* loss_best_lc, float* reduced_lc, float* step,
                                       uint8_t* acc) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
        loss_best[b] = loss0[b]; loss_best_lc[b] = loss0[b]; reduced_lc[b] = 1.0f; step[b] = step0;
        acc[b] = pred0[b];
    }
}

}  // namespace rvlm

static int loss_step(rvlm_vit* h, const rvlm_loss_spec* ls, int B, int reduction, float* loss_scalar,
                     uint8_t* pred_eq, hipStream_t s) {
    if (ls->loss_kind != RVLM_LOSS_L2) {
        RVLM_REQUIRE(ls->n_classes > 0 && ls->n_classes <= 1024, "loss: n_classes must be in 1..1024");
        RVLM_REQUIRE(ls->targets, "loss: head losses need targets");
    }
    PROF("loss", 0, 0);
    return rvlm_loss_grad(ls->loss_kind, reduction, h->emb, ls->ref, ls->targets, ls->y_target, B, h->D, ls->n_classes,
                          ls->logit_scale, h->loss_ps, loss_scalar, h->d_emb, pred_eq, h->loss_scratch, s);
}

// one call = forward (activations kept) + FARE / TeCoA loss + input gradient, i.e. what one
// iteration of pgd_train.py:33-38 asks of the model (out = forward(x + delta); loss = loss_fn(out, targets);
// grad = autograd.grad(loss, delta)).  Every output pointer is optional.
extern "C" int rvlm_vit_fwd_inputgrad(rvlm_vit* h, const float* x, const float* delta, int B, const rvlm_loss_spec* loss,
                                      float* out_emb, float* out_loss_per_sample, float* out_loss_scalar,
                                      float* out_grad_x, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x && loss && loss->ref, "rvlm_vit_fwd_inputgrad: null argument");
    RVLM_REQUIRE(B > 1 && B <= h->maxB, "rvlm_vit_fwd_inputgrad: need 1 < B <= max_batch");
    RVLM_REQUIRE(!h->inference_only, "rvlm_vit_fwd_inputgrad: inference-only handle");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = vit_forward(h, x, delta, B, loss->output_normalize, 1, h->emb, s))) return rc;
    if ((rc = loss_step(h, loss, B, loss->reduction, out_loss_scalar ? h->loss_scalar : nullptr, nullptr, s))) return rc;
    const size_t eb = (size_t)B * h->D * 4;
    if (out_emb) RVLM_HIP(hipMemcpyAsync(out_emb, h->emb, eb, hipMemcpyDeviceToDevice, s));
    if (out_loss_per_sample) RVLM_HIP(hipMemcpyAsync(out_loss_per_sample, h->loss_ps, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (out_loss_scalar) RVLM_HIP(hipMemcpyAsync(out_loss_scalar, h->loss_scalar, 4, hipMemcpyDeviceToDevice, s));
    if (out_grad_x && (rc = vit_backward(h, h->d_emb, B, out_grad_x, s))) return rc;
    return RVLM_OK;
}

// One perturbation loop; iterations [0, n_first) evaluate model and gradient on `hf` (a second handle of the same model, e.g.
// its fp32 mode), the others on `h`.  The attack state (delta, velocity, gradient) lives in h's buffers throughout; a
// handle only contributes forward + loss + input gradient (what pgd_train.py:33-38 asks of the model).
// handoff: the first iterations run forward + loss on `hf` and the input gradient on h's (bf16) kernels from hf's saved forward
// (vit_backward_from above).
// The model step of one iteration: forward(x + delta), loss (its scalar into lsc, when given), input gradient into grad.
struct PooledStep {
    rvlm_vit *h, *hf; int n_first; const rvlm_loss_spec* loss; bool handoff;
    int operator()(int it, const float* x, const float* delta, int B, float* lsc, float* grad, hipStream_t s) const;
};
template <typename Step>
static int pgd_run_impl(rvlm_vit* h, const Step& step, const float* x, const float* delta0, int B, int norm_kind, float eps,
                        int iterations, float stepsize, float momentum, int mode_max, float* x_adv_out, float* loss_trace,
                        int32_t* flags, hipStream_t s) {
    const size_t n = (size_t)B * 3 * h->in_h * h->in_w;
    float *delta = h->img_buf[0], *vel = h->img_buf[1], *grad = h->img_buf[2];
    int rc;
    if (flags && (rc = rvlm_check_image_range(x, n, flags, s))) return rc;
    if (delta0) RVLM_HIP(hipMemcpyAsync(delta, delta0, n * 4, hipMemcpyDeviceToDevice, s));
    else RVLM_HIP(hipMemsetAsync(delta, 0, n * 4, s));
    RVLM_HIP(hipMemsetAsync(vel, 0, n * 4, s));
    if (iterations == 0) {
        hipLaunchKernelGGL(add_kernel, dim3(ew_blocks(n)), dim3(256), 0, s, x, (const float*)delta, x_adv_out, n);
        RVLM_CHECK_LAUNCH();
    }
    for (int it = 0; it < iterations; ++it) {
        float* lsc = loss_trace ? loss_trace + it : (it < 4096 ? h->loss_scalar + it : nullptr);
        if ((rc = step(it, x, delta, B, lsc, grad, s))) return rc;
        {
            PROF("linf_update", 0, (double)n * 28);
            float* xo = it == iterations - 1 ? x_adv_out : nullptr;
            if (norm_kind == 2) rc = rvlm_pgd_l2_update(x, grad, delta, vel, n / B, B, eps, stepsize, momentum, mode_max, xo, flags, s);
            else rc = rvlm_pgd_linf_update(x, grad, delta, vel, n, eps, stepsize, momentum, mode_max, xo, flags, s);
            if (rc) return rc;
        }
    }
    return RVLM_OK;
}

int PooledStep::operator()(int it, const float* x, const float* delta, int B, float* lsc, float* grad, hipStream_t s) const {
    rvlm_vit* m = (hf && it < n_first) ? hf : h;
    // (a handoff iteration's forward runs FOR h: it writes h's bf16 tensors itself and keeps no probabilities)
    int rc = vit_forward(m, x, delta, B, loss->output_normalize, 1, m->emb, s, (handoff && m != h) ? h : nullptr);
    if (rc) return rc;
    if ((rc = loss_step(m, loss, B, loss->reduction, lsc, nullptr, s))) return rc;
    return (handoff && m != h) ? vit_backward_from(h, m, m->d_emb, B, grad, s) : vit_backward(m, m->d_emb, B, grad, s);
}

// The norm / batch / iteration checks of the perturbation loops' entries, under the entry's name (hf: the second handle of a mixed
// loop; h == null: the entry has a batch rule of its own)
static int pgd_loop_check(const std::string& who, int norm_kind, int iterations, int n_first, int B, const rvlm_vit* h,
                          const rvlm_vit* hf = nullptr) {
    if (norm_kind != 0 && norm_kind != 2) return fail(RVLM_ERR_UNSUPPORTED, who + ": norm must be L-inf (0) or L2 (2)");
    if (h && !(B > 1 && B <= h->maxB && (!hf || B <= hf->maxB)))
        return fail(RVLM_ERR_ARG, who + (hf ? ": need 1 < B <= max_batch of both handles" : ": need 1 < B <= max_batch"));
    if (!(iterations >= 0 && iterations <= 4096 && n_first >= 0)) return fail(RVLM_ERR_ARG, who + ": iterations");
    return RVLM_OK;
}

extern "C" int rvlm_pgd_run_norm(rvlm_vit* h, const float* x, const float* delta0, int B,
                                 const rvlm_loss_spec* loss, int norm_kind, float eps, int iterations, float stepsize,
                                 float momentum, int mode_max, float* x_adv_out, float* loss_trace,
                                 int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x && loss && x_adv_out && loss->ref, "rvlm_pgd_run: null argument");
    int rc = pgd_loop_check("rvlm_pgd_run", norm_kind, iterations, 0, B, h); if (rc) return rc;
    return pgd_run_impl(h, PooledStep{h, nullptr, 0, loss, false}, x, delta0, B, norm_kind, eps, iterations, stepsize, momentum,
                        mode_max, x_adv_out, loss_trace, flags, (hipStream_t)stream);
}

// Mixed-precision loop (precision "bf16+fp32-first" of the Python mirror): the first n_first iterations on h_first - a
// handle of the SAME model in the reference's own precision (fp32: train/pgd_train.py:30-38 runs no autocast) - and the
// rest on h.  FARE's first cotangent 2 (phi(x + d0) - phi(x)) is a difference of two nearly equal embeddings (~1e-2 of
// their norm at the random start), one part bf16 rounding noise in three; one fp32
// iteration - with loss->ref = the fp32 embedding of x - gives the reference's first step, after which the difference has
// grown tenfold and bf16 agrees to 0.98-0.996.
extern "C" int rvlm_pgd_run_mixed(rvlm_vit* h, rvlm_vit* h_first, int n_first, const float* x, const float* delta0, int B,
                                  const rvlm_loss_spec* loss, int norm_kind, float eps, int iterations, float stepsize,
                                  float momentum, int mode_max, float* x_adv_out, float* loss_trace,
                                  int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && h_first && x && loss && x_adv_out && loss->ref, "rvlm_pgd_run_mixed: null argument");
    int rc = pgd_loop_check("rvlm_pgd_run_mixed", norm_kind, iterations, n_first, B, h, h_first); if (rc) return rc;
    RVLM_REQUIRE(h->img == h_first->img && h->P == h_first->P && h->W == h_first->W && h->L == h_first->L &&
                 h->H == h_first->H && h->D == h_first->D && h->cfg.act == h_first->cfg.act,
                 "rvlm_pgd_run_mixed: the two handles must hold the same architecture");
    RVLM_REQUIRE(!h->inference_only && !h_first->inference_only, "rvlm_pgd_run_mixed: inference-only handle");
    RVLM_REQUIRE_SAME_INPUT(h, h_first, "rvlm_pgd_run_mixed");
    return pgd_run_impl(h, PooledStep{h, h_first, n_first, loss, false}, x, delta0, B, norm_kind, eps, iterations, stepsize, momentum,
                        mode_max, x_adv_out, loss_trace, flags, (hipStream_t)stream);
}

// ... with the handoff (round 6): the first n_first iterations' FORWARD + loss on h_first (fp32 storage: x3 or fp32 precision), their
// input gradient on h's bf16 backward from h_first's saved forward - FARE's first step needs a faithful embedding difference, not a
// faithful backward.  Both handles: same architecture AND the same max_batch.
extern "C" int rvlm_pgd_run_mixed_fwd(rvlm_vit* h, rvlm_vit* h_first, int n_first, const float* x, const float* delta0, int B,
                                      const rvlm_loss_spec* loss, int norm_kind, float eps, int iterations, float stepsize,
                                      float momentum, int mode_max, float* x_adv_out, float* loss_trace,
                                      int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && h_first && x && loss && x_adv_out && loss->ref, "rvlm_pgd_run_mixed_fwd: null argument");
    int rc = pgd_loop_check("rvlm_pgd_run_mixed_fwd", norm_kind, iterations, n_first, B, h, h_first); if (rc) return rc;
    RVLM_REQUIRE(h->lin.bf16 && !h_first->lin.bf16, "rvlm_pgd_run_mixed_fwd: h must be a bf16 handle, h_first an fp32-storage (fp32 / x3) one");
    RVLM_REQUIRE(h->Mp == h_first->Mp && h->Mp0 == h_first->Mp0, "rvlm_pgd_run_mixed_fwd: the two handles need the same max_batch");
    RVLM_REQUIRE(!h->inference_only && !h_first->inference_only, "rvlm_pgd_run_mixed_fwd: inference-only handle");
    RVLM_REQUIRE_SAME_INPUT(h, h_first, "rvlm_pgd_run_mixed_fwd");
    return pgd_run_impl(h, PooledStep{h, h_first, n_first, loss, true}, x, delta0, B, norm_kind, eps, iterations, stepsize, momentum,
                        mode_max, x_adv_out, loss_trace, flags, (hipStream_t)stream);
}

// forward to `depth` + token loss (its gradient written straight into the residual-gradient stream) + input gradient
static int tokens_step(rvlm_vit* h, const float* x, const float* delta, int B, int depth, int ln_post, int select, const float* ref,
                       int reduction, float* out_tokens, float* lsc, int32_t* flags, float* grad, hipStream_t s) {
    int rc;
    if ((rc = vit_forward_tokens(h, x, delta, B, TokPass{depth, ln_post, nullptr}, 1, nullptr, s))) return rc;
    const int S = h->S, W = h->W, M = B * S;
    float* t = ln_post ? h->tok_buf : h->xs[2 * depth];
    if (out_tokens) RVLM_HIP(hipMemcpyAsync(out_tokens, t, (size_t)M * W * 4, hipMemcpyDeviceToDevice, s));
    const bool want = grad != nullptr;
    const bool lp_only = h->lin.bf16 && h->lp_dres;
    {
        PROF("tokens_loss", 3.0 * M * W, (double)M * W * (8 + (want ? (lp_only ? 2 : h->lin.bf16 ? 6 : 4) : 0)));
        // ln_post = 0: d goes out as the stream itself.  ln_post = 1: as fp32 over the tokens in place, for ln_post's backward.
        float* d32 = !want ? nullptr : ln_post ? t : lp_only ? nullptr : h->dres;
        bf16_t* dlp = (want && !ln_post && h->lin.bf16) ? (bf16_t*)h->dres_lp : nullptr;
        if ((rc = tokens_l2_loss_grad(t, ref, B, S, W, select, reduction, d32, dlp, ln_post ? M : h->Mp, h->loss_ps, lsc, h->loss_scratch,
                                      flags, s))) return rc;
    }
    if (!want) return RVLM_OK;
    return vit_backward_tokens(h, TokSeed{ln_post ? t : nullptr, depth, ln_post}, nullptr, B, grad, s);
}
static int tokens_loop_check(const rvlm_vit* h, int B, int depth, int select, const float* ref, int reduction, const char* who) {
    int rc = tokens_check(h, B, depth, 1, who); if (rc) return rc;
    if (!ref) return fail(RVLM_ERR_ARG, std::string(who) + ": null reference tokens");
    if (select != RVLM_TOKENS_ALL && select != RVLM_TOKENS_PATCH) return fail(RVLM_ERR_ARG, std::string(who) + ": unknown select");
    if (reduction != RVLM_RED_MEAN && reduction != RVLM_RED_NONE) return fail(RVLM_ERR_ARG, std::string(who) + ": unknown reduction");
    if (tokens_l2_scratch_floats(B, h->S) > h->loss_scratch_floats) return fail(RVLM_ERR_UNSUPPORTED, std::string(who) + ": sequence too long for the loss scratch");
    return RVLM_OK;
}

extern "C" int rvlm_vit_tokens_fwd_inputgrad(rvlm_vit* h, const float* x, const float* delta, int B, int depth, int ln_post, int select,
                                             const float* ref_tokens, int reduction, float* out_tokens, float* out_loss_per_sample,
                                             float* out_loss_scalar, float* out_grad_x, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x, "rvlm_vit_tokens_fwd_inputgrad: null argument");
    int rc = tokens_loop_check(h, B, depth, select, ref_tokens, reduction, "rvlm_vit_tokens_fwd_inputgrad"); if (rc) return rc;
    if (ln_post && (rc = tok_ensure(h, true))) return rc;
    hipStream_t s = (hipStream_t)stream;
    if ((rc = tokens_step(h, x, delta, B, depth, ln_post != 0, select, ref_tokens, reduction, out_tokens,
                          out_loss_scalar ? h->loss_scalar : nullptr, nullptr, out_grad_x, s))) return rc;
    if (out_loss_per_sample) RVLM_HIP(hipMemcpyAsync(out_loss_per_sample, h->loss_ps, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (out_loss_scalar) RVLM_HIP(hipMemcpyAsync(out_loss_scalar, h->loss_scalar, 4, hipMemcpyDeviceToDevice, s));
    return RVLM_OK;
}

struct TokenStep {
    rvlm_vit* h; int depth, ln_post, select; const float* ref; int reduction; int32_t* flags;
    int operator()(int, const float* x, const float* delta, int B, float* lsc, float* grad, hipStream_t s) const {
        return tokens_step(h, x, delta, B, depth, ln_post, select, ref, reduction, nullptr, lsc, flags, grad, s);
    }
};

extern "C" int rvlm_pgd_run_tokens(rvlm_vit* h, const float* x, const float* delta0, int B, int depth, int ln_post, int select,
                                   const float* ref_tokens, int reduction, int norm_kind, float eps, int iterations, float stepsize,
                                   float momentum, int mode_max, float* x_adv_out, float* loss_trace, int32_t* flags,
                                   rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x && x_adv_out, "rvlm_pgd_run_tokens: null argument");
    int rc = pgd_loop_check("rvlm_pgd_run_tokens", norm_kind, iterations, 0, B, nullptr); if (rc) return rc;      // (batch: tokens_loop_check)
    rc = tokens_loop_check(h, B, depth, select, ref_tokens, reduction, "rvlm_pgd_run_tokens"); if (rc) return rc;
    if (ln_post && (rc = tok_ensure(h, true))) return rc;
    return pgd_run_impl(h, TokenStep{h, depth, ln_post != 0, select, ref_tokens, reduction, flags}, x, delta0, B, norm_kind, eps,
                        iterations, stepsize, momentum, mode_max, x_adv_out, loss_trace, flags, (hipStream_t)stream);
}

// apgd (vlm_eval/attacks/apgd.py:163-368; L-inf and L2, mask = None, maximising) on the per-image token loss, every image of the batch
// on its own: the loop of rvlm_apgd_run_norm below with the token step as the model and no classifier - `pred` is zero for every
// image, as rvlm_apgd_masked_bookkeeping has it, so x_best_adv follows the last iterate (apgd.py:310).  Only the schedule (k,
// size_decr, n_iter_min, counter3: data-independent) lives on the host; nothing is read back and nothing allocated.
// Buffers: img_buf[0] x_adv, [1] x_adv_old, [2] x_best_adv, [3] grad, [4] grad_best; x_best is kept in the caller's x_best_out.
extern "C" int rvlm_apgd_run_tokens(rvlm_vit* h, const float* x, const float* x_init, int B, int depth, int ln_post, int select,
                                    const float* ref_tokens, int norm_kind, float eps, int n_iter, float step0, float rho,
                                    float* x_best_out, float* loss_best_out, float* x_last_out, float* loss_trace_out,
                                    float* step_out, int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x && x_best_out, "rvlm_apgd_run_tokens: null argument");
    if (norm_kind != 0 && norm_kind != 2) return fail(RVLM_ERR_UNSUPPORTED, "rvlm_apgd_run_tokens: norm must be L-inf (0) or L2 (2)");
    RVLM_REQUIRE(n_iter >= 1 && n_iter <= 1024, "rvlm_apgd_run_tokens: n_iter must be in 1..1024");
    RVLM_REQUIRE(rho == rho, "rvlm_apgd_run_tokens: rho is NaN");
    int rc = tokens_loop_check(h, B, depth, select, ref_tokens, RVLM_RED_NONE, "rvlm_apgd_run_tokens"); if (rc) return rc;
    if (ln_post && (rc = tok_ensure(h, true))) return rc;
    hipStream_t s = (hipStream_t)stream;
    const size_t npix = (size_t)3 * h->in_h * h->in_w, n = npix * B;
    float *x_adv = h->img_buf[0], *x_adv_old = h->img_buf[1], *x_best_adv = h->img_buf[2], *grad = h->img_buf[3],
          *grad_best = h->img_buf[4], *x_best = x_best_out;
    // schedule (apgd.py:192-213)
    int k = std::max((int)(0.22 * n_iter), 1);
    const int n_iter_min = std::max((int)(0.06 * n_iter), 1), size_decr = std::max((int)(0.03 * n_iter), 1);
    int counter3 = 0;
    hipLaunchKernelGGL(clamp01_kernel, dim3(ew_blocks(n)), dim3(256), 0, s, x_init ? x_init : x, x_adv, n);
    RVLM_CHECK_LAUNCH();
    RVLM_HIP(hipMemcpyAsync(x_best, x_adv, n * 4, hipMemcpyDeviceToDevice, s));
    RVLM_HIP(hipMemcpyAsync(x_best_adv, x_adv, n * 4, hipMemcpyDeviceToDevice, s));
    RVLM_HIP(hipMemcpyAsync(x_adv_old, x_adv, n * 4, hipMemcpyDeviceToDevice, s));
    RVLM_HIP(hipMemsetAsync(h->ap_loss_steps, 0, (size_t)n_iter * B * 4, s));
    RVLM_HIP(hipMemsetAsync(h->ap_pred, 0, (size_t)B, s));          // no classifier: never "classified correctly"

    auto eval = [&](bool need_grad) -> int {     // per-image loss into loss_ps; its seed 2 (t - ref) carries no 1 / B
        return tokens_step(h, x_adv, nullptr, B, depth, ln_post != 0, select, ref_tokens, RVLM_RED_NONE, nullptr, nullptr, flags,
                           need_grad ? grad : nullptr, s);
    };
    if ((rc = eval(true))) return rc;
    RVLM_HIP(hipMemcpyAsync(grad_best, grad, n * 4, hipMemcpyDeviceToDevice, s));
    if (loss_trace_out) RVLM_HIP(hipMemcpyAsync(loss_trace_out, h->loss_ps, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(init_apgd_state_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, B, h->loss_ps, h->ap_pred, step0,
                       h->ap_loss_best, h->ap_loss_best_lc, h->ap_reduced_lc, h->ap_step, h->ap_acc);
    RVLM_CHECK_LAUNCH();
    for (int i = 0; i < n_iter; ++i) {
        {
            PROF("linf_update", 0, (double)n * 24);
            if ((rc = apgd_step_pooled(norm_kind, x, x_adv, x_adv_old, grad, h->ap_step, i > 0 ? 0.75f : 1.0f, eps, npix, B, flags, s)))
                return rc;
        }
        if ((rc = eval(i < n_iter - 1))) return rc;                 // apgd.py:300-304: the last iteration keeps the gradient it has
        counter3 += 1;
        const int do_check = counter3 == k;
        if ((rc = rvlm_apgd_controller_rho(i, B, n_iter, k, do_check, rho, h->loss_ps, h->ap_pred, h->ap_loss_steps, h->ap_loss_best,
                                           h->ap_loss_best_lc, h->ap_reduced_lc, h->ap_step, h->ap_acc, h->ap_f0, h->ap_f1, h->ap_f2,
                                           s))) return rc;
        {
            PROF("linf_update", 0, (double)n * 8);
            if ((rc = rvlm_apgd_select(x_adv, grad, x_best, grad_best, x_best_adv, h->ap_f0, h->ap_f1, h->ap_f2, npix, B, s))) return rc;
        }
        if (do_check) { counter3 = 0; k = std::max(k - size_decr, n_iter_min); }
    }
    if (loss_best_out) RVLM_HIP(hipMemcpyAsync(loss_best_out, h->ap_loss_best, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (x_last_out) RVLM_HIP(hipMemcpyAsync(x_last_out, x_best_adv, n * 4, hipMemcpyDeviceToDevice, s));
    if (loss_trace_out)
        RVLM_HIP(hipMemcpyAsync(loss_trace_out + B, h->ap_loss_steps, (size_t)n_iter * B * 4, hipMemcpyDeviceToDevice, s));
    if (step_out) RVLM_HIP(hipMemcpyAsync(step_out, h->ap_step, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    return RVLM_OK;
}

extern "C" int rvlm_pgd_run(rvlm_vit* h, const float* x, const float* delta0, int B,
                            const rvlm_loss_spec* loss, float eps, int iterations, float stepsize,
                            float momentum, int mode_max, float* x_adv_out, float* loss_trace,
                            int32_t* flags, rvlm_stream_t stream) {
    return rvlm_pgd_run_norm(h, x, delta0, B, loss, 0, eps, iterations, stepsize, momentum, mode_max, x_adv_out,
                             loss_trace, flags, stream);
}

extern "C" int rvlm_apgd_run_norm(rvlm_vit* h, const float* x, const float* x_init, int B,
                                  const rvlm_loss_spec* loss, int norm_kind, float eps, int n_iter, float step0,
                                  int train_variant, int logits_from_head, float* x_best_adv, float* x_best_out,
                                  float* loss_best_out, uint8_t* acc_out, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x && loss && loss->ref && loss->targets, "rvlm_apgd_run: null argument");
    if (norm_kind != 0 && norm_kind != 2) return fail(RVLM_ERR_UNSUPPORTED, "rvlm_apgd_run: norm must be L-inf (0) or L2 (2)");
    RVLM_REQUIRE(x_best_adv, "rvlm_apgd_run: x_best_adv output required");
    RVLM_REQUIRE(B > 1 && B <= h->maxB, "rvlm_apgd_run: need 1 < B <= max_batch");
    RVLM_REQUIRE(n_iter >= 1 && n_iter <= 1024, "rvlm_apgd_run: n_iter must be in 1..1024");
    RVLM_REQUIRE(!logits_from_head || loss->loss_kind != RVLM_LOSS_L2, "rvlm_apgd_run: head logits need a head loss (ce / dlr)");
    RVLM_REQUIRE(loss->loss_kind == RVLM_LOSS_L2 || loss->loss_kind == RVLM_LOSS_CE || logits_from_head,
                 "rvlm_apgd_run: the DLR losses run on the classification head (logits_from_head = 1)");
    hipStream_t s = (hipStream_t)stream;
    const size_t npix = (size_t)3 * h->in_h * h->in_w, n = npix * B;
    float *x_adv = h->img_buf[0], *x_adv_old = h->img_buf[1], *x_best = h->img_buf[2], *grad = h->img_buf[3],
          *grad_best = h->img_buf[4];
    int rc;
    // schedule (apgd_train.py:153-156)
    int k = std::max((int)(0.22 * n_iter), 1);
    const int n_iter_min = std::max((int)(0.06 * n_iter), 1), size_decr = std::max((int)(0.03 * n_iter), 1);
    int counter3 = 0;
    hipLaunchKernelGGL(clamp01_kernel, dim3(ew_blocks(n)), dim3(256), 0, s, x_init ? x_init : x, x_adv, n);
    RVLM_CHECK_LAUNCH();
    RVLM_HIP(hipMemcpyAsync(x_best, x_adv, n * 4, hipMemcpyDeviceToDevice, s));
    RVLM_HIP(hipMemcpyAsync(x_best_adv, x_adv, n * 4, hipMemcpyDeviceToDevice, s));
    RVLM_HIP(hipMemcpyAsync(x_adv_old, x_adv, n * 4, hipMemcpyDeviceToDevice, s));
    RVLM_HIP(hipMemsetAsync(h->ap_loss_steps, 0, (size_t)n_iter * B * 4, s));

    auto eval = [&](bool need_grad) -> int {
        int r;
        if ((r = vit_forward(h, x_adv, nullptr, B, loss->output_normalize, need_grad ? 1 : 0, h->emb, s))) return r;
        if ((r = loss_step(h, loss, B, RVLM_RED_NONE, nullptr, logits_from_head ? h->ap_pred : nullptr, s))) return r;
        if (!logits_from_head) {   // apgd_train.py:192,301: argmax over the model output (the embedding)
            if ((r = rvlm_argmax_eq(h->emb, loss->targets, B, h->D, h->ap_pred, s))) return r;
        }
        if (need_grad) { if ((r = vit_backward(h, h->d_emb, B, grad, s))) return r; }
        return RVLM_OK;
    };
    if ((rc = eval(true))) return rc;
    RVLM_HIP(hipMemcpyAsync(grad_best, grad, n * 4, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(init_apgd_state_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, B, h->loss_ps, h->ap_pred, step0,
                       h->ap_loss_best, h->ap_loss_best_lc, h->ap_reduced_lc, h->ap_step, h->ap_acc);
    RVLM_CHECK_LAUNCH();
    for (int i = 0; i < n_iter; ++i) {
        const float a = i > 0 ? 0.75f : 1.0f;
        {
            PROF("linf_update", 0, (double)n * 24);
            rc = norm_kind == 2 ? rvlm_apgd_l2_step(x, x_adv, x_adv_old, grad, h->ap_step, a, eps, npix, B, s)
                                : rvlm_apgd_linf_step(x, x_adv, x_adv_old, grad, h->ap_step, a, eps, npix, B, s);
            if (rc) return rc;
        }
        const bool need_grad = !(train_variant && i == n_iter - 1);   // apgd_train.py:293-295
        if ((rc = eval(need_grad))) return rc;
        counter3 += 1;
        const int do_check = counter3 == k;
        // apgd_train hard-codes the threshold (train/apgd_train.py:117,334: k3 = 0.75); `rho` is APGDAttack's parameter only, so
        // a value left on the handle by an APGDAttack(rho != 0.75) run does not reach a later apgd_train on the same handle
        if ((rc = rvlm_apgd_controller_rho(i, B, n_iter, k, do_check, train_variant ? 0.75 : h->ap_rho, h->loss_ps, h->ap_pred, h->ap_loss_steps,
                                       h->ap_loss_best, h->ap_loss_best_lc, h->ap_reduced_lc, h->ap_step,
                                       h->ap_acc, h->ap_f0, h->ap_f1, h->ap_f2, s))) return rc;
        {
            PROF("linf_update", 0, (double)n * 8);
            if ((rc = rvlm_apgd_select(x_adv, grad, x_best, grad_best, x_best_adv, h->ap_f0, h->ap_f1, h->ap_f2,
                                       npix, B, s))) return rc;
        }
        if (do_check) { counter3 = 0; k = std::max(k - size_decr, n_iter_min); }
    }
    if (x_best_out) RVLM_HIP(hipMemcpyAsync(x_best_out, x_best, n * 4, hipMemcpyDeviceToDevice, s));
    if (loss_best_out) RVLM_HIP(hipMemcpyAsync(loss_best_out, h->ap_loss_best, (size_t)B * 4, hipMemcpyDeviceToDevice, s));
    if (acc_out) RVLM_HIP(hipMemcpyAsync(acc_out, h->ap_acc, (size_t)B, hipMemcpyDeviceToDevice, s));
    return RVLM_OK;
}

extern "C" int rvlm_apgd_run(rvlm_vit* h, const float* x, const float* x_init, int B,
                             const rvlm_loss_spec* loss, float eps, int n_iter, float step0,
                             int train_variant, int logits_from_head, float* x_best_adv, float* x_best_out,
                             float* loss_best_out, uint8_t* acc_out, rvlm_stream_t stream) {
    return rvlm_apgd_run_norm(h, x, x_init, B, loss, 0, eps, n_iter, step0, train_variant, logits_from_head, x_best_adv,
                              x_best_out, loss_best_out, acc_out, stream);
}
