// Workspace plan and life cycle of the ViT engine (engine_internal.h): weight conversion, create / destroy, the input size and the
// other per-handle switches, and the profiling entries.
#include <algorithm>

#include "engine_internal.h"

namespace rvlm {

// ---- weights --------------------------------------------------------------------------------
// nk: [rows, cols] bf16 (ld = cols_pad) ; t: [cols, rows] bf16
static int conv_w(rvlm_vit* h, bf16_t** nk, bf16_t** t, const float* src, int rows, int cols, int cols_pad,
                  hipStream_t s, bool alloc) {
    if (!src) return fail(RVLM_ERR_ARG, "rvlm_vit: null weight pointer");
    if (alloc) {
        int rc = dev_alloc(h->arena, (void**)nk, (size_t)rows * cols_pad * 2); if (rc) return rc;
        rc = dev_alloc(h->arena, (void**)t, (size_t)cols_pad * rows * 2); if (rc) return rc;
    }
    if (convert_f32_to_bf16_pair(src, cols, *nk, cols_pad, *t, rows, rows, cols, s)) { RVLM_CHECK_LAUNCH(); return RVLM_OK; }
    int rc = convert_f32_to_bf16(src, cols, *nk, cols_pad, rows, cols, 0, s); if (rc) return rc;
    return convert_f32_to_bf16(src, cols, *t, rows, rows, cols, 1, s);
}

int load_weights(rvlm_vit* h, const rvlm_vit_weights* w, hipStream_t s, bool alloc) {
    const int W = h->W, L = h->L;
    int rc;
#define CP(dst, src, n) if ((rc = copy_f32(h->arena, &(dst), (src), (n), s, alloc, "rvlm_vit"))) return rc
    CP(h->cls, w->class_embedding, W);
    CP(h->pos, w->positional_embedding, (size_t)h->S * W);
    CP(h->proj, w->proj, (size_t)W * h->D);
    CP(h->lnpre_w, w->ln_pre_weight, W); CP(h->lnpre_b, w->ln_pre_bias, W);
    CP(h->lnpost_w, w->ln_post_weight, W); CP(h->lnpost_b, w->ln_post_bias, W);
    if (h->lin.bf16) {
        if ((rc = conv_w(h, &h->conv_nk, &h->conv_t, w->conv1_weight, W, h->Kp, h->Kpad, s, alloc))) return rc;
    } else {
        CP(h->conv_f32, w->conv1_weight, (size_t)W * h->Kp);
    }
    if (!w->blocks_host) return fail(RVLM_ERR_ARG, "rvlm_vit: blocks_host is null");
    for (int l = 0; l < L; ++l) {
        const rvlm_vit_block_weights& b = w->blocks_host[l];
        Layer& y = h->layers[l];
        if ((rc = load_block_vectors(h->arena, y, b, W, s, alloc, "rvlm_vit"))) return rc;
        for (auto& q : block_weights(y, b, W)) {
            if (h->lin.bf16) {
                if ((rc = conv_w(h, q.nk, q.t, q.src, q.rows, q.cols, q.cols, s, alloc))) return rc;
            } else {
                CP(*q.f32, q.src, (size_t)q.rows * q.cols);
                if (h->lin.x3) {      // [W_hi | W_lo | W_hi] and the same of W^T
                    if (alloc) {
                        if ((rc = dev_alloc(h->arena, (void**)q.nk, (size_t)q.rows * q.cols * 6, false))) return rc;
                        if ((rc = dev_alloc(h->arena, (void**)q.t, (size_t)q.rows * q.cols * 6, false))) return rc;
                    }
                    if ((rc = x3_prepare_weight(q.src, q.rows, q.cols, *q.nk, *q.t, s))) return rc;
                }
            }
        }
    }
#undef CP
    return RVLM_OK;
}

}  // namespace rvlm

// ---- C ABI: life cycle, switches, profiling -------------------------------------------------------------------------------
extern "C" int rvlm_vit_create(const rvlm_vit_config* cfg, const rvlm_vit_weights* weights,
                               rvlm_stream_t stream, rvlm_vit** out) {
    RVLM_REQUIRE(cfg && weights && out, "rvlm_vit_create: null argument");
    RVLM_REQUIRE(cfg->patch > 0 && cfg->image_size % cfg->patch == 0, "rvlm_vit_create: image_size % patch");
    RVLM_REQUIRE(cfg->heads > 0 && cfg->width == cfg->heads * 64, "rvlm_vit_create: head_dim must be 64");
    RVLM_REQUIRE(cfg->layers > 0 && cfg->out_dim > 0 && cfg->max_batch > 0, "rvlm_vit_create: sizes");
    RVLM_REQUIRE(cfg->precision == RVLM_PREC_F32 || cfg->precision == RVLM_PREC_BF16 || cfg->precision == RVLM_PREC_F32X3,
                 "rvlm_vit_create: precision");
    RVLM_REQUIRE(cfg->precision != RVLM_PREC_F32X3 || cfg->trainable <= 0, "rvlm_vit_create: the split-bf16 mode is an attack / inference "
                 "precision (no weight gradients)");
    RVLM_REQUIRE(cfg->act == RVLM_ACT_QUICK_GELU || cfg->act == RVLM_ACT_GELU, "rvlm_vit_create: act");
    RVLM_REQUIRE(cfg->width <= 2048, "rvlm_vit_create: width > 2048 unsupported");
    if (cfg->precision == RVLM_PREC_BF16) {      // the bf16 flash kernels' sequence limits (kernels.h), here instead of at the first step
        const long g = cfg->image_size / cfg->patch, seq = g * g + 1;
        if (seq > ATTN_BF16_MAX_S_FWD || (cfg->trainable >= 0 && seq > ATTN_BF16_MAX_S_BWD))
            return fail(RVLM_ERR_UNSUPPORTED, "rvlm_vit_create: bf16 attention takes at most 640 tokens (608 with a backward)");
    }
    hipStream_t s = (hipStream_t)stream;
    rvlm_vit* h = new rvlm_vit();
    static unsigned long long next_uid = 0;
    h->uid = __atomic_add_fetch(&next_uid, 1, __ATOMIC_RELAXED);
    h->cfg = *cfg;
    h->lin.bf16 = cfg->precision == RVLM_PREC_BF16;
    h->lin.x3 = cfg->precision == RVLM_PREC_F32X3;
    h->lin.act = cfg->act;
    h->esz = h->lin.bf16 ? 2 : 4;
    h->img = h->in_h = h->in_w = cfg->image_size; h->P = cfg->patch; h->G = h->img / h->P; h->S = h->G * h->G + 1;
    h->W = cfg->width; h->L = cfg->layers; h->H = cfg->heads; h->D = cfg->out_dim;
    h->Kp = 3 * h->P * h->P; h->Kpad = (int)round_up(h->Kp, 64);
    h->maxB = cfg->max_batch;
    h->Mp = (int)round_up((long)h->maxB * h->S, 256);
    h->Mp0 = (int)round_up((long)h->maxB * h->G * h->G, 256);
    h->layers.resize(h->L);
    const int W = h->W, L = h->L, S = h->S, B = h->maxB, D = h->D;
    const size_t Mp = h->Mp, Mp0 = h->Mp0, e = h->esz;
    auto body = [&]() -> int {
        int rc = load_weights(h, weights, s, true);
        if (rc) return rc;
        ALLOC(h->A0, Mp0 * h->Kpad * e);
        ALLOC(h->patch_out, Mp0 * W * 4);
        if (h->lin.x3 && W % 256 == 0) {      // split copy of a linear's input: up to [Mp, 3 * 4W] bf16 (0.8 GB for ViT-L/14 at B = 128)
            if ((rc = dev_alloc(h->arena, (void**)&h->lin.a3, Mp * 12 * W * 2, false))) return rc;
        }
        // RVLM_DRES_FP32=1: the fp32 residual-gradient stream in every backward (rounds 1-5)
        h->lp_dres = h->lin.bf16 && env_int("RVLM_DRES_FP32", 0) == 0;
        // RVLM_F32_FLASH=0: the batched attention path over kept probabilities (A/B and parity arm)
        h->own_flash = !h->lin.bf16 && attn_bwd_f32_flash_covers(S) && env_int("RVLM_F32_FLASH", 1) != 0;
        // (a provider needs the flash forward for its sequence length: otherwise the handoff exports from per-block fp32 tensors)
        const bool provider = cfg->trainable == -2 && !h->lin.bf16 && attn_fwd_f32_flash_covers(S);
        h->provider = provider;
        const bool inference_only = cfg->trainable < 0 && !(cfg->trainable == -2 && !h->lin.bf16);   // no backward of any kind: one slot per buffer kind
        h->inference_only = inference_only;
        h->xs.resize(2 * L + 1);
        for (size_t i = 0; i < h->xs.size(); ++i) {
            if (inference_only && i > 0) { h->xs[i] = h->xs[0]; continue; }
            ALLOC(h->xs[i], Mp * W * 4);
        }
        ALLOC(h->st_mean, (size_t)(2 * L + 2) * Mp * 4);
        ALLOC(h->st_rstd, (size_t)(2 * L + 2) * Mp * 4);
        ALLOC(h->ln_out, Mp * W * e);
        h->qkv.resize(L); h->attn_o.resize(L); h->lse.resize(L); h->h_pre.resize(L);
        const size_t Sp = round_up(S, 32);
        for (int l = 0; l < L; ++l) {
            if ((inference_only || provider) && l > 0) {
                h->qkv[l] = h->qkv[0]; h->attn_o[l] = h->attn_o[0]; h->lse[l] = h->lse[0]; h->h_pre[l] = h->h_pre[0];
                if (provider) { h->lse2.resize(L); ALLOC(h->lse2[l], (size_t)B * h->H * Sp * 4); }
                continue;
            }
            ALLOC(h->qkv[l], Mp * 3 * W * e);
            ALLOC(h->attn_o[l], Mp * W * e);
            // bf16: log-sum-exp rows of the flash kernels; fp32: the block's probabilities [B, H, S, round_up(S, 4)], zero pad columns - a
            // stub where the fp32 flash kernels run both directions (own_flash: nothing is kept)
            ALLOC(h->lse[l], h->lin.bf16 ? (size_t)B * h->H * Sp * 4 : h->own_flash ? 256 : (size_t)B * h->H * S * round_up(S, 4) * 4);
            ALLOC(h->h_pre[l], Mp * 4 * W * e);
            if (!h->lin.bf16 && !inference_only) {      // (2.4 MB per block at ViT-L/14, B = 128)
                h->lse2.resize(L);
                ALLOC(h->lse2[l], (size_t)B * h->H * Sp * 4);
            }
        }
        ALLOC(h->g_act, Mp * 4 * W * e);
        ALLOC(h->pooled, (size_t)B * W * 4);
        ALLOC(h->emb_raw, (size_t)B * D * 4);
        ALLOC(h->inv_norm, (size_t)B * 4);
        const size_t bs = provider ? 0 : 1;      // (a provider runs no backward: 256-byte stubs)
        ALLOC(h->dres, bs * Mp * W * 4);
        ALLOC(h->dres_lp, bs * Mp * W * e);
        ALLOC(h->d_o, bs * Mp * W * e);
        ALLOC(h->dqkv, bs * Mp * 3 * W * e);
        ALLOC(h->dh, bs * Mp * 4 * W * e);
        ALLOC(h->d_ln, bs * Mp * W * e);
        ALLOC(h->d_patch, bs * Mp0 * W * e);
        ALLOC(h->dA0, bs * Mp0 * h->Kpad * 4);
        ALLOC(h->dsum, (size_t)B * h->H * Sp * 4);
        ALLOC(h->d_raw, (size_t)B * D * 4);
        ALLOC(h->d_pooled, (size_t)B * W * 4);
        if (!h->lin.bf16) {
            // [B, H, S, round_up(S, 4)], zero-initialised: the pad columns are never written
            ALLOC(h->dscores, (h->own_flash ? 0 : bs) * (size_t)B * h->H * S * round_up(S, 4) * 4);
        } else { h->dscores = nullptr; }
        h->trainable = cfg->trainable > 0;
        h->tokens = h->dtok = nullptr; h->tA = h->tB = nullptr;
        h->cls_tail = h->lin.bf16 && env_int("RVLM_CLS_TAIL", 1) != 0;    // RVLM_CLS_TAIL=0: the last block on every row like the other blocks
        if (h->cls_tail) ALLOC(h->lse_cls, (size_t)B * h->H * 4);
        if (h->trainable) {
            h->ln1_out.resize(L); h->ln2_out.resize(L); h->g_act_l.resize(L);
            for (int l = 0; l < L; ++l) {
                ALLOC(h->ln1_out[l], Mp * W * e);
                ALLOC(h->ln2_out[l], Mp * W * e);
                ALLOC(h->g_act_l[l], Mp * 4 * W * e);
            }
            ALLOC(h->tokens, Mp * W * 4);
            ALLOC(h->dtok, Mp * W * 4);
            if (h->lin.bf16) {
                // What the copy-free contraction-major weight gradient leaves to these buffers: conv1 (max(W, Kpad) rows x all tokens),
                // and every linear when fewer than 256 tokens are in flight (4W rows x < 320 columns, short leading dimension).
                // Widths that are no multiple of 256 transpose every linear:
                // 4W rows x all tokens (0.57 GB for ViT-L/14 at B = 128).
                h->Mpt = (long)Mp + 16 * 128;
                const bool every_linear = W % 256 != 0;
                const size_t rows = (size_t)(every_linear ? std::max(4 * W, h->Kpad) : std::max(W, h->Kpad));
                h->t_elems = std::max(rows * (size_t)h->Mpt, (size_t)std::max(4 * W, h->Kpad) * 320);
                ALLOC(h->tA, h->t_elems * 2);
                ALLOC(h->tB, h->t_elems * 2);
            }
        }
        {
            // split-K slabs: 8 x <=256 rows x 4W columns for the few-row GEMMs; trainable handles also run
            // the weight-gradient GEMMs split-K (few output tiles, K = all tokens): up to 3 x [3W, W] slabs
            size_t sk = (size_t)8 * 256 * 4 * W * sizeof(float);
            // (sized from the plan itself - ADVICE r5: 16 W^2 floats cover W = 1024 exactly but not W = 768, whose QKV plan wants 9
            // slabs of [3W, W]; those shapes then fell to the transposing path, whose scratch the copy-free sizing no longer covers)
            if (cfg->trainable > 0)
                sk = std::max({sk, wgrad_slab_bytes(3 * W, W), wgrad_slab_bytes(W, W), wgrad_slab_bytes(4 * W, W), wgrad_slab_bytes(W, 4 * W)});
            ALLOC(h->lin.splitk, sk);
            h->lin.splitk_bytes = sk;
            if (cfg->trainable > 0) {
                // partial column sums: [2][RED_NCH][4W] (LayerNorm affine) or one row per 64-token tile of a transpose
                const size_t rf = std::max((size_t)2 * 128 * 4 * W, (size_t)((Mp + 16 * 128) / 64) * 4 * W);
                ALLOC(h->red_scratch, rf * sizeof(float));
                h->red_floats = rf;
            }
        }
        const size_t npix = (size_t)B * 3 * h->img * h->img;
        for (int i = 0; i < 5; ++i) ALLOC(h->img_buf[i], npix * 4);
        ALLOC(h->emb, (size_t)B * D * 4);
        ALLOC(h->d_emb, (size_t)B * D * 4);
        ALLOC(h->loss_ps, (size_t)B * 4);
        ALLOC(h->loss_scalar, 4096 * 4);
        h->loss_scratch_floats = (size_t)B * 1024 + (size_t)D * 1024;   // CE head with up to 1024 classes
        ALLOC(h->loss_scratch, h->loss_scratch_floats * 4);
        ALLOC(h->ap_loss_steps, (size_t)1024 * B * 4);
        ALLOC(h->ap_loss_best, (size_t)B * 4);
        ALLOC(h->ap_loss_best_lc, (size_t)B * 4);
        ALLOC(h->ap_reduced_lc, (size_t)B * 4);
        ALLOC(h->ap_step, (size_t)B * 4);
        ALLOC(h->ap_acc, B); ALLOC(h->ap_pred, B);
        ALLOC(h->ap_f0, B); ALLOC(h->ap_f1, B); ALLOC(h->ap_f2, B);
        hipError_t he = hipStreamSynchronize(s);
        if (he != hipSuccess) return fail(RVLM_ERR_HIP, std::string("create sync: ") + hipGetErrorString(he));
        return RVLM_OK;
    };
    const int rc = body();
    if (rc) {      // (one destroy on any failure; it must not cost the caller the message)
        const std::string msg = rvlm_last_error();
        rvlm_vit_destroy(h);
        return fail(rc, msg);
    }
    *out = h;
    return RVLM_OK;
}

extern "C" int rvlm_vit_destroy(rvlm_vit* h) {
    if (!h) return RVLM_OK;
    (void)hipDeviceSynchronize();
    for (auto& r : h->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (void* p : h->arena.allocs) (void)hipFree(p);
    delete h;
    return RVLM_OK;
}

extern "C" int rvlm_vit_load_weights(rvlm_vit* h, const rvlm_vit_weights* weights, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && weights, "rvlm_vit_load_weights: null argument");
    return load_weights(h, weights, (hipStream_t)stream, false);
}

extern "C" size_t rvlm_vit_workspace_bytes(const rvlm_vit* h) { return h ? h->arena.bytes : 0; }

extern "C" int rvlm_vit_set_input_size(rvlm_vit* h, int in_h, int in_w) {
    RVLM_REQUIRE(h, "rvlm_vit_set_input_size: null handle");
    if (in_h == 0 && in_w == 0) in_h = in_w = h->img;
    RVLM_REQUIRE(in_h >= 1 && in_w >= 1, "rvlm_vit_set_input_size: sizes must be positive ((0, 0) = the model's own)");
    if (in_h > h->img || in_w > h->img)
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_vit_set_input_size: inputs larger than image_size (down-sampling inside the engine)");
    const bool resize = in_h != h->img || in_w != h->img;
    if (resize && h->trainable)
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_vit_set_input_size: a trainable handle runs at the model's own resolution only");
    if (in_h == h->in_h && in_w == h->in_w) return RVLM_OK;
    ResizeAxis ah, aw;
    if (resize) {
        int rc;
        if ((rc = resize_axis_device(in_h, h->img, &ah))) return rc;
        if ((rc = resize_axis_device(in_w, h->img, &aw))) return rc;
    }
    h->rs_h = ah; h->rs_w = aw;
    h->in_h = in_h; h->in_w = in_w; h->resize = resize;
    h->saved_B = 0;      // a forward saved at another geometry is not this size's to differentiate
    return RVLM_OK;
}

extern "C" int rvlm_vit_set_flash_inference(rvlm_vit* h, int on) {
    RVLM_REQUIRE(h, "rvlm_vit_set_flash_inference: null handle");
    h->flash_inference = on != 0 && !h->lin.bf16;
    return RVLM_OK;
}

extern "C" int rvlm_vit_set_apgd_rho(rvlm_vit* h, double rho) {
    RVLM_REQUIRE(h && rho == rho, "rvlm_vit_set_apgd_rho: null handle or NaN");
    h->ap_rho = rho;
    return RVLM_OK;
}

extern "C" int rvlm_vit_set_profiling(rvlm_vit* h, int enabled) {
    RVLM_REQUIRE(h, "rvlm_vit_set_profiling: null handle");
    h->prof = enabled != 0;
    return RVLM_OK;
}
extern "C" int rvlm_vit_reset_profile(rvlm_vit* h) {
    RVLM_REQUIRE(h, "rvlm_vit_reset_profile: null handle");
    (void)hipDeviceSynchronize();
    for (auto& r : h->recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    h->recs.clear();
    for (auto& a : h->accs) a = ProfAcc();
    return RVLM_OK;
}
extern "C" int rvlm_vit_get_profile(rvlm_vit* h, rvlm_profile_entry* out, int* n) {
    RVLM_REQUIRE(h && out && n, "rvlm_vit_get_profile: null argument");
    RVLM_HIP(hipDeviceSynchronize());
    for (auto& a : h->accs) a.ms = 0;
    for (auto& r : h->recs) {
        float ms = 0.0f;
        hipError_t e = hipEventElapsedTime(&ms, r.a, r.b);
        if (e == hipSuccess) h->accs[r.cls].ms += ms;
    }
    int cnt = 0;
    for (size_t i = 0; i < h->cls_names.size() && cnt < *n; ++i) {
        if (h->accs[i].n == 0) continue;
        rvlm_profile_entry& e = out[cnt++];
        memset(&e, 0, sizeof(e));
        strncpy(e.name, h->cls_names[i].c_str(), sizeof(e.name) - 1);
        e.total_ms = h->accs[i].ms; e.flops = h->accs[i].flops; e.bytes = h->accs[i].bytes; e.launches = h->accs[i].n;
    }
    *n = cnt;
    return RVLM_OK;
}
