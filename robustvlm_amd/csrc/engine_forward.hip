// The forward half of the ViT engine (engine_internal.h): attention forward, the block walker, and the forward entries of the C ABI.
#include "engine_internal.h"

namespace rvlm {

// ---- attention (dispatch on precision) -------------------------------------------------------
// (fp32 storage only: lse2 = the block's log-sum-exp rows or null; qkv_bf / o_bf = the peer's bf16 qkv / attention output or null)
template <typename T>
static int attention_fwd(rvlm_vit* h, hipStream_t s, const FwdPass& fp, const void* qkv, void* o, float* lse, float* lse2,
                         bf16_t* qkv_bf, bf16_t* o_bf, int B);
template <>
int attention_fwd<bf16_t>(rvlm_vit* h, hipStream_t s, const FwdPass&, const void* qkv, void* o, float* lse, float*, bf16_t*, bf16_t*,
                          int B) {
    return attn_fwd_bf16((const bf16_t*)qkv, 3 * h->W, (bf16_t*)o, h->W, lse, B, h->H, h->S, s);
}
// fp32 mode: the score matrices are materialised as [B, H, S, Sld] with Sld = round_up(S, 4) and zero pad columns (never
// written), so that every product that contracts over or runs along the key dimension of S = 257 takes 16-byte operand loads
// on the fp32 matrix-pipe tiles (GemmF32::pad4); round 5: the unaligned scalar-load form ran the attention core at 26 TFLOP/s.
// P = softmax(0.125 Q K^T) of one block into `P` ([B, H, S, Sld]): the block's slot of rvlm_vit::lse, which in fp32 mode holds
// the probabilities themselves - the backward reads them back instead of recomputing scores + softmax (round 5: 13 GB for
// ViT-L/14 at B = 128 of 288, one batched GEMM + one softmax pass less per block and backward)
static int attn_scores_f32(rvlm_vit* h, hipStream_t s, const float* qkv, float* P, float* lse2, int B) {
    const int S = h->S, W = h->W, H = h->H, Sld = (int)round_up(S, 4);
    GemmF32 g;  // scores = 0.125 * Q K^T
    g.A = qkv; g.sam = 3 * W; g.sak = 1; g.sab1 = (long)S * 3 * W; g.sab2 = 64;
    g.B = qkv + W; g.sbn = 3 * W; g.sbk = 1; g.sbb1 = (long)S * 3 * W; g.sbb2 = 64;
    g.C = P; g.scm = Sld; g.scn = 1; g.scb1 = (long)H * S * Sld; g.scb2 = (long)S * Sld;
    g.M = S; g.N = S; g.K = 64; g.nb1 = B; g.nb2 = H; g.alpha = 0.125f;
    int rc = gemm_f32(g, s); if (rc) return rc;
    return softmax_rows_fwd(P, (long)B * H * S, S, Sld, s, lse2, (int)round_up(S, 32));
}
template <>
int attention_fwd<float>(rvlm_vit* h, hipStream_t s, const FwdPass& fp, const void* qkv_, void* o, float* P, float* lse2,
                         bf16_t* qkv_bf, bf16_t* o_bf, int B) {
    const int S = h->S, W = h->W, H = h->H, Sld = (int)round_up(S, 4);
    const float* qkv = (const float*)qkv_;
    int rc = RVLM_OK;
    if (fp.flash) {      // no backward of this handle's own will read P: one fused kernel, no score matrices
        if (attn_fwd_f32_flash(qkv, (float*)o, lse2, (int)round_up(S, 32), qkv_bf, o_bf, B, H, S, s, &rc)) return rc;
        if (fp.peer || h->own_flash)      // (no fall-through: there is no probability buffer behind P on these paths)
            return fail(RVLM_ERR_UNSUPPORTED, "attention forward: sequence length not covered by the fp32 flash kernel");
    }
    rc = attn_scores_f32(h, s, qkv, P, lse2, B); if (rc) return rc;
    GemmF32 g;  // O = P V
    g.A = P; g.sam = Sld; g.sak = 1; g.sab1 = (long)H * S * Sld; g.sab2 = (long)S * Sld; g.pad4 = 1;
    g.B = qkv + 2 * W; g.sbn = 1; g.sbk = 3 * W; g.sbb1 = (long)S * 3 * W; g.sbb2 = 64;
    g.C = (float*)o; g.scm = W; g.scn = 1; g.scb1 = (long)S * W; g.scb2 = 64;
    g.M = S; g.N = 64; g.K = S; g.nb1 = B; g.nb2 = H;
    return gemm_f32(g, s);
}

// ---- QKV projection of the last block under the class-token tail: K, V for every token, Q for the class rows only
// (the other 256 query rows of that block are dead).  Forward: qkv[:, W:3W] by the big GEMM (N = 2W), then the class
// rows' Q by a B-row GEMM.  (Backward: qkv_tail_bwd, engine_backward.hip.)
static int qkv_tail_fwd(rvlm_vit* h, hipStream_t s, const void* ln1o, const Layer& y, void* qkv, int B) {
    const int S = h->S, W = h->W, M = B * S;
    GemmBf16 g;
    g.A = (const bf16_t*)ln1o; g.lda = W; g.Bw = y.w_in_nk + (size_t)W * W; g.ldb = W;
    g.M = M; g.N = 2 * W; g.K = W; g.a_rows = (int)round_up(M, 128); g.epi = EPI_BF16;
    g.bias = y.b_in + W; g.out = (bf16_t*)qkv + W; g.ldo = 3 * W; g.act = h->cfg.act;
    with_scratch(h->lin, g);
    int rc = gemm_bf16_nt(g, s);
    if (rc) return rc;
    GemmBf16 q;
    q.A = (const bf16_t*)ln1o; q.lda = (long)S * W; q.Bw = y.w_in_nk; q.ldb = W;
    q.M = B; q.N = W; q.K = W; q.a_rows = B; q.epi = EPI_BF16;
    q.bias = y.b_in; q.out = qkv; q.ldo = (long)S * 3 * W; q.act = h->cfg.act;
    with_scratch(h->lin, q);
    return gemm_bf16_nt(q, s);
}

int tok_ensure(rvlm_vit* h, bool want_buf) {
    if (!h->tok_mean) { ALLOC(h->tok_mean, (size_t)h->Mp * 4); ALLOC(h->tok_rstd, (size_t)h->Mp * 4); }
    if (want_buf && !h->tok_buf) ALLOC(h->tok_buf, (size_t)h->Mp * h->W * 4);
    return RVLM_OK;
}

// ---- forward -----------------------------------------------------------------------------------
// for_peer: the bf16 handle whose backward will read this (saving) forward - the handoff - or null
template <typename T>
static int forward_impl(rvlm_vit* h, const float* x, const float* delta, int B, int normalize, int save,
                        float* out_emb, hipStream_t s, const TokPass* tp = nullptr, rvlm_vit* for_peer = nullptr) {
    const int S = h->S, W = h->W, L = h->L, D = h->D, M = B * S, M0 = B * h->G * h->G;
    const int Lrun = tp ? tp->depth : L;            // blocks run
    const bool tail = h->cls_tail && !tp;           // a token pass needs every row of the last block
    const double attn_flops = 4.0 * B * h->H * (double)S * S * 64;
    int rc;
    // EVERY forward overwrites state a pending backward reads (the shared LayerNorm statistics of all layers, slot 0 of
    // xs / qkv / attn_o / lse, pooled, emb_raw, inv_norm): a non-saving pass therefore invalidates the saved forward
    // instead of letting a later backward run on a mixture of two passes.
    h->saved_B = 0;
    h->lin.a3_of = nullptr;      // (x3) nothing an earlier enqueue left in the split copy is this pass's operand
    // a forward FOR a peer (handoff) is a saving forward of an fp32-storage handle on the fp32 flash attention (no probabilities
    // kept: this handle's own backward is refused for that pass, Saved::ForPeer); it overwrites the peer's bf16 tensors
    // (sequence lengths the flash kernel does not take - S = 577 at 336 px - run the batched attention path as before: the handoff then
    // exports the bf16 tensors itself and takes the log-sum-exp rows the softmax pass wrote, vit_backward_from)
    const bool flash_ok = !h->lin.bf16 && attn_fwd_f32_flash_covers(h->S);
    FwdPass fp;
    fp.peer = (flash_ok && save == 1) ? for_peer : nullptr;
    fp.flash = flash_ok && (h->own_flash || fp.peer != nullptr || (save == 0 && h->flash_inference));
    rvlm_vit* const peer = fp.peer;
    if (h->provider && save != 0 && !peer)
        return fail(RVLM_ERR_STATE, "forward: this handle was created as a forward provider (trainable = -2): its saving forwards are run "
                                    "for a bf16 handle (rvlm_vit_forward_for, rvlm_pgd_run_mixed_fwd)");
    if (peer) peer->saved_B = 0;
    h->exported_to = 0; h->exported_dact = false;
    {
        PROF("patch_im2col", 0, (double)B * 3 * h->in_h * h->in_w * (delta ? 8 : 4) + (double)M0 * h->Kpad * sizeof(T));
        rc = h->resize ? resize_im2col_normalize<T>(x, delta, B, h->rs_h, h->rs_w, h->P, h->cfg.mean, h->cfg.std, (T*)h->A0, h->Kpad,
                                                    h->Kpad, s)
                       : im2col_normalize<T>(x, delta, B, h->img, h->P, h->cfg.mean, h->cfg.std, (T*)h->A0, h->Kpad, h->Kpad, s);
        if (rc) return rc;
    }
    {
        PROF("gemm_patch_fwd", 2.0 * M0 * W * h->Kp, 0);
        if (h->lin.bf16) {
            GemmBf16 g;
            g.A = (const bf16_t*)h->A0; g.lda = h->Kpad; g.Bw = h->conv_nk; g.ldb = h->Kpad;
            g.M = M0; g.N = W; g.K = h->Kpad; g.a_rows = h->Mp0; g.epi = EPI_F32; g.out = h->patch_out; g.ldo = W;
            with_scratch(h->lin, g);
            rc = gemm_bf16_nt(g, s);
        } else {
            rc = linear_fwd<float>(h->lin, s, h->A0, h->Kpad, M0, W, h->Kp, h->conv_f32, nullptr, nullptr, EPI_F32,
                                   h->patch_out, W, nullptr, nullptr);
        }
        if (rc) return rc;
    }
    auto XS = [&](int i) { return h->xs[save ? i : 0]; };
    {
        PROF("embed_lnpre_fwd", 0, (double)M * W * 8);
        if ((rc = embed_lnpre_fwd<float>(h->patch_out, W, h->cls, h->pos, h->lnpre_w, h->lnpre_b, XS(0), W,
                                         h->mean_at(0), h->rstd_at(0), B, S, W, s,
                                         save == 2 ? h->tokens : nullptr))) return rc;
    }
    for (int l = 0; l < Lrun; ++l) {
        Layer& y = h->layers[l];
        const int sl = save ? l : 0;
        float* x_in = XS(2 * l); float* x_mid = XS(2 * l + 1); float* x_out = XS(2 * l + 2);
        void* ln1o = save == 2 ? h->ln1_out[l] : h->ln_out;     // linear inputs are kept only for wgrad
        void* ln2o = save == 2 ? h->ln2_out[l] : h->ln_out;
        void* gact = save == 2 ? h->g_act_l[l] : h->g_act;
        // The class-token tail is this block with (a) the steps after the attention on the class rows, (b) Q for the class rows only,
        // (c) the class query's attention, (e) no LayerNorm-into-split (the tail is bf16 only); its few-row launches are accounted as
        // two coarse profile classes (tail_attn_fwd, tail_mlp_fwd) instead of one per step.
        const bool tl = tail && l == L - 1;
        const Rows r = tl ? Rows{B, (long)S * W, B} : Rows{M, (long)W, 0};      // (a)
        {
            PROF("layernorm_fwd", 0, (double)M * W * (4 + sizeof(T)));
            if (ln_into_split(h->lin, s, x_in, y.ln1_w, y.ln1_b, ln1o, h->mean_at(1 + 2 * l), h->rstd_at(1 + 2 * l), M, 3 * W, W, &rc)) { if (rc) return rc; }
            else
            if ((rc = layernorm_fwd<T>(x_in, W, y.ln1_w, y.ln1_b, (T*)ln1o, W, h->mean_at(1 + 2 * l),
                                       h->rstd_at(1 + 2 * l), M, W, s))) return rc;
        }
        {
            PROF("gemm_qkv_fwd", tl ? 2.0 * M * W * 2 * W + 2.0 * B * W * W : 2.0 * M * W * 3 * W, 0);
            rc = tl ? qkv_tail_fwd(h, s, ln1o, y, h->qkv[sl], B)      // (b)
                    : linear_fwd<T>(h->lin, s, ln1o, W, M, 3 * W, W, y.w_in, y.w_in_nk, y.b_in, EPI_BF16, h->qkv[sl], 3 * W, nullptr, nullptr);
            if (rc) return rc;
        }
        if (tl) {      // (c)
            PROF("tail_attn_fwd", 4.0 * B * h->H * (double)S * 64, (double)M * 2 * W * sizeof(T));
            if ((rc = attn_cls_fwd_bf16((const bf16_t*)h->qkv[sl], 3 * W, (bf16_t*)h->attn_o[sl], W, h->lse_cls, B, h->H,
                                        S, s))) return rc;
        } else {
            PROF("attn_fwd", attn_flops, 0);
            float* lse2 = (save && !h->lse2.empty()) ? h->lse2[sl] : nullptr;      // (with a peer too: the lse rows stay in h->lse2)
            if ((rc = attention_fwd<T>(h, s, fp, h->qkv[sl], h->attn_o[sl], h->lse[sl], lse2, peer ? (bf16_t*)peer->qkv[l] : nullptr,
                                       peer ? (bf16_t*)peer->attn_o[l] : nullptr, B))) return rc;
        }
        ProfScope tail_mlp(h, s, tl ? "tail_mlp_fwd" : nullptr, 2.0 * B * W * 9 * W, 0);      // (the four launches below, to the end of the block)
        {
            PROF_IF(!tl, "gemm_out_fwd", 2.0 * M * W * W, 0);
            if ((rc = linear_fwd<T>(h->lin, s, h->attn_o[sl], W, r.M, W, W, y.w_out, y.w_out_nk, y.b_out, EPI_F32_RESID,
                                    x_mid, r.ld, nullptr, x_in))) return rc;
        }
        {
            PROF_IF(!tl, "layernorm_fwd", 0, (double)M * W * (4 + sizeof(T)));
            if (!tl && ln_into_split(h->lin, s, x_mid, y.ln2_w, y.ln2_b, ln2o, h->mean_at(2 + 2 * l), h->rstd_at(2 + 2 * l), M, 4 * W, W, &rc)) { if (rc) return rc; }      // (e)
            else
            if ((rc = layernorm_fwd<T>(x_mid, r.ld, y.ln2_w, y.ln2_b, (T*)ln2o, W, h->mean_at(2 + 2 * l),
                                       h->rstd_at(2 + 2 * l), r.M, W, s))) return rc;
        }
        {
            PROF_IF(!tl, "gemm_fc1_fwd", 2.0 * M * W * 4 * W, 0);
            if ((rc = linear_fwd<T>(h->lin, s, ln2o, W, r.M, 4 * W, W, y.w_fc, y.w_fc_nk, y.b_fc, EPI_BF16_ACT, gact, 4 * W,
                                    save ? h->h_pre[sl] : nullptr, nullptr, 0, peer ? (bf16_t*)peer->h_pre[l] : nullptr))) return rc;
            if (peer) h->exported_dact = true;      // (dact_out given, and out_pre with it - a peer's forward saves: linear_fwd wrote act'(fc1))
        }
        {
            PROF_IF(!tl, "gemm_fc2_fwd", 2.0 * M * W * 4 * W, 0);
            if ((rc = linear_fwd<T>(h->lin, s, gact, 4 * W, r.M, W, 4 * W, y.w_proj, y.w_proj_nk, y.b_proj,
                                    EPI_F32_RESID, x_out, r.ld, nullptr, x_mid))) return rc;
        }
    }
    if (tp) {
        PROF("tokens_out", 0, (double)M * W * 8);
        float* xt = XS(2 * Lrun);
        if (tp->ln_post) {
            if ((rc = layernorm_fwd<float>(xt, W, h->lnpost_w, h->lnpost_b, tp->out_tokens ? tp->out_tokens : h->tok_buf, W, h->tok_mean,
                                           h->tok_rstd, M, W, s))) return rc;
        } else if (tp->out_tokens) {
            RVLM_HIP(hipMemcpyAsync(tp->out_tokens, xt, (size_t)M * W * 4, hipMemcpyDeviceToDevice, s));
        }
    }
    if (Lrun == L) {
        PROF("head_fwd", 2.0 * B * W * D, 0);
        float* xf = XS(2 * L);
        if ((rc = layernorm_fwd<float>(xf, (long)S * W, h->lnpost_w, h->lnpost_b, h->pooled, W,
                                       h->mean_at(2 * L + 1), h->rstd_at(2 * L + 1), B, W, s))) return rc;
        GemmF32 g;
        g.A = h->pooled; g.sam = W; g.sak = 1;
        g.B = h->proj; g.sbn = 1; g.sbk = D;
        g.C = (normalize || !out_emb) ? h->emb_raw : out_emb; g.scm = D; g.scn = 1;      // (!out_emb: a token pass that did not ask for it)
        g.M = B; g.N = D; g.K = W;
        if ((rc = gemm_f32(g, s))) return rc;
        if (normalize) {
            if ((rc = l2_normalize_fwd(h->emb_raw, out_emb, h->inv_norm, B, D, s))) return rc;
        }
    }
    if (save) { h->saved_B = B; h->saved_norm = normalize != 0; h->saved_mode = (Saved)save; h->next_param_stage = 0; }
    if (save && tp) { h->saved_mode = save == 2 ? Saved::TokensParams : Saved::Tokens; h->saved_depth = Lrun; h->saved_lnpost = tp->ln_post != 0; }
    if (peer) {      // (for the peer's backward only - a provider's single slots / no probabilities kept for a batched backward)
        if (h->provider || !h->own_flash) h->saved_mode = Saved::ForPeer;
        h->exported_to = peer->uid;
    }
    return RVLM_OK;
}

// for_peer: see forward_impl
int vit_forward(rvlm_vit* h, const float* x, const float* delta, int B, int normalize, int save,
                float* out_emb, hipStream_t s, rvlm_vit* for_peer) {
    return h->lin.bf16 ? forward_impl<bf16_t>(h, x, delta, B, normalize, save, out_emb, s, nullptr, for_peer)
                   : forward_impl<float>(h, x, delta, B, normalize, save, out_emb, s, nullptr, for_peer);
}
int vit_forward_tokens(rvlm_vit* h, const float* x, const float* delta, int B, const TokPass& tp, int save, float* out_emb,
                       hipStream_t s) {
    return h->lin.bf16 ? forward_impl<bf16_t>(h, x, delta, B, 0, save, out_emb, s, &tp)
                   : forward_impl<float>(h, x, delta, B, 0, save, out_emb, s, &tp);
}

// ---- token-level entries (RVLM_HAS_TOKENS) ---------------------------------------------------------------------------------------
int tokens_check(const rvlm_vit* h, int B, int depth, int save, const char* who) {
    if (B <= 0 || B > h->maxB) return fail(RVLM_ERR_ARG, std::string(who) + ": batch exceeds max_batch");
    if (depth < 1 || depth > h->L) return fail(RVLM_ERR_ARG, std::string(who) + ": depth must be in 1..layers");
    if (save && h->provider) return fail(RVLM_ERR_STATE, std::string(who) + ": a forward-provider handle (trainable = -2) keeps no "
                                                         "activations of its own: token passes run on plain bf16 / fp32 / x3 handles");
    if (save && h->inference_only) return fail(RVLM_ERR_STATE, std::string(who) + ": inference-only handle cannot save activations");
    return RVLM_OK;
}

}  // namespace rvlm

// ---- C ABI: the forward entries -------------------------------------------------------------------------------------------
extern "C" int rvlm_vit_forward(rvlm_vit* h, const float* x, const float* delta, int B, int output_normalize,
                                int save_for_backward, float* out_emb, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x && out_emb, "rvlm_vit_forward: null argument");
    RVLM_REQUIRE(B > 0 && B <= h->maxB, "rvlm_vit_forward: batch exceeds max_batch");
    RVLM_REQUIRE(save_for_backward != 2 || h->trainable, "rvlm_vit_forward: save_for_backward == 2 needs a trainable handle");
    RVLM_REQUIRE(save_for_backward == 0 || !h->inference_only, "rvlm_vit_forward: inference-only handle cannot save activations");
    return vit_forward(h, x, delta, B, output_normalize, save_for_backward, out_emb, (hipStream_t)stream);
}

extern "C" int rvlm_vit_forward_for(rvlm_vit* h, rvlm_vit* consumer, const float* x, const float* delta, int B, int output_normalize,
                                    float* out_emb, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && consumer && x && out_emb, "rvlm_vit_forward_for: null argument");
    RVLM_REQUIRE(B > 0 && B <= h->maxB, "rvlm_vit_forward_for: batch exceeds max_batch");
    RVLM_REQUIRE(!h->lin.bf16 && consumer->lin.bf16 && !h->inference_only && !consumer->inference_only && h->Mp == consumer->Mp &&
                 h->W == consumer->W && h->L == consumer->L && h->S == consumer->S && h->H == consumer->H,
                 "rvlm_vit_forward_for: needs an fp32-storage handle and a bf16 handle of the same architecture and max_batch");
    RVLM_REQUIRE_SAME_INPUT(h, consumer, "rvlm_vit_forward_for");
    return vit_forward(h, x, delta, B, output_normalize, 1, out_emb, (hipStream_t)stream, consumer);
}

extern "C" int rvlm_vit_forward_tokens(rvlm_vit* h, const float* x, const float* delta, int B, int depth, int ln_post, int save,
                                       float* out_tokens, float* out_emb, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && x && out_tokens, "rvlm_vit_forward_tokens: null argument");
    int rc = tokens_check(h, B, depth, save, "rvlm_vit_forward_tokens"); if (rc) return rc;
    RVLM_REQUIRE(!out_emb || depth == h->L, "rvlm_vit_forward_tokens: the pooled embedding exists at depth == layers only");
    RVLM_REQUIRE(save == 0 || save == 1 || save == 2, "rvlm_vit_forward_tokens: save must be 0, 1 or 2");
    RVLM_REQUIRE(save != 2 || h->trainable, "rvlm_vit_forward_tokens: save == 2 needs a trainable handle (no weight gradients from a "
                                            "token pass of any other handle)");
    if (ln_post && (rc = tok_ensure(h, false))) return rc;
    return vit_forward_tokens(h, x, delta, B, TokPass{depth, ln_post != 0, out_tokens}, save, out_emb, (hipStream_t)stream);
}
