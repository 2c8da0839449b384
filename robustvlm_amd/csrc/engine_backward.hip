// The backward half of the ViT engine (engine_internal.h): attention backward, weight gradients, the block walker, the rule which
// backward may read which saved forward, the handoff, and the backward entries of the C ABI.
#include <algorithm>
#include <type_traits>

#include "engine_internal.h"

namespace rvlm {

// (lse: the saved forward's log-sum-exp rows - bf16 - or probabilities - fp32 batched path; lse2: the fp32 flash kernels' rows or null)
template <typename T>
static int attention_bwd(rvlm_vit* h, hipStream_t s, const void* qkv, const void* o, const void* d_o,
                         const float* lse, const float* lse2, void* dqkv, int B);
template <>
int attention_bwd<bf16_t>(rvlm_vit* h, hipStream_t s, const void* qkv, const void* o, const void* d_o,
                          const float* lse, const float*, void* dqkv, int B) {
    return attn_bwd_bf16((const bf16_t*)qkv, 3 * h->W, (const bf16_t*)o, h->W, (const bf16_t*)d_o, h->W,
                         lse, h->dsum, (bf16_t*)dqkv, 3 * h->W, B, h->H, h->S, s);
}
template <>
int attention_bwd<float>(rvlm_vit* h, hipStream_t s, const void* qkv_, const void* o_, const void* d_o_,
                         const float* P, const float* lse2, void* dqkv_, int B) {
    const int S = h->S, W = h->W, H = h->H, Sld = (int)round_up(S, 4);
    const float* qkv = (const float*)qkv_;
    const float* d_o = (const float*)d_o_;
    float* dqkv = (float*)dqkv_;
    int rc = RVLM_OK;                                             // (P: kept by the forward)
    if (h->own_flash) {      // probabilities recomputed from the forward's log-sum-exp rows
        if (attn_bwd_f32_flash(qkv, (const float*)o_, d_o, lse2, (int)round_up(S, 32), h->dsum, dqkv, B, H, S, s, &rc)) return rc;
        return fail(RVLM_ERR_STATE, "attention backward: flash kernels refused a sequence length they cover");
    }
    const long bs1 = (long)H * S * Sld, bs2 = (long)S * Sld, qs1 = (long)S * 3 * W, os1 = (long)S * W;
    GemmF32 g;  // dP = dO V^T
    g.A = d_o; g.sam = W; g.sak = 1; g.sab1 = os1; g.sab2 = 64;
    g.B = qkv + 2 * W; g.sbn = 3 * W; g.sbk = 1; g.sbb1 = qs1; g.sbb2 = 64;
    g.C = h->dscores; g.scm = Sld; g.scn = 1; g.scb1 = bs1; g.scb2 = bs2;
    g.M = S; g.N = S; g.K = 64; g.nb1 = B; g.nb2 = H;
    if ((rc = gemm_f32(g, s))) return rc;
    if ((rc = softmax_rows_bwd(P, h->dscores, (long)B * H * S, S, Sld, 0.125f, s))) return rc;
    GemmF32 q;  // dQ = dS K
    q.A = h->dscores; q.sam = Sld; q.sak = 1; q.sab1 = bs1; q.sab2 = bs2; q.pad4 = 1;
    q.B = qkv + W; q.sbn = 1; q.sbk = 3 * W; q.sbb1 = qs1; q.sbb2 = 64;
    q.C = dqkv; q.scm = 3 * W; q.scn = 1; q.scb1 = qs1; q.scb2 = 64;
    q.M = S; q.N = 64; q.K = S; q.nb1 = B; q.nb2 = H;
    if ((rc = gemm_f32(q, s))) return rc;
    GemmF32 k;  // dK = dS^T Q
    k.A = h->dscores; k.sam = 1; k.sak = Sld; k.sab1 = bs1; k.sab2 = bs2; k.pad4 = 1;
    k.B = qkv; k.sbn = 1; k.sbk = 3 * W; k.sbb1 = qs1; k.sbb2 = 64;
    k.C = dqkv + W; k.scm = 3 * W; k.scn = 1; k.scb1 = qs1; k.scb2 = 64;
    k.M = S; k.N = 64; k.K = S; k.nb1 = B; k.nb2 = H;
    if ((rc = gemm_f32(k, s))) return rc;
    GemmF32 v;  // dV = P^T dO
    v.A = P; v.sam = 1; v.sak = Sld; v.sab1 = bs1; v.sab2 = bs2; v.pad4 = 1;
    v.B = d_o; v.sbn = 1; v.sbk = W; v.sbb1 = os1; v.sbb2 = 64;
    v.C = dqkv + 2 * W; v.scm = 3 * W; v.scn = 1; v.scb1 = qs1; v.scb2 = 64;
    v.M = S; v.N = 64; v.K = S; v.nb1 = B; v.nb2 = H;
    return gemm_f32(v, s);
}

// ---- QKV dgrad of the last block under the class-token tail (forward: qkv_tail_fwd, engine_forward.hip): K, V for every token, Q for
// the class rows only.  d_ln = dqkv[:, W:3W] @ W_in[W:3W] for every row (K = 2W), then the class rows are overwritten with their
// full product (K = 3W).
static int qkv_tail_bwd(rvlm_vit* h, hipStream_t s, const void* dqkv, const Layer& y, void* d_ln, int B) {
    const int S = h->S, W = h->W, M = B * S;
    GemmBf16 g;
    g.A = (const bf16_t*)dqkv + W; g.lda = 3 * W; g.Bw = y.w_in_t + W; g.ldb = 3 * W;
    g.M = M; g.N = W; g.K = 2 * W; g.a_rows = (int)round_up(M, 128); g.epi = EPI_BF16;
    g.out = d_ln; g.ldo = W; g.act = h->cfg.act;
    with_scratch(h->lin, g);
    int rc = gemm_bf16_nt(g, s);
    if (rc) return rc;
    GemmBf16 q;
    q.A = (const bf16_t*)dqkv; q.lda = (long)S * 3 * W; q.Bw = y.w_in_t; q.ldb = 3 * W;
    q.M = B; q.N = W; q.K = 3 * W; q.a_rows = B; q.epi = EPI_BF16;
    q.out = d_ln; q.ldo = (long)S * W; q.act = h->cfg.act;
    with_scratch(h->lin, q);
    return gemm_bf16_nt(q, s);
}

__global__ void __launch_bounds__(256)
widen_bf16_kernel(const bf16_t* __restrict__ src, float* __restrict__ dst, size_t n8) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (size_t)gridDim.x * blockDim.x) {
        const bf16x8 v = *(const bf16x8*)(src + 8 * i);
        float o[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (float)v[e];
        *(float4*)(dst + 8 * i) = *(const float4*)&o[0];
        *(float4*)(dst + 8 * i + 4) = *(const float4*)&o[4];
    }
}

// ---- weight gradients ------------------------------------------------------------------------------
// dW[N,K] (+)= dY[M,N]^T @ X[M,K]
// dbias != null: dbias[N] (+)= column sums of dY as well (fused into the operand transpose where that exists)
template <typename T>
static int wgrad(rvlm_vit* h, hipStream_t s, const void* dY, long lddy, const void* X, long ldx, int M, int N, int K,
                 float* dW, long lddw, int accumulate, float* dbias = nullptr);
template <>
int wgrad<bf16_t>(rvlm_vit* h, hipStream_t s, const void* dY, long lddy, const void* X, long ldx, int M, int N,
                  int K, float* dW, long lddw, int accumulate, float* dbias) {
    // contraction over the token dimension.  Encoder shapes: the persistent kernel's contraction-major form reads dY and X as the
    // backward left them (token-major), split-K over token chunks in one batched launch - no transposed copies.
    int rc, splits = 0, Kc = 0;
    if (wgrad_split_plan(M, N, K, h->lin.splitk_bytes, &splits, &Kc) && lddy % 8 == 0 && ldx % 8 == 0 &&
        (((size_t)dY | (size_t)X) & 15) == 0) {
        if (dbias && (rc = colsum<bf16_t>((const bf16_t*)dY, lddy, M, N, dbias, accumulate, h->red_scratch, h->red_floats, s)))
            return rc;
        return gemm_bf16_wgrad_tn((const bf16_t*)dY, lddy, (const bf16_t*)X, ldx, M, splits, Kc, N, K, dW, lddw, accumulate,
                                  h->lin.splitk, h->lin.splitk_bytes, s);
    }
    // other shapes (conv1: K = 3*P*P): whole-K transposes zero-padded to a multiple of 64, NT GEMM as usual
    if (dbias && (rc = colsum<bf16_t>((const bf16_t*)dY, lddy, M, N, dbias, accumulate, h->red_scratch, h->red_floats, s)))
        return rc;
    const int Mk = (int)round_up(M, 64);
    // leading dimension of the transposed copies: all tokens when the operand's rows fit that way (conv1; every linear of a
    // width that is no multiple of 256), else the few tokens of this call (the < 256-token fallback of the encoder linears)
    const size_t need_rows = (size_t)round_up(std::max(N, K), 128);
    long ldt = h->Mpt;
    if (need_rows * (size_t)ldt > h->t_elems) ldt = Mk;
    if (need_rows * (size_t)ldt > h->t_elems || Mk > ldt)
        return fail(RVLM_ERR_STATE, "wgrad: transposed-operand scratch too small for this shape");
    if ((rc = transpose_pad<bf16_t>((const bf16_t*)dY, lddy, M, N, (bf16_t*)h->tA, ldt, Mk, s))) return rc;
    if ((rc = transpose_pad<bf16_t>((const bf16_t*)X, ldx, M, K, (bf16_t*)h->tB, ldt, Mk, s))) return rc;
    GemmBf16 g;
    g.A = (const bf16_t*)h->tA; g.lda = ldt; g.Bw = (const bf16_t*)h->tB; g.ldb = ldt;
    g.M = N; g.N = K; g.K = Mk; g.a_rows = (int)std::min<size_t>(h->t_elems / (size_t)ldt, (size_t)4 * h->W);
    g.epi = accumulate ? EPI_F32_RESID : EPI_F32; g.residual = accumulate ? dW : nullptr;
    g.out = dW; g.ldo = lddw;
    with_scratch(h->lin, g);
    return gemm_bf16_nt(g, s);
}
template <>
int wgrad<float>(rvlm_vit* h, hipStream_t s, const void* dY, long lddy, const void* X, long ldx, int M, int N, int K,
                 float* dW, long lddw, int accumulate, float* dbias) {
    int rc;
    if (dbias && (rc = colsum<float>((const float*)dY, lddy, M, N, dbias, accumulate, h->red_scratch, h->red_floats, s)))
        return rc;
    GemmF32 g;
    g.A = (const float*)dY; g.sam = 1; g.sak = lddy;      // (m_out = n, k = token)
    g.B = (const float*)X; g.sbn = 1; g.sbk = ldx;        // (n_out = k, k = token)
    g.C = dW; g.scm = lddw; g.scn = 1;
    g.M = N; g.N = K; g.K = M;
    g.residual = accumulate ? dW : nullptr;
    return gemm_f32(g, s);
}

// ---- backward ------------------------------------------------------------------------------------
static SavedView own_view(const rvlm_vit* h) {
    return {h->xs.data(), h->st_mean, h->st_rstd, h->Mp, h->patch_out, h->emb_raw, h->inv_norm, h->lse.data(),
            h->lse2.empty() ? nullptr : h->lse2.data(), h->saved_norm, h->cls_tail};
}

static inline float* grad_of(const float* p) { return const_cast<float*>(p); }

// Head, first half: d_raw = l2-normalise'(d_emb) where the forward normalised, [sink: proj gradient], d_pooled = d_raw @ proj^T,
// [sink: ln_post's gradients].  Leaves h->d_pooled.
static int head_dpooled(rvlm_vit* h, const SavedView& v, const float* d_emb, int B, const ParamSink* sink, hipStream_t s) {
    const int W = h->W, L = h->L, D = h->D;
    int rc;
    const float* d_raw = d_emb;
    if (v.norm) {
        if ((rc = l2_normalize_bwd(d_emb, v.emb_raw, v.inv_norm, h->d_raw, B, D, s))) return rc;
        d_raw = h->d_raw;
    }
    if (sink) {   // dproj[W,D] (+)= pooled^T d_raw
        GemmF32 g;
        g.A = h->pooled; g.sam = 1; g.sak = W;
        g.B = d_raw; g.sbn = 1; g.sbk = D;
        g.C = grad_of(sink->gw->proj); g.scm = D; g.scn = 1;
        g.M = W; g.N = D; g.K = B;
        g.residual = sink->accumulate ? sink->gw->proj : nullptr;
        if ((rc = gemm_f32(g, s))) return rc;
    }
    GemmF32 g;  // d_pooled = d_raw @ proj^T
    g.A = d_raw; g.sam = D; g.sak = 1;
    g.B = h->proj; g.sbn = D; g.sbk = 1;
    g.C = h->d_pooled; g.scm = W; g.scn = 1;
    g.M = B; g.N = W; g.K = D;
    if ((rc = gemm_f32(g, s))) return rc;
    if (sink) return ln_param_grad<float>(h->d_pooled, W, v.xs[2 * L], (long)h->S * W, v.mean_at(2 * L + 1), v.rstd_at(2 * L + 1), B, W,
                                          grad_of(sink->gw->ln_post_weight), grad_of(sink->gw->ln_post_bias), sink->accumulate,
                                          h->red_scratch, h->red_floats, s);
    return RVLM_OK;
}
// Head, second half: ln_post'(d_pooled) into the class rows (stride S*W) of d32 and / or dlp, written or added (accumulate).
template <typename To>
static int head_lnpost_bwd(rvlm_vit* h, const SavedView& v, float* d32, To* dlp, int accumulate, int B, hipStream_t s) {
    const long SW = (long)h->S * h->W;
    return layernorm_bwd<float, To>(h->d_pooled, h->W, v.xs[2 * h->L], SW, h->lnpost_w, v.mean_at(2 * h->L + 1), v.rstd_at(2 * h->L + 1),
                                    d32, SW, dlp, SW, accumulate, B, h->W, s);
}

// Embedding stage of the input-gradient pass: ln_pre / embedding backward, patch GEMM, col2im
template <typename T>
static int embed_bwd_input(rvlm_vit* h, const SavedView& v, bool widen, int B, float* grad_x, hipStream_t s) {
    const int S = h->S, W = h->W, M = B * S, M0 = B * h->G * h->G;
    int rc;
    {
        PROF("embed_lnpre_bwd", 0, (double)M * W * 8);
        if (widen) {      // (the embedding backward reads the residual gradient as fp32: one widening pass per backward, 40 us)
            hipLaunchKernelGGL(widen_bf16_kernel, dim3(ew_blocks((size_t)M * W / 8)), dim3(256), 0, s, (const bf16_t*)h->dres_lp, h->dres, (size_t)M * W / 8);
            RVLM_CHECK_LAUNCH();
        }
        if ((rc = embed_lnpre_bwd<T>(h->dres, W, v.patch_out, W, h->cls, h->pos, h->lnpre_w, v.mean_at(0),
                                     v.rstd_at(0), (T*)h->d_patch, W, B, S, W, s))) return rc;
    }
    {
        PROF("gemm_patch_bwd", 2.0 * M0 * W * h->Kp, 0);
        if (h->lin.bf16) {
            GemmBf16 g;
            g.A = (const bf16_t*)h->d_patch; g.lda = W; g.Bw = h->conv_t; g.ldb = W;
            g.M = M0; g.N = h->Kpad; g.K = W; g.a_rows = h->Mp0; g.epi = EPI_F32; g.out = h->dA0; g.ldo = h->Kpad;
            with_scratch(h->lin, g);
            rc = gemm_bf16_nt(g, s);
        } else {
            GemmF32 g;
            g.A = (const float*)h->d_patch; g.sam = W; g.sak = 1;
            g.B = h->conv_f32; g.sbn = 1; g.sbk = h->Kp;
            g.C = h->dA0; g.scm = h->Kpad; g.scn = 1;
            g.M = M0; g.N = h->Kp; g.K = W;
            rc = gemm_f32(g, s);
        }
        if (rc) return rc;
    }
    PROF("patch_col2im", 0, (double)B * 3 * h->img * h->img * 4 + (double)B * 3 * h->in_h * h->in_w * 4);
    return h->resize ? col2im_resize_grad<float>(h->dA0, h->Kpad, B, h->rs_h, h->rs_w, h->P, h->cfg.std, grad_x, s)
                     : col2im_grad<float>(h->dA0, h->Kpad, B, h->img, h->P, h->cfg.std, grad_x, s);
}
// Embedding stage of the parameter pass: ln_pre, positional / class embedding, conv1
template <typename T>
static int embed_bwd_params(rvlm_vit* h, const SavedView& v, const ParamSink& k, int B, hipStream_t s) {
    const int S = h->S, W = h->W, M = B * S, M0 = B * h->G * h->G, acc = k.accumulate;
    int rc;
    if ((rc = ln_param_grad<float>(h->dres, W, h->tokens, W, v.mean_at(0), v.rstd_at(0), M, W, grad_of(k.gw->ln_pre_weight),
                                   grad_of(k.gw->ln_pre_bias), acc, h->red_scratch, h->red_floats, s))) return rc;
    if ((rc = layernorm_bwd<float, float>(h->dres, W, h->tokens, W, h->lnpre_w, v.mean_at(0), v.rstd_at(0), h->dtok,
                                          W, nullptr, W, 0, M, W, s))) return rc;
    if ((rc = pos_cls_grad(h->dtok, W, B, S, W, grad_of(k.gw->positional_embedding), grad_of(k.gw->class_embedding), acc, s))) return rc;
    if ((rc = gather_patch_rows<T>(h->dtok, W, B, S, W, (T*)h->d_patch, W, s))) return rc;
    // conv1.weight [W, 3*P*P] (+)= d_patch^T A0   (A0 has Kpad >= Kp columns; only Kp are weights)
    return wgrad<T>(h, s, h->d_patch, W, h->A0, h->Kpad, M0, W, h->Kp, grad_of(k.gw->conv1_weight), h->Kp, acc);
}

// Gradients of parameters a token cotangent cannot reach: zeros where the pass writes, untouched where it adds
static int zero_unreached(const ParamSink& k, float* g, size_t n, hipStream_t s) {
    if (!k.accumulate) RVLM_HIP(hipMemsetAsync(g, 0, n * 4, s));
    return RVLM_OK;
}
static int zero_block_grads(rvlm_vit* h, const ParamSink& k, int l, hipStream_t s) {
    const size_t W = (size_t)h->W;
    const rvlm_vit_block_weights& g = k.gw->blocks_host[l];
    const struct { const float* p; size_t n; } t[] = {
        {g.ln_1_weight, W}, {g.ln_1_bias, W}, {g.attn_in_proj_weight, 3 * W * W}, {g.attn_in_proj_bias, 3 * W},
        {g.attn_out_proj_weight, W * W}, {g.attn_out_proj_bias, W}, {g.ln_2_weight, W}, {g.ln_2_bias, W},
        {g.mlp_c_fc_weight, 4 * W * W}, {g.mlp_c_fc_bias, 4 * W}, {g.mlp_c_proj_weight, 4 * W * W}, {g.mlp_c_proj_bias, W}};
    for (const auto& e : t) { int rc = zero_unreached(k, grad_of(e.p), e.n, s); if (rc) return rc; }
    return RVLM_OK;
}

// The backward walker: head (or token seed), blocks from the top down, embeddings - on h's kernels, scratch and weights, of the saved
// forward `v`.  Without a sink: the input gradient into grad_x.  With a sink: the parameter pass - the same chain with each linear's
// weight gradient issued before its dgrad and each LayerNorm's before its backward, from the inputs a save-mode-2 forward kept on h
// (ln1_out, ln2_out, g_act_l, tokens), cut into the sink's stages, always on the fp32 residual-gradient stream, and WITHOUT profile
// scopes (a training step's classes are not part of rvlm_vit_get_profile).
// With a token seed AND a sink: the parameter pass of a token forward (Saved::TokensParams).  Stage 0 seeds the stream from d_tokens
// and owns proj / ln_post; the stages of blocks >= depth own parameters the cotangent cannot reach.  Unreached parameters are
// zero-filled by their stage when the pass writes (accumulate == 0) and left alone when it adds.
// fp32_dres: keep the fp32 stream where the handle would run the bf16-only one (rvlm_vit::lp_dres).
template <typename T>
static int backward_impl(rvlm_vit* h, const SavedView& v, const float* d_emb, int B, float* grad_x, hipStream_t s, bool fp32_dres = false,
                         const TokSeed* ts = nullptr, const ParamSink* sink = nullptr) {
    const int S = h->S, W = h->W, L = h->L, D = h->D, M = B * S;
    const int Ltop = ts ? ts->depth : L;            // the stream enters above block Ltop - 1
    const bool tail = v.tail && !ts;
    const bool prof = !sink;
    const int st0 = sink ? sink->stage_begin : 0, st1 = sink ? sink->stage_end : L + 2;
    const int acc = sink ? sink->accumulate : 0;
    const double attn_flops = 8.0 * B * h->H * (double)S * S * 64;
    constexpr bool LP = !std::is_same<T, float>::value;
    // the fp32 residual-gradient stream, or none (LayerNorm backward then accumulates in the bf16 buffer, rvlm_vit::lp_dres)
    float* const dres32 = (LP && h->lp_dres && !fp32_dres && !sink) ? nullptr : h->dres;
    T* const dres_lp = LP ? (T*)h->dres_lp : nullptr;
    int rc;
    h->lin.a3_of = nullptr;
    if (ts && st0 <= 0 && st1 > 0) {
        // token pass: the stream starts as the token cotangent (every row live), plus the pooled path's class rows when d_emb is given
        PROF_IF(prof, "tokens_seed", d_emb ? 2.0 * B * W * D : 0.0, (double)M * W * (4 + (dres32 ? 4 : 0) + (LP ? sizeof(T) : 0)));
        if (d_emb && (rc = head_dpooled(h, v, d_emb, B, sink, s))) return rc;      // (a token pass's embedding is un-normalised)
        if (sink) {      // stage 0's parameters: proj and ln_post from the pooled path (above), ln_post over every row from the tokens
            if (!d_emb && (rc = zero_unreached(*sink, grad_of(sink->gw->proj), (size_t)W * D, s))) return rc;
            if (ts->ln_post) {
                if ((rc = ln_param_grad<float>(ts->d_tokens, W, v.xs[2 * Ltop], W, h->tok_mean, h->tok_rstd, M, W,
                                               grad_of(sink->gw->ln_post_weight), grad_of(sink->gw->ln_post_bias), (d_emb || acc) ? 1 : 0,
                                               h->red_scratch, h->red_floats, s))) return rc;
            } else if (!d_emb) {
                if ((rc = zero_unreached(*sink, grad_of(sink->gw->ln_post_weight), (size_t)W, s))) return rc;
                if ((rc = zero_unreached(*sink, grad_of(sink->gw->ln_post_bias), (size_t)W, s))) return rc;
            }
        }
        if (ts->d_tokens && !ts->ln_post) {
            const float* cls_add = nullptr;
            if (d_emb) {  // ln_post'(d_pooled) into the class rows of the fp32 buffer (a scratch where the stream is bf16 only): the seed
                          // kernel adds them in fp32 before it rounds
                if ((rc = head_lnpost_bwd<float>(h, v, h->dres, nullptr, 0, B, s))) return rc;
                cls_add = h->dres;
            }
            if ((rc = tokens_seed(ts->d_tokens, cls_add, (long)S * W, dres32, LP ? (bf16_t*)h->dres_lp : nullptr, M, h->Mp, S, W, s))) return rc;
        } else if (ts->d_tokens) {
            if (h->Mp > M) {
                if (dres32) RVLM_HIP(hipMemsetAsync(dres32 + (size_t)M * W, 0, (size_t)(h->Mp - M) * W * 4, s));
                if (LP) RVLM_HIP(hipMemsetAsync((T*)h->dres_lp + (size_t)M * W, 0, (size_t)(h->Mp - M) * W * sizeof(T), s));
            }
            if ((rc = layernorm_bwd<float, T>(ts->d_tokens, W, v.xs[2 * Ltop], W, h->lnpost_w, h->tok_mean, h->tok_rstd, dres32, W,
                                              dres_lp, W, 0, M, W, s))) return rc;
            if (d_emb && (rc = head_lnpost_bwd<T>(h, v, dres32, dres_lp, 1, B, s))) return rc;
        }
    } else if (!ts && st0 <= 0 && st1 > 0) {
        PROF_IF(prof, "head_bwd", 2.0 * B * W * D, 0);
        if ((rc = head_dpooled(h, v, d_emb, B, sink, s))) return rc;
        if (!tail) {   // with the class-token tail the last block's ln_1 backward overwrites the other rows
            if (dres32) RVLM_HIP(hipMemsetAsync(dres32, 0, (size_t)h->Mp * W * 4, s));
            if (LP) RVLM_HIP(hipMemsetAsync(h->dres_lp, 0, (size_t)h->Mp * W * sizeof(T), s));
        }
        if ((rc = head_lnpost_bwd<T>(h, v, dres32, dres_lp, 0, B, s))) return rc;
    }
    const void* dres_A = LP ? (const void*)h->dres_lp : (const void*)h->dres;
    for (int l = L - 1; sink && l >= Ltop; --l)      // blocks the token pass did not run
        if (L - l >= st0 && L - l < st1 && (rc = zero_block_grads(h, *sink, l, s))) return rc;
    for (int l = Ltop - 1; l >= 0; --l) {
        if (L - l < st0 || L - l >= st1) continue;
        Layer& y = h->layers[l];
        const rvlm_vit_block_weights* gb = sink ? &sink->gw->blocks_host[l] : nullptr;
        // The class-token tail is this block with (a) the steps before the attention (in backward order) on the class rows, (b) the
        // QKV dgrad over K, V of every row and Q of the class rows, (c) the class query's attention backward, (d) an ln_1 backward that
        // overwrites the rows that carry no residual gradient yet; its few-row launches are accounted as two coarse profile classes
        // (tail_mlp_bwd, tail_attn_bwd) instead of one per step.
        const bool tl = tail && l == L - 1;
        const Rows r = tl ? Rows{B, (long)S * W, B} : Rows{M, (long)W, 0};      // (a)
        const bool pf = prof && !tl;
        {
            ProfScope tail_mlp(h, s, (prof && tl) ? "tail_mlp_bwd" : nullptr, 2.0 * B * W * 9 * W, 0);      // (the four dgrad / LayerNorm launches)
            {   // fc2 (c_proj): dY = d(residual), X = act(fc1)
                PROF_IF(pf, "gemm_fc2_bwd", 2.0 * M * W * 4 * W, 0);
                if (sink && (rc = wgrad<T>(h, s, dres_A, r.ld, h->g_act_l[l], 4 * W, r.M, W, 4 * W, grad_of(gb->mlp_c_proj_weight), 4 * W, acc,
                                           grad_of(gb->mlp_c_proj_bias)))) return rc;
                if ((rc = linear_dgrad<T>(h->lin, s, dres_A, r.ld, r.M, W, 4 * W, y.w_proj, 4 * W, y.w_proj_t, EPI_BF16_DACT,
                                          h->dh, 4 * W, h->h_pre[l], r.a_rows))) return rc;
            }
            {   // fc1 (c_fc)  (its A operand is the B-row dh, not the stream: no a_rows)
                PROF_IF(pf, "gemm_fc1_bwd", 2.0 * M * W * 4 * W, 0);
                if (sink && (rc = wgrad<T>(h, s, h->dh, 4 * W, h->ln2_out[l], W, r.M, 4 * W, W, grad_of(gb->mlp_c_fc_weight), W, acc,
                                           grad_of(gb->mlp_c_fc_bias)))) return rc;
                if ((rc = linear_dgrad<T>(h->lin, s, h->dh, 4 * W, r.M, 4 * W, W, y.w_fc, W, y.w_fc_t, EPI_BF16, h->d_ln, W,
                                          nullptr))) return rc;
            }
            {
                PROF_IF(pf, "layernorm_bwd", 0, (double)M * W * ((dres32 ? 12 : 6) + 2 * sizeof(T)));
                if (sink && (rc = ln_param_grad<T>((const T*)h->d_ln, W, v.xs[2 * l + 1], r.ld, v.mean_at(2 + 2 * l), v.rstd_at(2 + 2 * l),
                                                   r.M, W, grad_of(gb->ln_2_weight), grad_of(gb->ln_2_bias), acc, h->red_scratch,
                                                   h->red_floats, s))) return rc;
                if ((rc = layernorm_bwd<T, T>((const T*)h->d_ln, W, v.xs[2 * l + 1], r.ld, y.ln2_w, v.mean_at(2 + 2 * l),
                                              v.rstd_at(2 + 2 * l), dres32, r.ld, dres_lp, r.ld, 1, r.M, W, s))) return rc;
            }
            {   // attention out-proj
                PROF_IF(pf, "gemm_out_bwd", 2.0 * M * W * W, 0);
                if (sink && (rc = wgrad<T>(h, s, dres_A, r.ld, h->attn_o[l], W, r.M, W, W, grad_of(gb->attn_out_proj_weight), W, acc,
                                           grad_of(gb->attn_out_proj_bias)))) return rc;
                if ((rc = linear_dgrad<T>(h->lin, s, dres_A, r.ld, r.M, W, W, y.w_out, W, y.w_out_t, EPI_BF16, h->d_o, W,
                                          nullptr, r.a_rows))) return rc;
            }
        }
        if (tl) {      // (c)
            PROF_IF(prof, "tail_attn_bwd", 12.0 * B * h->H * (double)S * 64, (double)M * 5 * W * sizeof(T));
            if ((rc = attn_cls_bwd_bf16((const bf16_t*)h->qkv[l], 3 * W, (const bf16_t*)h->attn_o[l], W,
                                        (const bf16_t*)h->d_o, W, h->lse_cls, (bf16_t*)h->dqkv, 3 * W, B, h->H, S, s)))
                return rc;
        } else {
            PROF_IF(prof, "attn_bwd", attn_flops, 0);
            if ((rc = attention_bwd<T>(h, s, h->qkv[l], h->attn_o[l], h->d_o, v.lse[l], v.lse2 ? v.lse2[l] : nullptr, h->dqkv, B)))
                return rc;
        }
        {   // qkv in-proj  (b: the parameter pass takes the plain dgrad on the tail too, next to its weight gradient over every row)
            const bool qkv_tail = tl && !sink;
            PROF_IF(prof, "gemm_qkv_bwd", qkv_tail ? 2.0 * M * W * 2 * W + 2.0 * B * W * 3 * W : 2.0 * M * W * 3 * W, 0);
            if (sink && (rc = wgrad<T>(h, s, h->dqkv, 3 * W, h->ln1_out[l], W, M, 3 * W, W, grad_of(gb->attn_in_proj_weight), W, acc,
                                       grad_of(gb->attn_in_proj_bias)))) return rc;
            rc = qkv_tail ? qkv_tail_bwd(h, s, h->dqkv, y, h->d_ln, B)
                          : linear_dgrad<T>(h->lin, s, h->dqkv, 3 * W, M, 3 * W, W, y.w_in, W, y.w_in_t, EPI_BF16, h->d_ln, W, nullptr);
            if (rc) return rc;
        }
        {
            PROF_IF(prof, "layernorm_bwd", 0, (double)M * W * ((dres32 ? 12 : 6) + 2 * sizeof(T)));
            if (sink && (rc = ln_param_grad<T>((const T*)h->d_ln, W, v.xs[2 * l], W, v.mean_at(1 + 2 * l), v.rstd_at(1 + 2 * l), M, W,
                                               grad_of(gb->ln_1_weight), grad_of(gb->ln_1_bias), acc, h->red_scratch, h->red_floats, s)))
                return rc;
            if ((rc = layernorm_bwd<T, T>((const T*)h->d_ln, W, v.xs[2 * l], W, y.ln1_w, v.mean_at(1 + 2 * l), v.rstd_at(1 + 2 * l),
                                          dres32, W, dres_lp, W, tl ? -S : 1, M, W, s))) return rc;      // (d)
        }
    }
    if (st1 <= L + 1) return RVLM_OK;
    return sink ? embed_bwd_params<T>(h, v, *sink, B, s) : embed_bwd_input<T>(h, v, dres32 == nullptr, B, grad_x, s);
}

// (which backward may read which saved forward: enum Reader, engine_internal.h)
int saved_check(const rvlm_vit* h, Reader r, int B, const char* who) {
    const bool have = B > 0 && h->saved_B == B;
    const Saved m = h->saved_mode;
    switch (r) {
    case Reader::Input:
        if (!have) return fail(RVLM_ERR_STATE, "rvlm_vit_backward_input: no saved forward for this batch size");
        if (m == Saved::ForPeer) return fail(RVLM_ERR_STATE, "backward: the saved forward was run for another handle's backward (no probabilities kept)");
        if (is_token_pass(m)) return fail(RVLM_ERR_STATE, "backward: the saved forward is a token pass (rvlm_vit_backward_input_tokens differentiates it)");
        break;
    case Reader::Params:
        if (!have || m != Saved::Params) return fail(RVLM_ERR_STATE, std::string(who) + ": needs a forward with save_for_backward == 2 for this batch");
        break;
    case Reader::Tokens:
        if (!have || !is_token_pass(m))
            return fail(RVLM_ERR_STATE, h->saved_B > 0 && !is_token_pass(m)
                            ? "rvlm_vit_backward_input_tokens: the saved forward is a pooled pass (rvlm_vit_backward_input differentiates it)"
                            : "rvlm_vit_backward_input_tokens: no saved token forward for this batch size");
        break;
    case Reader::TokensParams:
        if (!have || m != Saved::TokensParams)
            return fail(RVLM_ERR_STATE, std::string(who) + ": needs a token forward with save == 2 for this batch");
        break;
    case Reader::Handoff:
        if (!have) return fail(RVLM_ERR_STATE, "handoff: no saved forward for this batch size on the fp32-storage handle");
        if (is_token_pass(m)) return fail(RVLM_ERR_STATE, "handoff: the saved forward is a token pass (the handoff precisions take pooled passes only)");
        break;
    }
    return RVLM_OK;
}

int vit_backward_tokens(rvlm_vit* h, const TokSeed& ts, const float* d_emb, int B, float* grad_x, hipStream_t s) {
    return h->lin.bf16 ? backward_impl<bf16_t>(h, own_view(h), d_emb, B, grad_x, s, false, &ts)
                   : backward_impl<float>(h, own_view(h), d_emb, B, grad_x, s, false, &ts);
}
int vit_backward(rvlm_vit* h, const float* d_emb, int B, float* grad_x, hipStream_t s) {
    int rc = saved_check(h, Reader::Input, B); if (rc) return rc;
    return h->lin.bf16 ? backward_impl<bf16_t>(h, own_view(h), d_emb, B, grad_x, s) : backward_impl<float>(h, own_view(h), d_emb, B, grad_x, s);
}
int vit_backward_params(rvlm_vit* h, const float* d_emb, int B, const ParamSink& sink, hipStream_t s) {
    return h->lin.bf16 ? backward_impl<bf16_t>(h, own_view(h), d_emb, B, nullptr, s, true, nullptr, &sink)
                   : backward_impl<float>(h, own_view(h), d_emb, B, nullptr, s, true, nullptr, &sink);
}
int vit_backward_params_tokens(rvlm_vit* h, const TokSeed& ts, const float* d_emb, int B, const ParamSink& sink, hipStream_t s) {
    return h->lin.bf16 ? backward_impl<bf16_t>(h, own_view(h), d_emb, B, nullptr, s, true, &ts, &sink)
                   : backward_impl<float>(h, own_view(h), d_emb, B, nullptr, s, true, &ts, &sink);
}

// HANDOFF (round 6): the input gradient of the forward SAVED ON `hx` (an fp32-storage handle: x3 or fp32 precision) evaluated by the
// bf16 handle `hb`'s backward kernels.  FARE's first cotangent 2 (phi(x + d0) - phi(x)) needs a faithful FORWARD - the difference of two
// nearly equal embeddings is where bf16 rounding noise decides a fifth of the first step's signs - but not a faithful backward: the
// cotangent's way back through the network only meets relative rounding errors (oracle/split_bf16_emulation.py: split-bf16 forward +
// bf16 backward 0.998 first-step sign agreement with the fp32 oracle; split-bf16 both ways 0.9996; bf16 both ways 0.82).  What the
// bf16 backward reads as fp32 (residual stream, LayerNorm statistics, patch embeddings, the unnormalised output) it reads from hx's
// buffers in place (the SavedView of hx's forward); what it reads in bf16 (qkv, attention output, act'(fc1)) is exported here from the
// fp32 tensors hx kept; the log-sum-exp rows were written by hx's softmax pass in the flash kernels' convention.  The view carries no
// class-token tail (hx ran the last block on every row) and the pass keeps the fp32 residual-gradient stream.
int vit_backward_from(rvlm_vit* hb, rvlm_vit* hx, const float* d_emb, int B, float* grad_x, hipStream_t s) {
    if (!hb->lin.bf16 || hx->lin.bf16) return fail(RVLM_ERR_STATE, "handoff: needs a bf16 handle and an fp32-storage (fp32 / x3) handle");
    int rc = saved_check(hx, Reader::Handoff, B); if (rc) return rc;
    if (hx->lse2.empty() || hb->inference_only) return fail(RVLM_ERR_STATE, "handoff: inference-only handle");
    if (hb->Mp != hx->Mp || hb->Mp0 != hx->Mp0 || hb->W != hx->W || hb->L != hx->L || hb->S != hx->S || hb->H != hx->H ||
        hb->D != hx->D || hb->P != hx->P || hb->cfg.act != hx->cfg.act)
        return fail(RVLM_ERR_STATE, "handoff: the two handles must hold the same architecture and max_batch");
    rvlm_vit* h = hb;                      // (PROF accounts on the bf16 handle)
    const int W = hb->W, L = hb->L, M = B * hb->S;
    {
        PROF("handoff_export", 0, (double)M * W * (3 * 6 + 6 + 4 * 6) * L);
        const bool have_qo = hx->exported_to == hb->uid, have_dact = have_qo && hx->exported_dact;     // written by the forward itself
        if (hx->provider && !(have_qo && have_dact))
            return fail(RVLM_ERR_STATE, "handoff: the forward-provider handle's saved pass was not run for this bf16 handle");
        for (int l = 0; l < L; ++l) {
            if (!have_qo && (rc = x3_export_bf16((const float*)hx->qkv[l], 3 * W, (bf16_t*)hb->qkv[l], 3 * W, M, 3 * W, 0, 0, s))) return rc;
            if (!have_qo && (rc = x3_export_bf16((const float*)hx->attn_o[l], W, (bf16_t*)hb->attn_o[l], W, M, W, 0, 0, s))) return rc;
            if (!have_dact && (rc = x3_export_bf16((const float*)hx->h_pre[l], 4 * W, (bf16_t*)hb->h_pre[l], 4 * W, M, 4 * W, hb->cfg.act, 1, s))) return rc;
        }
    }
    SavedView v = own_view(hx);      // ... read by the bf16 kernels: the flash-convention rows as their lse, every row of the last block
    v.lse = hx->lse2.data(); v.lse2 = nullptr; v.tail = false;
    rc = backward_impl<bf16_t>(hb, v, d_emb, B, grad_x, s, /*fp32_dres=*/true);
    hb->saved_B = 0;        // (hb's own saved forward, if any, lost its bf16 tensors to the exports)
    return rc;
}

}  // namespace rvlm

// ---- C ABI: the backward entries ------------------------------------------------------------------------------------------
extern "C" int rvlm_vit_backward_input(rvlm_vit* h, const float* d_emb, int B, float* grad_x,
                                       rvlm_stream_t stream) {
    RVLM_REQUIRE(h && d_emb && grad_x, "rvlm_vit_backward_input: null argument");
    return vit_backward(h, d_emb, B, grad_x, (hipStream_t)stream);
}

extern "C" int rvlm_vit_backward_input_from(rvlm_vit* h, rvlm_vit* h_saved, const float* d_emb, int B, float* grad_x,
                                            rvlm_stream_t stream) {
    RVLM_REQUIRE(h && h_saved && d_emb && grad_x, "rvlm_vit_backward_input_from: null argument");
    RVLM_REQUIRE_SAME_INPUT(h, h_saved, "rvlm_vit_backward_input_from");
    return vit_backward_from(h, h_saved, d_emb, B, grad_x, (hipStream_t)stream);
}

extern "C" int rvlm_vit_backward_params(rvlm_vit* h, const float* d_emb, int B, const rvlm_vit_weights* grads,
                                        int accumulate, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && d_emb && grads && grads->blocks_host, "rvlm_vit_backward_params: null argument");
    if (!h->trainable) return fail(RVLM_ERR_STATE, "rvlm_vit_backward_params: handle was not created trainable");
    int rc = saved_check(h, Reader::Params, B, "rvlm_vit_backward_params"); if (rc) return rc;
    h->next_param_stage = h->L + 2;
    return vit_backward_params(h, d_emb, B, ParamSink{grads, accumulate, 0, h->L + 2}, (hipStream_t)stream);
}

extern "C" int rvlm_vit_backward_params_stages(rvlm_vit* h, const float* d_emb, int B, const rvlm_vit_weights* grads,
                                               int accumulate, int stage_begin, int stage_end, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && d_emb && grads && grads->blocks_host, "rvlm_vit_backward_params_stages: null argument");
    if (!h->trainable) return fail(RVLM_ERR_STATE, "rvlm_vit_backward_params_stages: handle was not created trainable");
    int rc = saved_check(h, Reader::Params, B, "rvlm_vit_backward_params_stages"); if (rc) return rc;
    RVLM_REQUIRE(stage_begin >= 0 && stage_begin < stage_end && stage_end <= h->L + 2,
                 "rvlm_vit_backward_params_stages: need 0 <= stage_begin < stage_end <= layers + 2");
    // stages of one backward hand the residual gradient to each other through the handle: stage k reads what stage
    // k-1 left.  A range that does not continue where the saved forward's backward stands (a skipped or repeated
    // stage) would read stale gradients and write wrong ones silently - refuse it.  Stage 0 restarts the backward.
    if (stage_begin != 0 && stage_begin != h->next_param_stage)
        return fail(RVLM_ERR_STATE, "rvlm_vit_backward_params_stages: stages of one backward must run in order from 0 "
                                    "(stage_begin does not continue the previous call's stage_end)");
    rc = vit_backward_params(h, d_emb, B, ParamSink{grads, accumulate, stage_begin, stage_end}, (hipStream_t)stream);
    h->next_param_stage = rc == RVLM_OK ? stage_end : -1;
    return rc;
}

extern "C" int rvlm_vit_backward_input_tokens(rvlm_vit* h, const float* d_tokens, const float* d_emb, int B, float* grad_x,
                                              rvlm_stream_t stream) {
    RVLM_REQUIRE(h && d_tokens && grad_x, "rvlm_vit_backward_input_tokens: null argument");
    if (h->provider || h->inference_only)
        return fail(RVLM_ERR_STATE, "rvlm_vit_backward_input_tokens: forward-provider and inference-only handles have no backward");
    int rc = saved_check(h, Reader::Tokens, B); if (rc) return rc;
    RVLM_REQUIRE(!d_emb || h->saved_depth == h->L, "rvlm_vit_backward_input_tokens: d_emb needs a token pass of depth == layers");
    return vit_backward_tokens(h, TokSeed{d_tokens, h->saved_depth, h->saved_lnpost}, d_emb, B, grad_x, (hipStream_t)stream);
}

// ---- token parameter pass (RVLM_HAS_TOKEN_TRAINING) ---------------------------------------------------------------------------
static int params_tokens_check(rvlm_vit* h, const float* d_emb, int B, const char* who) {
    if (!h->trainable) return fail(RVLM_ERR_STATE, std::string(who) + ": handle was not created trainable");
    int rc = saved_check(h, Reader::TokensParams, B, who); if (rc) return rc;
    if (d_emb && h->saved_depth != h->L) return fail(RVLM_ERR_ARG, std::string(who) + ": d_emb needs a token pass of depth == layers");
    return RVLM_OK;
}

extern "C" int rvlm_vit_backward_params_tokens(rvlm_vit* h, const float* d_tokens, const float* d_emb, int B,
                                               const rvlm_vit_weights* grads, int accumulate, rvlm_stream_t stream) {
    RVLM_REQUIRE(h && d_tokens && grads && grads->blocks_host, "rvlm_vit_backward_params_tokens: null argument");
    int rc = params_tokens_check(h, d_emb, B, "rvlm_vit_backward_params_tokens"); if (rc) return rc;
    h->next_param_stage = h->L + 2;
    return vit_backward_params_tokens(h, TokSeed{d_tokens, h->saved_depth, h->saved_lnpost}, d_emb, B,
                                      ParamSink{grads, accumulate, 0, h->L + 2}, (hipStream_t)stream);
}

extern "C" int rvlm_vit_backward_params_tokens_stages(rvlm_vit* h, const float* d_tokens, const float* d_emb, int B,
                                                      const rvlm_vit_weights* grads, int accumulate, int stage_begin, int stage_end,
                                                      rvlm_stream_t stream) {
    RVLM_REQUIRE(h && d_tokens && grads && grads->blocks_host, "rvlm_vit_backward_params_tokens_stages: null argument");
    int rc = params_tokens_check(h, d_emb, B, "rvlm_vit_backward_params_tokens_stages"); if (rc) return rc;
    RVLM_REQUIRE(stage_begin >= 0 && stage_begin < stage_end && stage_end <= h->L + 2,
                 "rvlm_vit_backward_params_tokens_stages: need 0 <= stage_begin < stage_end <= layers + 2");
    // (the in-order rule of rvlm_vit_backward_params_stages: the stages hand the residual gradient to each other through the handle)
    if (stage_begin != 0 && stage_begin != h->next_param_stage)
        return fail(RVLM_ERR_STATE, "rvlm_vit_backward_params_tokens_stages: stages of one backward must run in order from 0 "
                                    "(stage_begin does not continue the previous call's stage_end)");
    rc = vit_backward_params_tokens(h, TokSeed{d_tokens, h->saved_depth, h->saved_lnpost}, d_emb, B,
                                    ParamSink{grads, accumulate, stage_begin, stage_end}, (hipStream_t)stream);
    h->next_param_stage = rc == RVLM_OK ? stage_end : -1;
    return rc;
}
