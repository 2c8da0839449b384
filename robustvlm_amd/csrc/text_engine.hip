// rvlm_text: the CLIP text tower (open_clip CLIP.encode_text), forward only - the zero-shot / TeCoA head T = encode_text(prompts) the
// reference builds under no_grad on the frozen model (train/adversarial_training_clip.py:150-180, CLIP_eval/eval_utils.py:63-85).
//
// A handle of its own on the vision engine's building blocks: the linear layer with its dispatch on precision, the block-weight record
// and the allocator (linear.h), layernorm_fwd / gemm_f32 / l2_normalize_fwd, plus the text tower's own kernels (attention_causal.hip,
// text_kernels.hip).  Same residual block as the vision tower; what differs is the token-embedding front end, the causal mask and the
// pooling at the EOT token.
//
// Active length: the residual stream holds the first `active` positions of every prompt (row n * active + t).  Behind a causal mask
// nothing later can reach the EOT row, so every per-token pass runs on N * active rows instead of N * context.
#include <algorithm>
#include <vector>

#include "linear.h"
#include "text_kernels.h"
#include "../../include/rvlm_kernels.h"

using namespace rvlm;

struct rvlm_text {
    rvlm_text_config cfg;
    int W, L, H, D, ctx, vocab, maxN, Mp;
    // the precision (lin.bf16, lin.x3) and the x3 split operand.  NO split-K scratch (lin.splitk stays null): every output element is
    // then one k-ordered accumulation whatever M is, so neither the chunking of a batch nor the active length changes the bits of a prompt
    LinearCtx lin;
    size_t esz = 4;                       // activation element size
    std::vector<Layer> layers;            // (forward only: the *_t forms stay null)
    float *tok_emb, *pos, *lnf_w, *lnf_b, *proj;
    float *xa, *xb;                       // [Mp, W] fp32 residual stream (in / mid; the block's output goes back into xa)
    void *ln_out, *qkv, *attn_o, *gact;   // [Mp, W], [Mp, 3W], [Mp, W], [Mp, 4W] in the activation type
    float *rows, *pooled, *emb_raw, *inv_norm;   // [maxN, W], [maxN, W], [maxN, D], [maxN]
    int32_t* eot;                         // [maxN]
    DeviceArena arena;
};

namespace rvlm {

// t3_scratch (x3 only): 4 W * W * 6 bytes for the transposed split form x3_prepare_weight writes next to the one kept
static int t_load_weights(rvlm_text* h, const rvlm_text_weights* w, bf16_t* t3_scratch, hipStream_t s) {
    const int W = h->W;
    int rc;
#define CP(dst, src, n) if ((rc = copy_f32(h->arena, &(dst), (src), (n), s, true, "rvlm_text"))) return rc
    CP(h->tok_emb, w->token_embedding, (size_t)h->vocab * W);
    CP(h->pos, w->positional_embedding, (size_t)h->ctx * W);
    CP(h->lnf_w, w->ln_final_weight, W); CP(h->lnf_b, w->ln_final_bias, W);
    CP(h->proj, w->text_projection, (size_t)W * h->D);
    if (!w->blocks_host) return fail(RVLM_ERR_ARG, "rvlm_text: blocks_host is null");
    for (int l = 0; l < h->L; ++l) {
        const rvlm_vit_block_weights& b = w->blocks_host[l];
        Layer& y = h->layers[l];
        if ((rc = load_block_vectors(h->arena, y, b, W, s, true, "rvlm_text"))) return rc;
        for (auto& q : block_weights(y, b, W)) {      // the [N, K] forms only: a forward never reads W^T
            if (!q.src) return fail(RVLM_ERR_ARG, "rvlm_text: null weight pointer");
            if (h->lin.bf16) {
                // rows padded to the GEMM's 128-row operand tiles (zero-filled)
                if ((rc = dev_alloc(h->arena, (void**)q.nk, (size_t)round_up(q.rows, 128) * q.cols * 2))) return rc;
                if ((rc = convert_f32_to_bf16(q.src, q.cols, *q.nk, q.cols, q.rows, q.cols, 0, s))) return rc;
            } else {
                CP(*q.f32, q.src, (size_t)q.rows * q.cols);
                if (h->lin.x3) {      // [W_hi | W_lo | W_hi]; x3_prepare_weight also writes the dgrad operand (W^T), which a forward never reads
                    if ((rc = dev_alloc(h->arena, (void**)q.nk, (size_t)q.rows * q.cols * 6))) return rc;
                    if ((rc = x3_prepare_weight(q.src, q.rows, q.cols, *q.nk, t3_scratch, s))) return rc;
                }
            }
        }
    }
#undef CP
    return RVLM_OK;
}

// LayerNorm in front of a linear of N_next outputs: x3 writes that linear's split operand itself where the kernel covers the width
template <typename T>
static int ln_fwd(rvlm_text* h, hipStream_t s, const float* x, const float* gamma, const float* beta, int M, int N_next) {
    const int W = h->W;
    int rc = RVLM_OK;
    if (ln_into_split(h->lin, s, x, gamma, beta, h->ln_out, nullptr, nullptr, M, N_next, W, &rc)) return rc;
    return layernorm_fwd<T>(x, W, gamma, beta, (T*)h->ln_out, W, nullptr, nullptr, M, W, s);
}

// T: the activation type (bf16_t on a bf16 handle, float on fp32 storage - fp32 and x3)
template <typename T>
static int text_forward(rvlm_text* h, const int32_t* tokens, int N, int A, int normalize, float* out_emb, uint32_t* flags, hipStream_t s) {
    const int W = h->W, D = h->D, M = N * A;
    int rc;
    h->lin.a3_of = nullptr;
    if ((rc = text_embed_fwd(tokens, h->tok_emb, h->pos, h->xa, h->eot, flags, N, h->ctx, A, h->vocab, W, s))) return rc;
    for (int l = 0; l < h->L; ++l) {
        Layer& y = h->layers[l];
        if ((rc = ln_fwd<T>(h, s, h->xa, y.ln1_w, y.ln1_b, M, 3 * W))) return rc;
        if ((rc = linear_fwd<T>(h->lin, s, h->ln_out, W, M, 3 * W, W, y.w_in, y.w_in_nk, y.b_in, EPI_BF16, h->qkv, 3 * W, nullptr, nullptr))) return rc;
        if (h->lin.bf16) rc = attn_causal_fwd_bf16((const bf16_t*)h->qkv, 3 * W, (bf16_t*)h->attn_o, W, N, h->H, A, A, s);
        else rc = attn_causal_fwd_f32((const float*)h->qkv, 3 * W, (float*)h->attn_o, W, N, h->H, A, A, s);
        if (rc) return rc;
        if ((rc = linear_fwd<T>(h->lin, s, h->attn_o, W, M, W, W, y.w_out, y.w_out_nk, y.b_out, EPI_F32_RESID, h->xb, W, nullptr, h->xa))) return rc;
        if ((rc = ln_fwd<T>(h, s, h->xb, y.ln2_w, y.ln2_b, M, 4 * W))) return rc;
        if ((rc = linear_fwd<T>(h->lin, s, h->ln_out, W, M, 4 * W, W, y.w_fc, y.w_fc_nk, y.b_fc, EPI_BF16_ACT, h->gact, 4 * W, nullptr, nullptr))) return rc;
        if ((rc = linear_fwd<T>(h->lin, s, h->gact, 4 * W, M, W, 4 * W, y.w_proj, y.w_proj_nk, y.b_proj, EPI_F32_RESID, h->xa, W, nullptr, h->xb)))
            return rc;
    }
    // head: ln_final on the EOT row of every prompt only, @ text_projection, optional L2 normalisation
    if ((rc = text_gather_eot(h->xa, h->eot, h->rows, N, A, W, s))) return rc;
    if ((rc = layernorm_fwd<float>(h->rows, W, h->lnf_w, h->lnf_b, h->pooled, W, nullptr, nullptr, N, W, s))) return rc;
    GemmF32 g;
    g.A = h->pooled; g.sam = W; g.sak = 1;
    g.B = h->proj; g.sbn = 1; g.sbk = D;
    g.C = normalize ? h->emb_raw : out_emb; g.scm = D; g.scn = 1;
    g.M = N; g.N = D; g.K = W;
    if ((rc = gemm_f32(g, s))) return rc;
    if (normalize) return l2_normalize_fwd(h->emb_raw, out_emb, h->inv_norm, N, D, s);
    return RVLM_OK;
}

}  // namespace rvlm

extern "C" int rvlm_text_destroy(rvlm_text* h) {
    if (!h) return RVLM_OK;
    (void)hipDeviceSynchronize();
    for (void* p : h->arena.allocs) (void)hipFree(p);
    delete h;
    return RVLM_OK;
}

extern "C" int rvlm_text_create(const rvlm_text_config* cfg, const rvlm_text_weights* weights, rvlm_stream_t stream, rvlm_text** out) {
    RVLM_REQUIRE(cfg && weights && out, "rvlm_text_create: null argument");
    *out = nullptr;
    RVLM_REQUIRE(cfg->heads > 0 && cfg->width == cfg->heads * 64, "rvlm_text_create: head_dim must be 64");
    RVLM_REQUIRE(cfg->vocab > 0 && cfg->layers > 0 && cfg->out_dim > 0, "rvlm_text_create: vocab, layers and out_dim must be positive");
    RVLM_REQUIRE(cfg->out_dim % 4 == 0, "rvlm_text_create: out_dim must be a multiple of 4");
    RVLM_REQUIRE(cfg->act == RVLM_ACT_QUICK_GELU || cfg->act == RVLM_ACT_GELU, "rvlm_text_create: unknown activation");
    RVLM_REQUIRE(cfg->precision == RVLM_PREC_F32 || cfg->precision == RVLM_PREC_BF16 || cfg->precision == RVLM_PREC_F32X3,
                 "rvlm_text_create: unknown precision");
    if (cfg->context < 1 || cfg->context > 96)
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_text_create: the causal attention kernels cover context <= 96 (CLIP: 77)");
    const int max_batch = cfg->max_batch > 0 ? cfg->max_batch : 1024;
    const int W = cfg->width;
    const long Mp = round_up((long)max_batch * cfg->context, 256);
    RVLM_REQUIRE(Mp * 4L * W < (1L << 31), "rvlm_text_create: max_batch * context * 4 * width exceeds 2^31 elements");
    // x3: a width the persistent GEMM takes must keep fc2 (K = 4 W) on it for every batch size up to max_batch - its split operand
    // is bounded by the GEMM's 31-bit byte offsets; past that bound fc2 alone would drop to the fp32 tiles
    if (cfg->precision == RVLM_PREC_F32X3 && W % 256 == 0 && Mp * 3 * 4L * W * 2 >= (1L << 31))
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_text_create: max_batch too large for the split-bf16 operand buffer (round_up(max_batch * "
                                          "context, 256) * 12 * width * 2 bytes must stay below 2^31): lower max_batch, the caller chunks");
    rvlm_text* h = new rvlm_text();
    h->cfg = *cfg; h->cfg.max_batch = max_batch;
    h->W = W; h->L = cfg->layers; h->H = cfg->heads; h->D = cfg->out_dim; h->ctx = cfg->context; h->vocab = cfg->vocab;
    h->maxN = max_batch; h->Mp = (int)Mp;
    h->lin.bf16 = cfg->precision == RVLM_PREC_BF16; h->lin.x3 = cfg->precision == RVLM_PREC_F32X3; h->lin.act = cfg->act;
    h->esz = h->lin.bf16 ? 2 : 4;
    h->layers.resize(h->L);
    hipStream_t s = (hipStream_t)stream;
    auto body = [&]() -> int {
        int rc;
        const size_t mp = (size_t)h->Mp, e = h->esz;
        ALLOC(h->xa, mp * W * 4); ALLOC(h->xb, mp * W * 4);
        ALLOC(h->ln_out, mp * W * e); ALLOC(h->qkv, mp * 3 * W * e); ALLOC(h->attn_o, mp * W * e); ALLOC(h->gact, mp * 4 * W * e);
        if (h->lin.x3) ALLOC(h->lin.a3, mp * 3 * 4 * W * 2);
        ALLOC(h->rows, (size_t)h->maxN * W * 4); ALLOC(h->pooled, (size_t)h->maxN * W * 4);
        ALLOC(h->emb_raw, (size_t)h->maxN * h->D * 4); ALLOC(h->inv_norm, (size_t)h->maxN * 4);
        ALLOC(h->eot, (size_t)h->maxN * 4);
        bf16_t* t3 = nullptr;
        if (h->lin.x3) RVLM_HIP(hipMalloc((void**)&t3, (size_t)4 * W * W * 6));
        rc = t_load_weights(h, weights, t3, s);
        const hipError_t es = hipStreamSynchronize(s);
        if (t3) (void)hipFree(t3);
        if (rc) return rc;
        RVLM_HIP(es);
        return RVLM_OK;
    };
    const int rc = body();
    if (rc) {
        const std::string msg = rvlm_last_error();
        rvlm_text_destroy(h);
        return fail(rc, msg);
    }
    *out = h;
    return RVLM_OK;
}

extern "C" size_t rvlm_text_workspace_bytes(const rvlm_text* h) { return h ? h->arena.bytes : 0; }

extern "C" int rvlm_text_encode(rvlm_text* h, const int32_t* tokens, int N, int active_len, int normalize, float* out_emb, uint32_t* flags,
                                rvlm_stream_t stream) {
    RVLM_REQUIRE(h && tokens && out_emb, "rvlm_text_encode: null argument");
    RVLM_REQUIRE(N >= 1 && N <= h->maxN, "rvlm_text_encode: N outside [1, max_batch]");
    RVLM_REQUIRE(active_len >= 0 && active_len <= h->ctx, "rvlm_text_encode: active_len outside [0, context]");
    const int A = active_len ? active_len : h->ctx;
    return h->lin.bf16 ? text_forward<bf16_t>(h, tokens, N, A, normalize, out_emb, flags, (hipStream_t)stream)
                       : text_forward<float>(h, tokens, N, A, normalize, out_emb, flags, (hipStream_t)stream);
}

// ---- kernel-level test hooks (include/rvlm_kernels.h) ------------------------------------------
extern "C" int rvlm_k_attn_causal_fwd_bf16(const uint16_t* qkv, uint16_t* o, int B, int H, int S, int active_len, rvlm_stream_t stream) {
    return attn_causal_fwd_bf16((const bf16_t*)qkv, 3L * 64 * H, (bf16_t*)o, 64L * H, B, H, S, active_len ? active_len : S, (hipStream_t)stream);
}
extern "C" int rvlm_k_attn_causal_fwd_f32(const float* qkv, float* o, int B, int H, int S, int active_len, rvlm_stream_t stream) {
    return attn_causal_fwd_f32(qkv, 3L * 64 * H, o, 64L * H, B, H, S, active_len ? active_len : S, (hipStream_t)stream);
}
extern "C" int rvlm_k_text_embed(const int32_t* tokens, const float* token_embedding, const float* positional_embedding, float* x, int32_t* eot,
                                 uint32_t* flags, int N, int context, int active_len, int vocab, int W, rvlm_stream_t stream) {
    return text_embed_fwd(tokens, token_embedding, positional_embedding, x, eot, flags, N, context, active_len ? active_len : context, vocab, W,
                          (hipStream_t)stream);
}
