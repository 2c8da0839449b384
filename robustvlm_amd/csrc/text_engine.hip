// rvlm_text: the CLIP text tower (open_clip CLIP.encode_text), forward only - the zero-shot / TeCoA head T = encode_text(prompts) the
// reference builds under no_grad on the frozen model (train/adversarial_training_clip.py:150-180, CLIP_eval/eval_utils.py:63-85).
//
// A handle of its own: it sequences the kernel-level entry points the vision engine is built from (gemm_bf16_nt, x3_split_rows /
// x3_layernorm_fwd / x3_act, gemm_f32, layernorm_fwd, l2_normalize_fwd) plus the text tower's own kernels (attention_causal.hip,
// text_kernels.hip).  Same residual block as the vision tower; what differs is the token-embedding front end, the causal mask and the
// pooling at the EOT token.  The little of engine.hip's precision dispatch that a forward needs is restated in linear().
//
// Active length: the residual stream holds the first `active` positions of every prompt (row n * active + t).  Behind a causal mask
// nothing later can reach the EOT row, so every per-token pass runs on N * active rows instead of N * context.
#include <algorithm>
#include <vector>

#include "text_kernels.h"
#include "../../include/rvlm_kernels.h"

namespace rvlm {
struct TextLayer {
    float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *b_in, *b_out, *b_fc, *b_proj;
    float *w_in = nullptr, *w_out = nullptr, *w_fc = nullptr, *w_proj = nullptr;                  // fp32 storage (reference layout)
    bf16_t *w_in_nk = nullptr, *w_out_nk = nullptr, *w_fc_nk = nullptr, *w_proj_nk = nullptr;      // bf16: [N, K]; x3: [N, 3K] = [hi | lo | hi]
};
}  // namespace rvlm

using namespace rvlm;

struct rvlm_text {
    rvlm_text_config cfg;
    int W, L, H, D, ctx, vocab, maxN, Mp;
    bool bf16 = false, x3 = false;
    size_t esz = 4;                       // activation element size
    std::vector<TextLayer> layers;
    float *tok_emb, *pos, *lnf_w, *lnf_b, *proj;
    float *xa, *xb;                       // [Mp, W] fp32 residual stream (in / mid; the block's output goes back into xa)
    void *ln_out, *qkv, *attn_o, *gact;   // [Mp, W], [Mp, 3W], [Mp, W], [Mp, 4W] in the activation type
    bf16_t* a3 = nullptr;                 // x3: [Mp, 3 * 4W] split copy [hi | hi | lo] of the operand in front of a GEMM
    const void* a3_of = nullptr;          // x3: the fp32 buffer whose split a3 already holds
    float *rows, *pooled, *emb_raw, *inv_norm;   // [maxN, W], [maxN, W], [maxN, D], [maxN]
    int32_t* eot;                         // [maxN]
    std::vector<void*> allocs;
    size_t bytes = 0;
};

namespace rvlm {

static int t_alloc(rvlm_text* h, void** p, size_t bytes) {
    bytes = std::max<size_t>((bytes + 255) & ~(size_t)255, 256);
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(RVLM_ERR_HIP, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    e = hipMemset(*p, 0, bytes);
    if (e != hipSuccess) return fail(RVLM_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    h->allocs.push_back(*p);
    h->bytes += bytes;
    return RVLM_OK;
}
#define T_ALLOC(ptr, bytes) do { int _rc = t_alloc(h, (void**)&(ptr), (bytes)); if (_rc) return _rc; } while (0)

static int t_copy(rvlm_text* h, float** dst, const float* src, size_t n, hipStream_t s) {
    if (!src) return fail(RVLM_ERR_ARG, "rvlm_text: null weight pointer");
    int rc = t_alloc(h, (void**)dst, n * 4);
    if (rc) return rc;
    RVLM_HIP(hipMemcpyAsync(*dst, src, n * 4, hipMemcpyDeviceToDevice, s));
    return RVLM_OK;
}

// the shapes the persistent bf16 GEMM takes for a split-bf16 product (the vision engine's rule, engine.hip x3_takes)
static inline bool t_x3_takes(const rvlm_text* h, int M, int N, int K) {
    return h->x3 && h->a3 && M >= 256 && N % 256 == 0 && K % 128 == 0 && (long)round_up(M, 256) * 3 * K * 2 < (1L << 31);
}

// t3_scratch (x3 only): 4 W * W * 6 bytes for the transposed split form x3_prepare_weight writes next to the one kept
static int t_load_weights(rvlm_text* h, const rvlm_text_weights* w, bf16_t* t3_scratch, hipStream_t s) {
    const int W = h->W;
    int rc;
#define CP(dst, src, n) if ((rc = t_copy(h, &(dst), (src), (n), s))) return rc
    CP(h->tok_emb, w->token_embedding, (size_t)h->vocab * W);
    CP(h->pos, w->positional_embedding, (size_t)h->ctx * W);
    CP(h->lnf_w, w->ln_final_weight, W); CP(h->lnf_b, w->ln_final_bias, W);
    CP(h->proj, w->text_projection, (size_t)W * h->D);
    if (!w->blocks_host) return fail(RVLM_ERR_ARG, "rvlm_text: blocks_host is null");
    for (int l = 0; l < h->L; ++l) {
        const rvlm_vit_block_weights& b = w->blocks_host[l];
        TextLayer& y = h->layers[l];
        CP(y.ln1_w, b.ln_1_weight, W); CP(y.ln1_b, b.ln_1_bias, W);
        CP(y.ln2_w, b.ln_2_weight, W); CP(y.ln2_b, b.ln_2_bias, W);
        CP(y.b_in, b.attn_in_proj_bias, 3 * W); CP(y.b_out, b.attn_out_proj_bias, W);
        CP(y.b_fc, b.mlp_c_fc_bias, 4 * W); CP(y.b_proj, b.mlp_c_proj_bias, W);
        struct { bf16_t** nk; float** f32; const float* src; int rows, cols; } ws[4] = {
            {&y.w_in_nk, &y.w_in, b.attn_in_proj_weight, 3 * W, W}, {&y.w_out_nk, &y.w_out, b.attn_out_proj_weight, W, W},
            {&y.w_fc_nk, &y.w_fc, b.mlp_c_fc_weight, 4 * W, W}, {&y.w_proj_nk, &y.w_proj, b.mlp_c_proj_weight, W, 4 * W}};
        for (auto& q : ws) {
            if (!q.src) return fail(RVLM_ERR_ARG, "rvlm_text: null weight pointer");
            if (h->bf16) {
                // rows padded to the GEMM's 128-row operand tiles (zero-filled)
                if ((rc = t_alloc(h, (void**)q.nk, (size_t)round_up(q.rows, 128) * q.cols * 2))) return rc;
                if ((rc = convert_f32_to_bf16(q.src, q.cols, *q.nk, q.cols, q.rows, q.cols, 0, s))) return rc;
            } else {
                CP(*q.f32, q.src, (size_t)q.rows * q.cols);
                if (h->x3) {      // [W_hi | W_lo | W_hi]; x3_prepare_weight also writes the dgrad operand (W^T), which a forward never reads
                    if ((rc = t_alloc(h, (void**)q.nk, (size_t)q.rows * q.cols * 6))) return rc;
                    if ((rc = x3_prepare_weight(q.src, q.rows, q.cols, *q.nk, t3_scratch, s))) return rc;
                }
            }
        }
    }
#undef CP
    return RVLM_OK;
}

// out[M, N] = epi(A[M, K] @ Wt[N, K]^T + bias): epi EPI_BF16 (plain), EPI_BF16_ACT (activation), EPI_F32_RESID (+ residual, fp32 out) -
// the forward half of engine.hip's linear_fwd.  The GEMM descriptors carry NO split-K scratch: every output element is then one
// k-ordered accumulation whatever M is, so neither the chunking of a batch nor the active length changes the bits of a prompt.
static int linear(rvlm_text* h, hipStream_t s, const void* A, long lda, int M, int N, int K, const float* w_f32, const bf16_t* w_nk,
                  const float* bias, int epi, void* out, long ldo, const float* residual) {
    if (h->bf16) {
        GemmBf16 g;
        g.A = (const bf16_t*)A; g.lda = lda; g.Bw = w_nk; g.ldb = K; g.M = M; g.N = N; g.K = K;
        g.a_rows = (int)round_up(M, 128); g.epi = epi; g.bias = bias; g.out = out; g.ldo = ldo;
        g.residual = residual; g.act = h->cfg.act;
        return gemm_bf16_nt(g, s);
    }
    if (t_x3_takes(h, M, N, K) && w_nk) {
        // A3 = [A_hi | A_hi | A_lo] against W3 = [W_hi | W_lo | W_hi]: one bf16 GEMM of contraction length 3 K, fp32 epilogue; the
        // activation of fc1 is its own pass over the fp32 pre-activation and writes fc2's split operand directly
        int rc = RVLM_OK;
        if (h->a3_of != A && (rc = x3_split_rows((const float*)A, lda, h->a3, M, (int)round_up(M, 256), K, s))) return rc;
        h->a3_of = nullptr;
        GemmBf16 g;
        g.A = h->a3; g.lda = 3L * K; g.Bw = w_nk; g.ldb = 3L * K; g.M = M; g.N = N; g.K = 3 * K;
        g.a_rows = (int)round_up(M, 256); g.bias = bias; g.residual = residual;
        g.epi = residual ? EPI_F32_RESID : EPI_F32;
        g.out = out; g.ldo = ldo; g.act = h->cfg.act;
        if ((rc = gemm_bf16_nt(g, s))) return rc;
        if (epi == EPI_BF16_ACT) {
            // (fc2 is [M, N] x [K, N]^T: only if IT takes the split path may the activation skip the fp32 buffer)
            const bool fuse = t_x3_takes(h, M, K, N);
            if ((rc = x3_act((const float*)out, ldo, (float*)out, ldo, fuse ? h->a3 : nullptr, M, (int)round_up(M, 256), N, h->cfg.act, 0, s)))
                return rc;
            if (fuse) h->a3_of = out;
        }
        return RVLM_OK;
    }
    GemmF32 g;
    g.A = (const float*)A; g.sam = lda; g.sak = 1;
    g.B = w_f32; g.sbn = K; g.sbk = 1;
    g.C = (float*)out; g.scm = ldo; g.scn = 1;
    g.M = M; g.N = N; g.K = K; g.bias = bias; g.residual = residual;
    if (epi == EPI_BF16_ACT) g.act = h->cfg.act;
    return gemm_f32(g, s);
}

// LayerNorm in front of a linear of N_next outputs: x3 writes that linear's split operand itself where the kernel covers the width
static int ln_fwd(rvlm_text* h, hipStream_t s, const float* x, const float* gamma, const float* beta, int M, int N_next) {
    const int W = h->W;
    int rc = RVLM_OK;
    if (t_x3_takes(h, M, N_next, W) && x3_layernorm_fwd(x, W, gamma, beta, h->a3, nullptr, nullptr, M, (int)round_up(M, 256), W, s, &rc)) {
        if (rc == RVLM_OK) h->a3_of = h->ln_out;
        return rc;
    }
    if (h->bf16) return layernorm_fwd<bf16_t>(x, W, gamma, beta, (bf16_t*)h->ln_out, W, nullptr, nullptr, M, W, s);
    return layernorm_fwd<float>(x, W, gamma, beta, (float*)h->ln_out, W, nullptr, nullptr, M, W, s);
}

static int text_forward(rvlm_text* h, const int32_t* tokens, int N, int A, int normalize, float* out_emb, uint32_t* flags, hipStream_t s) {
    const int W = h->W, D = h->D, M = N * A;
    int rc;
    h->a3_of = nullptr;
    if ((rc = text_embed_fwd(tokens, h->tok_emb, h->pos, h->xa, h->eot, flags, N, h->ctx, A, h->vocab, W, s))) return rc;
    for (int l = 0; l < h->L; ++l) {
        TextLayer& y = h->layers[l];
        if ((rc = ln_fwd(h, s, h->xa, y.ln1_w, y.ln1_b, M, 3 * W))) return rc;
        if ((rc = linear(h, s, h->ln_out, W, M, 3 * W, W, y.w_in, y.w_in_nk, y.b_in, EPI_BF16, h->qkv, 3 * W, nullptr))) return rc;
        if (h->bf16) rc = attn_causal_fwd_bf16((const bf16_t*)h->qkv, 3 * W, (bf16_t*)h->attn_o, W, N, h->H, A, A, s);
        else rc = attn_causal_fwd_f32((const float*)h->qkv, 3 * W, (float*)h->attn_o, W, N, h->H, A, A, s);
        if (rc) return rc;
        if ((rc = linear(h, s, h->attn_o, W, M, W, W, y.w_out, y.w_out_nk, y.b_out, EPI_F32_RESID, h->xb, W, h->xa))) return rc;
        if ((rc = ln_fwd(h, s, h->xb, y.ln2_w, y.ln2_b, M, 4 * W))) return rc;
        if ((rc = linear(h, s, h->ln_out, W, M, 4 * W, W, y.w_fc, y.w_fc_nk, y.b_fc, EPI_BF16_ACT, h->gact, 4 * W, nullptr))) return rc;
        if ((rc = linear(h, s, h->gact, 4 * W, M, W, 4 * W, y.w_proj, y.w_proj_nk, y.b_proj, EPI_F32_RESID, h->xa, W, h->xb))) return rc;
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
    for (void* p : h->allocs) (void)hipFree(p);
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
    h->bf16 = cfg->precision == RVLM_PREC_BF16; h->x3 = cfg->precision == RVLM_PREC_F32X3;
    h->esz = h->bf16 ? 2 : 4;
    h->layers.resize(h->L);
    hipStream_t s = (hipStream_t)stream;
    auto body = [&]() -> int {
        int rc;
        const size_t mp = (size_t)h->Mp, e = h->esz;
        T_ALLOC(h->xa, mp * W * 4); T_ALLOC(h->xb, mp * W * 4);
        T_ALLOC(h->ln_out, mp * W * e); T_ALLOC(h->qkv, mp * 3 * W * e); T_ALLOC(h->attn_o, mp * W * e); T_ALLOC(h->gact, mp * 4 * W * e);
        if (h->x3) T_ALLOC(h->a3, mp * 3 * 4 * W * 2);
        T_ALLOC(h->rows, (size_t)h->maxN * W * 4); T_ALLOC(h->pooled, (size_t)h->maxN * W * 4);
        T_ALLOC(h->emb_raw, (size_t)h->maxN * h->D * 4); T_ALLOC(h->inv_norm, (size_t)h->maxN * 4);
        T_ALLOC(h->eot, (size_t)h->maxN * 4);
        bf16_t* t3 = nullptr;
        if (h->x3) RVLM_HIP(hipMalloc((void**)&t3, (size_t)4 * W * W * 6));
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

extern "C" size_t rvlm_text_workspace_bytes(const rvlm_text* h) { return h ? h->bytes : 0; }

extern "C" int rvlm_text_encode(rvlm_text* h, const int32_t* tokens, int N, int active_len, int normalize, float* out_emb, uint32_t* flags,
                                rvlm_stream_t stream) {
    RVLM_REQUIRE(h && tokens && out_emb, "rvlm_text_encode: null argument");
    RVLM_REQUIRE(N >= 1 && N <= h->maxN, "rvlm_text_encode: N outside [1, max_batch]");
    RVLM_REQUIRE(active_len >= 0 && active_len <= h->ctx, "rvlm_text_encode: active_len outside [0, context]");
    return text_forward(h, tokens, N, active_len ? active_len : h->ctx, normalize, out_emb, flags, (hipStream_t)stream);
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
