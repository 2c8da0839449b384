// The fixed-function "ViT forward + input-gradient" engine and the device-resident PGD / APGD loops: what its sources share.
//
// Not an autograd graph: one handle owns the converted weights and a workspace sized for max_batch
// (MI355X has 288 GB of HBM3E, so every activation the dgrad chain needs is simply kept resident:
// ~19 GB at ViT-L/14, B=128, bf16), and forward / backward are fixed launch sequences on the caller's
// stream with no host synchronisation.  Only the INPUT gradient is produced (no wgrad, no saved
// linear inputs), exactly what torch.autograd.grad(loss, perturbation) asks for in
// train/pgd_train.py:38 and train/apgd_train.py:185,295.
//
// Sources: engine_create.hip, engine_forward.hip, engine_backward.hip, engine_attacks.hip (what each holds: DESIGN.md section 1).  A
// function that crosses one of them is declared at the end of this file; everything else is static in its file.
#pragma once
#include <cstring>
#include <string>
#include <vector>

#include "linear.h"

namespace rvlm {

// What kind of forward a handle holds saved (meaningful while saved_B > 0).  Input and Params are the values of the C ABI's
// save_for_backward (1, 2); the other two are set by the forward itself.
enum class Saved {
    None = 0,
    Input = 1,      // activations of the input-gradient chain
    Params = 2,     // ... and the inputs of every linear layer (trainable handles)
    ForPeer = 3,    // run for another handle's backward (FwdPass::peer): a provider's single slots / no probabilities kept
    Tokens = 4,     // a token pass: saved_depth blocks, every row of the last one, token rows as outputs
    TokensParams = 5,   // ... and the inputs of every linear layer of those blocks (trainable handles): a superset of Tokens
};
static inline bool is_token_pass(Saved m) { return m == Saved::Tokens || m == Saved::TokensParams; }

struct ProfRec { int cls; hipEvent_t a, b; };
struct ProfAcc { double ms = 0, flops = 0, bytes = 0; int64_t n = 0; };

}  // namespace rvlm

using namespace rvlm;

struct rvlm_vit {
    rvlm_vit_config cfg;
    int S, G, W, L, H, D, P, img, Kp, Kpad, maxB, Mp, Mp0;
    LinearCtx lin;       // the precision (lin.bf16, lin.x3), the x3 split operand and the split-K slabs: what the linear layers read (linear.h)
    size_t esz;  // activation element size
    std::vector<Layer> layers;
    float *cls, *pos, *proj, *lnpre_w, *lnpre_b, *lnpost_w, *lnpost_b, *conv_f32;
    bf16_t *conv_nk, *conv_t;
    // activations
    void* A0;            // [Mp0, Kpad] T
    float* patch_out;    // [Mp0, W] f32
    std::vector<float*> xs;      // 2L+1 x [Mp, W] f32 residual stream
    float *st_mean, *st_rstd;    // [(2L+2) * Mp]
    void* ln_out;        // [Mp, W] T
    std::vector<void*> qkv;      // L x [Mp, 3W] T
    std::vector<void*> attn_o;   // L x [Mp, W] T
    std::vector<float*> lse;     // L x [B*H*Sp]
    std::vector<float*> lse2;    // fp32 storage: L x [B*H*Sp], the flash kernels' log-sum-exp rows, written by the softmax pass of a
                                 // saving forward for the handoff to a bf16 handle's backward (vit_backward_from)
    // A saving forward run FOR a bf16 handle (the handoff, FwdPass::peer) writes that handle's bf16 qkv / attention output / act'(fc1)
    // as it goes.  What was exported is remembered per saved forward.
    unsigned long long uid = 0;          // unique per created handle (never reused, unlike an address)
    unsigned long long exported_to = 0;  // uid of the handle the saved forward's bf16 qkv / attention output / lse rows already sit in
    bool exported_dact = false;          // ... and its act'(fc1)
    // Non-saving forwards on the flash kernel too (rvlm_vit_set_flash_inference).  OFF by default: a handle's saving and non-saving
    // forwards must agree BIT FOR BIT - FARE's loss at delta = 0 is |phi(x) - phi(x)|^2 = 0 with a zero gradient exactly (apgd_train
    // starts there, train/apgd_train.py:157-160), and 1e-7 of rounding difference between two attention paths turns that into a
    // random sign pattern.  ON for the fp32-storage handle of a handoff engine, whose saving forwards (run for the peer) are flash.
    bool flash_inference = false;
    // fp32-storage handle at a sequence length the fp32 flash BACKWARD takes (S = 257): every attention of this handle - saving or not,
    // forward and backward - runs on the flash kernels (attention_f32.hip); no probabilities are kept or allocated (13 GB at ViT-L/14,
    // B = 128) and saving / non-saving forwards agree bit for bit by construction.
    bool own_flash = false;
    // bf16 handles, attack path (backward_impl): the residual-GRADIENT stream is the bf16 buffer only - the LayerNorm backward reads it
    // to accumulate and writes it back, 10 instead of 16 B per element and pass (no fp32 copy).  What it costs: an accumulator of 49
    // terms rounded to 8 bits of mantissa 49 times - measured by the emulation (oracle/split_bf16_emulation.py, arm
    // f32fwd-bf16bwd-bf16res: first-step sign agreement of a bf16 backward 0.9982 -> 0.9961, CLIP-like 0.9977 -> 0.9945) and by the
    // full-size tests; the handoff's backward (the faithful first iteration) and the training step keep the fp32 stream.
    // RVLM_DRES_FP32=1 (read at creation) keeps it everywhere.
    bool lp_dres = false;
    std::vector<void*> h_pre;    // L x [Mp, 4W] T
    void* g_act;         // [Mp, 4W] T
    float *pooled, *emb_raw, *inv_norm;   // [maxB, W], [maxB, D], [maxB]
    // backward scratch
    float* dres;  void* dres_lp;  void* d_o;  void* dqkv;  void* dh;  void* d_ln;  void* d_patch;
    float* dA0;   float* dsum;   float *d_raw, *d_pooled;
    float* dscores;            // fp32 mode: dP / dS of one block [B, H, S, round_up(S, 4)] (the probabilities live in lse[l])
    // class-token tail (bf16 mode): in the last block only the class token's row is live downstream of the attention
    // (the output is ln_post(x[:, 0]) @ proj), so out-proj / MLP / their LayerNorm run on B rows and the attention on
    // the class query only.  Row b of the B-row intermediates is image b; x rows stay in place (stride S*W).
    bool cls_tail = false;
    float* lse_cls = nullptr;
    float* red_scratch = nullptr;   // partial column sums of the training step
    size_t red_floats = 0;
    // training (cfg.trainable): inputs of every linear layer + embedding tokens + transpose scratch
    bool trainable = false;
    bool inference_only = false;
    bool provider = false;       // cfg.trainable == -2: an fp32-storage handle whose saving forwards are all run FOR a bf16 handle
                                 // (rvlm_vit_forward_for / rvlm_pgd_run_mixed_fwd) on the flash attention: the fp32 residual stream, the
                                 // LayerNorm statistics and the log-sum-exp rows are kept per block; qkv, attention output, fc1
                                 // pre-activation and probabilities have ONE slot (their bf16 forms are written into the consumer as
                                 // the forward goes), and there is no backward scratch: 51 -> 13 GiB at ViT-L/14, B = 128
    std::vector<void*> ln1_out, ln2_out, g_act_l;   // L x [Mp,W], [Mp,W], [Mp,4W] T
    float *tokens, *dtok;      // [Mp, W] f32
    void *tA, *tB;             // bf16 mode: transposed operands of the wgrad GEMMs the copy-free form does not take
                               // (conv1, widths that are no multiple of 256, fewer than 256 tokens); t_elems elements each
    long Mpt = 0;
    size_t t_elems = 0;        // bf16 elements of tA (= of tB)
    // Input size (rvlm_vit_set_input_size): images and perturbations are [B, 3, in_h, in_w]; where that is not (img, img) the
    // bicubic resize to (img, img) is part of the model, fused into the patch embedding both ways (resize_kernels.hip).
    int in_h = 0, in_w = 0;    // = img when no resize is active
    bool resize = false;
    ResizeAxis rs_h, rs_w;     // device tables of (in_h -> img), (in_w -> img) while `resize`
    // attack state
    float* img_buf[5];         // [maxB*3*img*img] (covers every input size up to the model's own)
    float *emb, *d_emb, *loss_ps, *loss_scalar, *loss_scratch;
    float *ap_loss_steps, *ap_loss_best, *ap_loss_best_lc, *ap_reduced_lc, *ap_step;
    uint8_t *ap_acc, *ap_pred, *ap_f0, *ap_f1, *ap_f2;
    double ap_rho = 0.75;      // APGDAttack's oscillation threshold (rvlm_vit_set_apgd_rho)
    size_t loss_scratch_floats;
    // bookkeeping
    DeviceArena arena;
    int saved_B = 0;
    Saved saved_mode = Saved::None;
    int next_param_stage = 0;   // rvlm_vit_backward_params_stages: the stage the saved forward's backward continues at
    bool saved_norm = false;
    // token passes (rvlm_vit_forward_tokens): Saved::Tokens = the saved forward ran `saved_depth` blocks, every row of the last one
    // (no class-token tail), and its outputs were the token rows (ln_post applied or not) - differentiated by
    // rvlm_vit_backward_input_tokens only; Saved::TokensParams (save = 2) also by rvlm_vit_backward_params_tokens.  What only the
    // ln_post form needs is allocated by the first pass that asks for it.
    int saved_depth = 0;
    bool saved_lnpost = false;
    float *tok_mean = nullptr, *tok_rstd = nullptr;   // [Mp] statistics of ln_post over every token row
    float* tok_buf = nullptr;                         // [Mp, W] ln_post(tokens) of the fused loss loop, differentiated in place
    // profiling
    bool prof = false;
    std::vector<ProfRec> recs;
    std::vector<std::string> cls_names;
    std::vector<ProfAcc> accs;
    std::vector<double> cls_flops, cls_bytes;

    float* mean_at(int i) { return st_mean + (size_t)i * Mp; }
    float* rstd_at(int i) { return st_rstd + (size_t)i * Mp; }
};

namespace rvlm {

// ---- profiling ------------------------------------------------------------------------------
static inline int prof_class(rvlm_vit* h, const char* name) {
    for (size_t i = 0; i < h->cls_names.size(); ++i) if (h->cls_names[i] == name) return (int)i;
    h->cls_names.push_back(name);
    h->accs.emplace_back();
    return (int)h->cls_names.size() - 1;
}
struct ProfScope {
    rvlm_vit* h; hipStream_t s; int idx = -1;
    ProfScope(rvlm_vit* h_, hipStream_t s_, const char* name, double flops, double bytes) : h(h_), s(s_) {   // (null name: no scope)
        if (!h->prof || !name) return;
        ProfRec r;
        r.cls = prof_class(h, name);
        (void)hipEventCreate(&r.a); (void)hipEventCreate(&r.b);
        (void)hipEventRecord(r.a, s);
        h->recs.push_back(r);
        idx = (int)h->recs.size() - 1;
        h->accs[r.cls].flops += flops;
        h->accs[r.cls].bytes += bytes;
        h->accs[r.cls].n += 1;
    }
    ~ProfScope() { if (idx >= 0) (void)hipEventRecord(h->recs[idx].b, s); }
};
#define PROF(name, flops, bytes) ProfScope _ps(h, s, name, (double)(flops), (double)(bytes))
// ... recorded only where `on` holds (the walkers: a pass that records no scopes; a step the class-token tail accounts coarsely)
#define PROF_IF(on, name, flops, bytes) ProfScope _ps(h, s, (on) ? name : nullptr, (double)(flops), (double)(bytes))

// What a forward pass decides once, at its top (forward_impl): the bf16 handle it runs for (the handoff) or none, and whether its
// attention runs as the fp32 flash kernel.
struct FwdPass { rvlm_vit* peer = nullptr; bool flash = false; };

// ---- token passes ---------------------------------------------------------------------------------
// forward: run `depth` blocks (all rows), hand out the token rows; the head runs at depth == L only
struct TokPass { int depth; int ln_post; float* out_tokens; };
// backward: the residual-gradient stream starts from d_tokens [B, S, W] at block depth - 1 (d_tokens == null: the loss kernel
// has written the stream already)
struct TokSeed { const float* d_tokens; int depth; int ln_post; };

// ---- row geometry of a transformer block ---------------------------------------------------------
// Which rows of a block are live downstream of its attention, as the (M, leading dimension) the steps after the attention run on.
// Every row: {B*S, W, 0}.  Class-token tail (rvlm_vit::cls_tail, last block of a pooled bf16 pass): {B, S*W, B} - the B class rows,
// read and written in place in the [B*S, W] residual stream; row b of the B-row intermediates is image b.  a_rows is what the dgrad
// GEMMs that read the stream are told about the readable rows of their A operand (0: the default, M rounded up).
struct Rows { int M; long ld; int a_rows; };

// What a backward reads of a SAVED FORWARD, as opposed to what it reads of the handle it runs on (weights, scratch, the bf16
// qkv / attention output / act'(fc1), and - parameter pass - the kept linear inputs).  A handle's own backward views itself; the
// handoff (vit_backward_from) views the fp32-storage handle's forward from the bf16 handle's kernels.
struct SavedView {
    float* const* xs;                     // 2L+1 residual-stream slots
    const float *st_mean, *st_rstd;       // LayerNorm statistics, slot i at i * Mp
    long Mp;
    const float *patch_out, *emb_raw, *inv_norm;
    float* const* lse;                    // per block: log-sum-exp rows (bf16 kernels) / probabilities (fp32 batched path)
    float* const* lse2;                   // per block: the fp32 flash kernels' log-sum-exp rows, or null
    bool norm;                            // the forward's output was l2-normalised
    bool tail;                            // its last block ran as the class-token tail
    const float* mean_at(int i) const { return st_mean + (size_t)i * Mp; }
    const float* rstd_at(int i) const { return st_rstd + (size_t)i * Mp; }
};

// Where a backward that also produces the parameter gradients puts them, and which of its stages this call runs.  Stages in
// execution order: 0 = head (proj, ln_post), 1 + j = transformer block L-1-j, L + 1 = embeddings (ln_pre, positional / class
// embedding, conv1).  [stage_begin, stage_end) lets the host cut the pass into gradient buckets whose all-reduce overlaps the
// remaining stages (robustvlm_amd/trainer.py); the stages hand the residual gradient to each other through the handle.
struct ParamSink { const rvlm_vit_weights* gw; int accumulate, stage_begin, stage_end; };

// Which backward may read which saved forward.  A pooled forward the handle kept for itself (Input, or Params: a superset) is read by
// the input-gradient backward; only Params by the parameter pass; only a token pass (Tokens, or TokensParams: a superset) by the token
// backward; only TokensParams by the token parameter pass; the handoff takes any pooled pass of the fp32-storage handle (its own, or
// one run for the peer).
// (Input is checked by vit_backward for every caller; only rvlm_vit_backward_input can arrive there without a forward of its own.)
enum class Reader { Input, Params, Tokens, TokensParams, Handoff };
int saved_check(const rvlm_vit* h, Reader r, int B, const char* who = "");

static inline bool same_input_size(const rvlm_vit* a, const rvlm_vit* b) { return a->in_h == b->in_h && a->in_w == b->in_w; }
#define RVLM_REQUIRE_SAME_INPUT(a, b, who)                                                                                   \
    do {                                                                                                                      \
        if (!same_input_size(a, b)) return fail(RVLM_ERR_STATE, who ": the two handles are set to different input sizes");   \
    } while (0)

// ---- what crosses a file ------------------------------------------------------------------------------
// engine_create.hip  (alloc: false refreshes the weights of a created handle in place)
int load_weights(rvlm_vit* h, const rvlm_vit_weights* w, hipStream_t s, bool alloc);
// engine_forward.hip  (for_peer: the bf16 handle whose backward will read this saving forward - the handoff - or null)
int vit_forward(rvlm_vit* h, const float* x, const float* delta, int B, int normalize, int save, float* out_emb, hipStream_t s,
                rvlm_vit* for_peer = nullptr);
int vit_forward_tokens(rvlm_vit* h, const float* x, const float* delta, int B, const TokPass& tp, int save, float* out_emb, hipStream_t s);
int tok_ensure(rvlm_vit* h, bool want_buf);
int tokens_check(const rvlm_vit* h, int B, int depth, int save, const char* who);
// engine_backward.hip
int vit_backward(rvlm_vit* h, const float* d_emb, int B, float* grad_x, hipStream_t s);
int vit_backward_tokens(rvlm_vit* h, const TokSeed& ts, const float* d_emb, int B, float* grad_x, hipStream_t s);
int vit_backward_params(rvlm_vit* h, const float* d_emb, int B, const ParamSink& sink, hipStream_t s);
int vit_backward_params_tokens(rvlm_vit* h, const TokSeed& ts, const float* d_emb, int B, const ParamSink& sink, hipStream_t s);
int vit_backward_from(rvlm_vit* hb, rvlm_vit* hx, const float* d_emb, int B, float* grad_x, hipStream_t s);
// vlm_attack_kernels.hip: rvlm_apgd_linf_step (norm_kind 0) / rvlm_apgd_l2_step (2) with a flag word (RVLM_FLAG_NAN_GRAD) or null
int apgd_step_pooled(int norm_kind, const float* x, float* x_adv, float* x_adv_old, const float* grad, const float* step, float a,
                     float eps, size_t n_per_sample, int B, int32_t* flags, hipStream_t stream);
// grid of the element-wise kernels (grid-stride loops of 256 threads)
static inline int ew_blocks(size_t n) { size_t b = (n + 1023) / 1024; if (b > 2048) b = 2048; if (b < 1) b = 1; return (int)b; }

}  // namespace rvlm
