/* rvlm_kernels.h - kernel-level entry points of librvlm.so (unit-test / benchmarking surface).
 *
 * Not part of the drop-in boundary (that is rvlm.h); these expose the individual HIP kernels the
 * encoder is built from so tests/ can check each one against the oracle in isolation.
 * bf16 buffers are passed as uint16_t* (raw bfloat16 bits).  All pointers are device pointers.
 */
#ifndef RVLM_KERNELS_H
#define RVLM_KERNELS_H
#include "rvlm.h"
#ifdef __cplusplus
extern "C" {
#endif

/* C[M,N] = epi(A[M,K] @ Bw[N,K]^T): epi 0 bf16 out(+bias); 1 f32 out(+bias)(+residual f32);
 * 2 h=acc+bias: out=bf16 act(h), out_pre=bf16 act'(h); 3 out=bf16 acc*h_pre (h_pre = a stored act'(h));
 * 4 f32 out(+bias).
 * A must be readable for round_up(M,128) rows. */
int rvlm_k_gemm_bf16_nt(const uint16_t* A, long lda, const uint16_t* Bw, long ldb, int M, int N, int K,
                        int a_rows, int epi, const float* bias, void* out, long ldo, uint16_t* out_pre,
                        const uint16_t* h_pre, const float* residual, int act, rvlm_stream_t stream);
/* generic strided batched fp32 GEMM (see robustvlm_amd/csrc/kernels.h: GemmF32) */
int rvlm_k_gemm_f32(const float* A, long sam, long sak, const float* B, long sbn, long sbk, float* C,
                    long scm, long scn, int M, int N, int K, float alpha, const float* bias,
                    rvlm_stream_t stream);
/* the same with one batch dimension (element strides sab / sbb / scb) and the whole epilogue: act >= 0 applies RVLM_ACT_*
 * (C_pre, if given, receives the pre-activation), dact_h multiplies by act'(dact_h[m, n]) (QuickGELU), residual adds */
int rvlm_k_gemm_f32_ex(const float* A, long sam, long sak, long sab, const float* B, long sbn, long sbk, long sbb,
                       float* C, long scm, long scn, long scb, int M, int N, int K, int nb, float alpha,
                       const float* bias, int act, float* C_pre, const float* dact_h, const float* residual,
                       rvlm_stream_t stream);
/* 1: the VALU fmaf-chain tiles for every later fp32 GEMM instead of the v_mfma_f32_32x32x2_f32 tiles (the two are
 * bit-identical: both evaluate every output element as the k-ordered fp32 fma chain); 0: default */
int rvlm_k_gemm_f32_set_valu(int on);
/* fp32 attention path: in-place row softmax of s (backward = 0), or ds = p * (ds - sum(p * ds)) * scale in place (backward = 1);
 * rows of `cols` values, `ld` floats apart */
int rvlm_k_softmax_rows(const float* p, float* s, long rows, int cols, int ld, float scale, int backward, rvlm_stream_t stream);
/* bf16 flash attention on packed qkv [B*S, 3W] (head_dim 64); lse2 [B*H*round_up(S,32)] */
/* fp32 flash forward (csrc/attention_f32.hip): qkv fp32 [B*S, 3*64*H], o fp32 [B*S, 64*H]; optional lse2 [B*H, round_up(S, 32)] (log2
 * domain of 0.125 log2(e) q.k) and bf16 copies qkv_bf / o_bf in the same layouts; S <= 288 */
int rvlm_k_attn_fwd_f32_flash(const float* qkv, float* o, float* lse2, uint16_t* qkv_bf, uint16_t* o_bf, int B, int H, int S,
                              rvlm_stream_t stream);
/* fp32 flash backward: dqkv fp32 [B*S, 3*64*H] from qkv, o, d_o (fp32) and the forward's lse2 rows; dsum [B*H, round_up(S, 32)] scratch;
 * S = 32 NK + 1..4, NK <= 8 */
int rvlm_k_attn_bwd_f32_flash(const float* qkv, const float* o, const float* d_o, const float* lse2, float* dsum, float* dqkv,
                              int B, int H, int S, rvlm_stream_t stream);
int rvlm_k_attn_fwd_bf16(const uint16_t* qkv, uint16_t* o, float* lse2, int B, int H, int S,
                         rvlm_stream_t stream);
int rvlm_k_attn_bwd_bf16(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse2,
                         float* dsum_scratch, uint16_t* dqkv, int B, int H, int S, rvlm_stream_t stream);
/* 1: ds_read_b64_tr_b16 transposed fragments (default); 0: scalar-LDS-read validation variant */
int rvlm_k_attn_set_use_tr(int on);
/* 0: 128x128 GEMM kernel only; 1 / 2: the production dispatch (persistent 256x256 kernel unless the fill rule or the
 * few-row rule sends the shape to the 128x128 kernel); 3: persistent kernel for every shape it can take (M >= 256,
 * N % 256 == 0, K % 128 == 0) regardless of those rules; -1: env RVLM_GEMM_VARIANT (default 2) */
int rvlm_k_gemm_set_variant(int v);
/* Bit mask of the kernel families the last rvlm_k_gemm_bf16_nt call (or the engine's last GEMM) launched (bits 2, 8 and 64
 * named kernels that left the tree and stay unused) */
#define RVLM_GEMM_K_128 1         /* gemm_bf16_nt_kernel, 128x128 tiles */
#define RVLM_GEMM_K_PERSISTENT 4  /* gemm_bf16_nt_256p_kernel, the persistent 256x256 kernel */
#define RVLM_GEMM_K_SPLITK 16     /* split-K slabs on the 128x128 kernel + splitk_reduce_kernel */
#define RVLM_GEMM_K_STRIP 32      /* remainder rows computed by the persistent kernel's strip phase (same launch) */
int rvlm_k_gemm_last_kernels(void);
/* persistent 256x256 kernel: device buffer of 256*8*4 uint64 receiving per-tile s_memtime stamps (tile start, first
 * K-step done, mainloop done, epilogue issued); NULL switches tracing off */
int rvlm_k_gemm_set_trace(void* ptr);
/* measurement only: the persistent GEMM's operand request stream (same tile order, 8 waves x (4 + 4) pieces of 8 rows x
 * 128 B per K-step) with no MFMA and no LDS, `depth` K-steps (depth x 64 KiB per CU) in flight in registers.
 * mode bit 0: one s_barrier per K-step (a wave waits for the slowest wave's pieces, like a GEMM K-step); bit 1: pieces by
 * LDS-DMA into LDS instead of into registers (depth <= 2).  A [M, K], Bw [N, K] bf16 row-major; M, N % 256 == 0,
 * K % 64 == 0; `out` >= 512 words (never written in practice). */
int rvlm_k_probe_operand_stream(const uint16_t* A, const uint16_t* Bw, int M, int N, int K, int depth, int mode,
                                uint32_t* out, rvlm_stream_t stream);
/* workgroups per CU reported by the runtime for attn fwd (96-VGPR build), attn fwd (default), attn dq */
int rvlm_k_attn_occupancy(int S, int* out3);
int rvlm_k_layernorm_fwd_f32(const float* x, const float* gamma, const float* beta, float* y,
                             float* mean, float* rstd, int M, int W, rvlm_stream_t stream);
/* bf16 dy and bf16 copy of the residual gradient; dres == NULL: the copy is the stream itself (accumulate reads it); accumulate < 0:
 * only rows that are multiples of -accumulate accumulate, the others are overwritten */
int rvlm_k_layernorm_bwd_bf16(const uint16_t* dy, const float* x, const float* gamma, const float* mean, const float* rstd,
                              float* dres, uint16_t* dres_lp, int accumulate, int M, int W, rvlm_stream_t stream);
int rvlm_k_layernorm_bwd_f32(const float* dy, const float* x, const float* gamma, const float* mean,
                             const float* rstd, float* dres, int accumulate, int M, int W,
                             rvlm_stream_t stream);
/* micro-probe of ds_read_b64_tr_b16: out[lane*4+j] for a 64-lane wave reading the bf16 buffer `src`
 * (>= 2048 elements, copied to LDS) at per-lane byte offsets `offs[64]`. */
int rvlm_k_probe_tr16(const uint16_t* src, const int32_t* offs, uint16_t* out, rvlm_stream_t stream);

/* Weight gradient of one linear layer on the split-K path of the training step (train/adversarial_training_clip.py:
 * 356-364, loss.backward()): dW[N,K] (+)= dY[M,N]^T X[M,K] (bf16 operands, fp32 result), dbias[N] (+)= column sums of
 * dY (NULL: skipped).  N, K multiples of 256, M >= 256.  `work`: device scratch of rvlm_k_wgrad_work_bytes(M, N, K). */
size_t rvlm_k_wgrad_work_bytes(int M, int N, int K);
int rvlm_k_wgrad_bf16(const uint16_t* dY, long lddy, const uint16_t* X, long ldx, int M, int N, int K, float* dW,
                      long lddw, int accumulate, float* dbias, void* work, size_t work_bytes, rvlm_stream_t stream);
/* 1: rvlm_k_wgrad_bf16 runs the form the training step used until round 4 (token-chunk transposes + NT GEMM) instead of the
 * copy-free contraction-major GEMM - the A/B arm of tests and benches; 0 (default): the training step's path. */
void rvlm_k_wgrad_set_transposed(int v);

/* Text tower (csrc/attention_causal.hip, csrc/text_kernels.hip).  Causal flash attention forward on packed qkv [B*S, 3*64*H]
 * (row i of a prompt attends to keys j <= i, scale 1/8), o [B*S, 64*H], S <= 96; only rows < active_len of every prompt are read and
 * written (0 = S).  bf16 buffers as raw bits. */
int rvlm_k_attn_causal_fwd_bf16(const uint16_t* qkv, uint16_t* o, int B, int H, int S, int active_len, rvlm_stream_t stream);
int rvlm_k_attn_causal_fwd_f32(const float* qkv, float* o, int B, int H, int S, int active_len, rvlm_stream_t stream);
/* x[n*active_len + t, :] = token_embedding[tokens[n, t], :] + positional_embedding[t, :] (tokens [N, context] int32), eot[n] = first
 * position of prompt n's largest id; flags (optional) |= RVLM_FLAG_TOKEN_RANGE / RVLM_FLAG_EOT_ACTIVE.  active_len 0 = context. */
int rvlm_k_text_embed(const int32_t* tokens, const float* token_embedding, const float* positional_embedding, float* x, int32_t* eot,
                      uint32_t* flags, int N, int context, int active_len, int vocab, int W, rvlm_stream_t stream);

/* The encoder's non-GEMM kernels, one entry per host launcher (tests/test_gpu_kernel_rows.py).  Row-major, contiguous rows
 * (leading dimension = the row width) unless a leading dimension is passed. */
/* LayerNorm kernels of the bf16 engine come in two forms: the row-register kernels (8 columns per lane and 512-column slab,
 * W = 512 / 1024 / 1536 / 2048) and the generic one.  rvlm_k_layernorm_form: the form rvlm_k_layernorm_fwd_bf16 and
 * rvlm_k_layernorm_bwd_bf16 run at width W (the dispatchers' own rule). */
#define RVLM_LN_FORM_GENERIC 0
#define RVLM_LN_FORM_ROW8 1
int rvlm_k_layernorm_form(int W);
int rvlm_k_layernorm_fwd_bf16(const float* x, const float* gamma, const float* beta, uint16_t* y, float* mean, float* rstd,
                              int M, int W, rvlm_stream_t stream);
/* split-bf16 ("x3") operand passes (csrc/x3_kernels.hip).  A3 [rows_out, 3K] = [hi | hi | lo] of A [M, K], rows M .. rows_out - 1
 * zero; K % 8 == 0 */
int rvlm_k_x3_split_rows(const float* A, long lda, uint16_t* A3, int M, int rows_out, int K, rvlm_stream_t stream);
/* mode 0: act(h); mode 1: out * act'(h).  A3 == NULL: the fp32 result goes to out [M, N]; else to A3 [rows_out, 3N] = [hi | hi | lo]
 * (out is then only read, in mode 1).  dact_bf (mode 0 only, optional): bf16(act'(h)), row stride ld_dact */
int rvlm_k_x3_act(const float* h, long ldh, float* out, long ldo, uint16_t* A3, int M, int rows_out, int N, int act, int mode,
                  uint16_t* dact_bf, long ld_dact, rvlm_stream_t stream);
/* out = bf16(A) (dact 0) or bf16(act'(A)) (dact 1) */
int rvlm_k_x3_export_bf16(const float* A, long lda, uint16_t* out, long ldo, int M, int N, int act, int dact, rvlm_stream_t stream);
/* LayerNorm whose result is written as the split copy A3 [rows_out, 3W]; RVLM_ERR_UNSUPPORTED (nothing launched) unless
 * W = 512 / 1024 / 1536 / 2048 */
int rvlm_k_x3_layernorm_fwd(const float* x, const float* gamma, const float* beta, uint16_t* A3, float* mean, float* rstd, int M,
                            int rows_out, int W, rvlm_stream_t stream);
/* weight [rows, cols] -> nk3 [rows, 3 cols] = [hi | lo | hi], t3 [cols, 3 rows] = the same of the transpose */
int rvlm_k_x3_prepare_weight(const float* src, int rows, int cols, uint16_t* nk3, uint16_t* t3, rvlm_stream_t stream);
/* class-token attention of the last block on packed qkv [B*S, 3*64*H]: o [B, 64*H] (row b = image b's class token), lse [B*H]
 * (natural log); bwd writes dqkv [B*S, 3*64*H] in full (dQ rows of the other tokens are zero) */
int rvlm_k_attn_cls_fwd_bf16(const uint16_t* qkv, uint16_t* o, float* lse, int B, int H, int S, rvlm_stream_t stream);
int rvlm_k_attn_cls_bwd_bf16(const uint16_t* qkv, const uint16_t* o, const uint16_t* d_o, const float* lse, uint16_t* dqkv, int B,
                             int H, int S, rvlm_stream_t stream);
/* tokens = [cls ; patch_out [B*(S-1), W]] + pos [S, W]; x0 [B*S, W] = ln_pre(tokens), mean / rstd [B*S]; tokens_out optional.
 * bwd: d_patch [B*(S-1), W] (fp32, or bf16 with bf16_out) = the LayerNorm backward of the patch rows of dx0 */
int rvlm_k_embed_lnpre_fwd(const float* patch_out, const float* cls, const float* pos, const float* gamma, const float* beta,
                           float* x0, float* mean, float* rstd, float* tokens_out, int B, int S, int W, rvlm_stream_t stream);
int rvlm_k_embed_lnpre_bwd(const float* dx0, const float* patch_out, const float* pos, const float* gamma, const float* mean,
                           const float* rstd, void* d_patch, int bf16_out, int B, int S, int W, rvlm_stream_t stream);
/* A0 [B*(img/P)^2, lda] (fp32, or bf16 with bf16_out): columns c*P*P + i*P + j = ((x (+ delta)) - mean_c) / std_c, columns
 * 3*P*P .. Kpad-1 zero; mean3 / std3 are HOST arrays of 3.  col2im: grad_x [B, 3, img, img] = dA0[row, col] / std_c */
int rvlm_k_im2col_normalize(const float* x, const float* delta, int B, int img, int P, const float* mean3, const float* std3,
                            void* A0, long lda, int Kpad, int bf16_out, rvlm_stream_t stream);
int rvlm_k_col2im_grad(const void* dA0, long lda, int bf16_in, int B, int img, int P, const float* std3, float* grad_x,
                       rvlm_stream_t stream);
/* The same two with a bicubic resize (rvlm.h, RVLM_HAS_INPUT_RESIZE) between the image and the patches: x / delta / grad_x are
 * [B, 3, in_h, in_w], the patches those of the (img, img) image; delta is added before the resize; 1 / std is applied once per
 * low-resolution pixel. */
int rvlm_k_resize_im2col_normalize(const float* x, const float* delta, int B, int in_h, int in_w, int img, int P, const float* mean3,
                                   const float* std3, void* A0, long lda, int Kpad, int bf16_out, rvlm_stream_t stream);
int rvlm_k_col2im_resize_grad(const void* dA0, long lda, int bf16_in, int B, int in_h, int in_w, int img, int P, const float* std3,
                              float* grad_x, rvlm_stream_t stream);
/* backward of rvlm_l2_normalize_rows: d_raw = (d_out - ehat (ehat . d_out)) * inv_norm */
int rvlm_k_l2_normalize_bwd(const float* d_out, const float* e_raw, const float* inv_norm, float* d_raw, int B, int D,
                            rvlm_stream_t stream);

/* token_kernels.hip: the start of the residual-gradient stream from a token cotangent d_tok [M, W] fp32 - d32 (fp32) and / or
 * dlp (bf16) rows [0, M) = d_tok (+ cls_add[b, :] on row b S, cls_add [B, W] or NULL), rows [M, Mp) = 0.  W % 8 == 0. */
int rvlm_k_tokens_seed(const float* d_tok, const float* cls_add, float* d32, uint16_t* dlp, int M, int Mp, int S, int W,
                       rvlm_stream_t stream);

/* The training step's kernels, one entry per host launcher of csrc/train_kernels.hip (tests/test_gpu_train_kernels.py).  Leading
 * dimensions in elements.  The column reductions run in two passes - R rows in rvlm_k_reduce_chunks(R) row chunks, then the sum of the
 * chunks' partials - and take caller-owned scratch `red` of red_floats floats: rvlm_k_reduce_chunks(R) * C for rvlm_k_colsum, twice
 * that for rvlm_k_ln_param_grad; RVLM_ERR_STATE (nothing launched) when it is smaller.  rvlm_k_colsum_form: the form rvlm_k_colsum
 * runs for an operand of that element type, width, leading dimension and address (only the address's low four bits matter) - the
 * dispatchers' own rules, like rvlm_k_layernorm_form. */
#define RVLM_COLSUM_FORM_GENERIC 0   /* colsum_partial_kernel<T>: 64 columns x 4 row lanes per workgroup, one element per lane */
#define RVLM_COLSUM_FORM_16B 1       /* colsum8_partial_kernel: bf16, C % 256 == 0, every row 16-byte aligned; 16 B per lane */
int rvlm_k_reduce_chunks(int R);
int rvlm_k_colsum_form(int bf16_in, int C, long ld, size_t base_alignment);
/* out[c] (+)= sum_r in[r, c]; in [R, C] fp32, or bf16 with bf16_in (bias gradients) */
int rvlm_k_colsum(const void* in, int bf16_in, long ld, int R, int C, float* out, int accumulate, float* red, size_t red_floats,
                  rvlm_stream_t stream);
/* LayerNorm affine gradients: dgamma[c] (+)= sum_r dy[r, c] (x[r, c] - mean[r]) rstd[r], dbeta[c] (+)= sum_r dy[r, c]; dy fp32, or
 * bf16 with bf16_dy; x fp32; mean / rstd [R] */
int rvlm_k_ln_param_grad(const void* dy, int bf16_dy, long lddy, const float* x, long ldx, const float* mean, const float* rstd,
                         int R, int C, float* dgamma, float* dbeta, int accumulate, float* red, size_t red_floats,
                         rvlm_stream_t stream);
/* dpos[s, c] (+)= sum_b dtok[b S + s, c] (dpos [S, W] contiguous), dcls[c] (+)= the same for s = 0 */
int rvlm_k_pos_cls_grad(const float* dtok, long ld, int B, int S, int W, float* dpos, float* dcls, int accumulate,
                        rvlm_stream_t stream);
/* d_patch[b (S - 1) + s - 1, :] = dtok[b S + s, :] for s >= 1 (the class rows are not read); d_patch fp32, or bf16 (round to nearest
 * even) with bf16_out */
int rvlm_k_gather_patch_rows(const float* dtok, long ld, int B, int S, int W, void* d_patch, long ldp, int bf16_out,
                             rvlm_stream_t stream);
/* bf16: out[c, r] = in[r, c] for r < R, 0 for R <= r < Rp (the K padding of the weight-gradient GEMM); out [C, Rp], rows ldo apart */
int rvlm_k_transpose_pad(const uint16_t* in, long ldi, int R, int C, uint16_t* out, long ldo, int Rp, rvlm_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
