// Launch API of the text tower's own kernels (host side): causal flash attention (attention_causal.hip) and the
// token-embedding front end / EOT gather (text_kernels.hip).  Each returns an rvlm_status.
#pragma once
#include "kernels.h"

namespace rvlm {

// Causal flash attention forward, head_dim 64, qkv packed [B * S, 3 * 64 * H] (q | k | v): prompt b at rows b * S .. b * S + S - 1,
// row i attends to keys j <= i (open_clip build_attention_mask), scale 1/8.  Only rows i < active of every prompt are read and
// written (1 <= active <= S <= 96); the rows behind them are left untouched.  No log-sum-exp output (forward only).
int attn_causal_fwd_bf16(const bf16_t* qkv, long ldqkv, bf16_t* o, long ldo, int B, int H, int S, int active, hipStream_t s);
int attn_causal_fwd_f32(const float* qkv, long ldqkv, float* o, long ldo, int B, int H, int S, int active, hipStream_t s);

// x[n * active + t, :] = token_embedding[tokens[n, t], :] + positional_embedding[t, :] for t < active (tokens [N, context] int32);
// eot[n] = first position of the largest id of prompt n (text.argmax(dim=-1)).  flags (optional device word) |=
// RVLM_FLAG_TOKEN_RANGE for an id outside [0, vocab) (the row is then built from id 0), RVLM_FLAG_EOT_ACTIVE for eot[n] >= active.
int text_embed_fwd(const int32_t* tokens, const float* token_embedding, const float* positional_embedding, float* x, int32_t* eot,
                   uint32_t* flags, int N, int context, int active, int vocab, int W, hipStream_t s);
// out[n, :] = x[n * active + min(eot[n], active - 1), :]
int text_gather_eot(const float* x, const int32_t* eot, float* out, int N, int active, int W, hipStream_t s);

}  // namespace rvlm
