// Front and back end of the CLIP text tower (open_clip CLIP.encode_text, model.py): token embedding + positional embedding into the
// fp32 residual stream, the EOT position of every prompt (text.argmax(dim=-1)), and the gather of the EOT rows in front of ln_final.
// The residual stream holds the first `active` positions of every prompt only (row n * active + t): behind a causal mask nothing
// at a later position can reach the EOT row.
#include <algorithm>

#include "text_kernels.h"

namespace rvlm {

// one 16-byte chunk per thread and step: x[n * A + t, c .. c + 3] = E[id, c ..] + P[t, c ..]
__global__ void __launch_bounds__(256)
text_embed_kernel(const int32_t* __restrict__ tokens, const float* __restrict__ E, const float* __restrict__ P, float* __restrict__ x,
                  uint32_t* __restrict__ flags, int N, int context, int A, int vocab, int W) {
    const int chunks = W >> 2;
    const long total = (long)N * A * chunks;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % chunks);
        const long row = i / chunks;
        const int t = (int)(row % A), n = (int)(row / A);
        int id = tokens[(long)n * context + t];
        if (id < 0 || id >= vocab) {      // reported, never dereferenced
            if (flags && c == 0) atomicOr(flags, (uint32_t)RVLM_FLAG_TOKEN_RANGE);
            id = 0;
        }
        const float4 e = *(const float4*)(E + (long)id * W + 4 * c), p = *(const float4*)(P + (long)t * W + 4 * c);
        *(float4*)(x + row * W + 4 * c) = make_float4(e.x + p.x, e.y + p.y, e.z + p.z, e.w + p.w);
    }
}

// one wave per prompt: the FIRST position of the largest id over the whole context (torch argmax semantics on ties)
__global__ void __launch_bounds__(256)
text_eot_kernel(const int32_t* __restrict__ tokens, int32_t* __restrict__ eot, uint32_t* __restrict__ flags, int N, int context, int A) {
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (n >= N) return;
    int best = INT32_MIN, pos = INT32_MAX;
    for (int t = lane; t < context; t += 64) {      // ascending t per lane: strict > keeps the first occurrence
        const int v = tokens[(long)n * context + t];
        if (v > best) { best = v; pos = t; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int ob = __shfl_xor(best, o, 64), op = __shfl_xor(pos, o, 64);
        if (ob > best || (ob == best && op < pos)) { best = ob; pos = op; }
    }
    if (lane == 0) {
        eot[n] = pos;
        if (pos >= A && flags) atomicOr(flags, (uint32_t)RVLM_FLAG_EOT_ACTIVE);
    }
}

__global__ void __launch_bounds__(256)
text_gather_eot_kernel(const float* __restrict__ x, const int32_t* __restrict__ eot, float* __restrict__ out, int N, int A, int W) {
    const int chunks = W >> 2;
    const long total = (long)N * chunks;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int c = (int)(i % chunks), n = (int)(i / chunks);
        const int t = min(eot[n], A - 1);      // (eot >= A was flagged by text_eot_kernel: the call fails, the read stays in bounds)
        *(float4*)(out + (long)n * W + 4 * c) = *(const float4*)(x + ((long)n * A + t) * W + 4 * c);
    }
}

int text_embed_fwd(const int32_t* tokens, const float* token_embedding, const float* positional_embedding, float* x, int32_t* eot,
                   uint32_t* flags, int N, int context, int active, int vocab, int W, hipStream_t s) {
    if (!tokens || !token_embedding || !positional_embedding || !x || !eot || N <= 0 || vocab <= 0)
        return fail(RVLM_ERR_ARG, "text_embed_fwd: bad arguments");
    if (context < 1 || active < 1 || active > context || W % 4 != 0 ||
        (((size_t)token_embedding | (size_t)positional_embedding | (size_t)x) & 15))
        return fail(RVLM_ERR_ARG, "text_embed_fwd: need 1 <= active <= context, W % 4 == 0, 16-byte aligned buffers");
    const long total = (long)N * active * (W >> 2);
    const int grid = (int)std::min<long>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(text_embed_kernel, dim3(grid), dim3(256), 0, s, tokens, token_embedding, positional_embedding, x, flags, N, context,
                       active, vocab, W);
    RVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(text_eot_kernel, dim3(cdiv(N, 4)), dim3(256), 0, s, tokens, eot, flags, N, context, active);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

int text_gather_eot(const float* x, const int32_t* eot, float* out, int N, int active, int W, hipStream_t s) {
    if (!x || !eot || !out || N <= 0 || active < 1 || W % 4 != 0) return fail(RVLM_ERR_ARG, "text_gather_eot: bad arguments");
    const long total = (long)N * (W >> 2);
    const int grid = (int)std::min<long>((total + 255) / 256, 256 * 32);
    hipLaunchKernelGGL(text_gather_eot_kernel, dim3(grid), dim3(256), 0, s, x, eot, out, N, active, W);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

}  // namespace rvlm
