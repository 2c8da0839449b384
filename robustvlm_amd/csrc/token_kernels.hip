// Token-level door of the encoder (RVLM_HAS_TOKENS): the kernels that turn a [B, S, W] cotangent - or FARE's embedding-L2 taken over
// the tokens a VLM reads (llava/model/multimodal_encoder/clip_encoder.py:55-65, open_flamingo/src/flamingo.py:217,242) - into the
// start of the residual-gradient stream in the form the handle's backward runs on (fp32, fp32 + bf16 copy, or bf16 only).
//
// rvlm_tokens_cosine (RVLM_HAS_TOKEN_TRAINING) is the logging metric of the token training step over the same rows.
//
// Rules all kernels keep: 16-byte global accesses (8 consecutive columns per thread and step; W is a multiple of 64), trip counts
// from the shape alone, fixed-order fp32 sums (per-thread partial over a shape-derived index sequence, xor-shuffle tree inside the
// wave, the four wave partials through LDS summed in wave order, the chunk partials of an image summed in chunk order by one thread):
// the same input gives the same bits on every run, no float atomics.  A non-finite per-image loss raises
// RVLM_FLAG_TOKENS_NONFINITE; nothing in any kernel branches or loops on a data value.
#include "kernels.h"

namespace rvlm {

constexpr int TOK_ROWS = 8;      // token rows of one workgroup

__device__ __forceinline__ void tok_load8(const float* p, float (&v)[8]) {
    const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
    v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
// 8 consecutive values of one row into whichever forms of the stream exist
__device__ __forceinline__ void tok_store8(float* d32, bf16_t* dlp, long off, const float (&v)[8]) {
    if (d32) {
        *(float4*)(d32 + off) = make_float4(v[0], v[1], v[2], v[3]);
        *(float4*)(d32 + off + 4) = make_float4(v[4], v[5], v[6], v[7]);
    }
    if (dlp) {
        bf16x8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] = (bf16_t)v[e];
        *(bf16x8*)(dlp + off) = o;
    }
}

// stream[m, :] = d_tok[m, :] (+ cls_add[b, :] on the class row m = b S) for m < M, 0 for M <= m < Mp.
// cls_add (ld_cls floats between images) may BE the class rows of d32: every element is read and then written by the same thread.
__global__ void __launch_bounds__(256)
tokens_seed_kernel(const float* __restrict__ d_tok, const float* cls_add, long ld_cls, float* d32, bf16_t* __restrict__ dlp,
                   int M, int Mp, int S, int W) {
    const int W8 = W >> 3, nvec = TOK_ROWS * W8;
    const int row0 = blockIdx.x * TOK_ROWS;
    for (int i = threadIdx.x; i < nvec; i += 256) {
        const int row = row0 + i / W8, c = (i % W8) << 3;
        if (row >= Mp) continue;
        float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (row < M) {
            tok_load8(d_tok + (long)row * W + c, v);
            if (cls_add && row % S == 0) {
                float a[8];
                tok_load8(cls_add + (long)(row / S) * ld_cls + c, a);
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] += a[e];
            }
        }
        tok_store8(d32, dlp, (long)row * W + c, v);
    }
}

// One workgroup per (image, chunk of TOK_ROWS token rows), then one per TOK_ROWS pad rows.  Rows s >= first are selected and meet
// row s - first of the reference [B, S - first, W]; d = 2 (t - ref) gscale goes out as the seed, unselected and pad rows as zeros.
// d32 may alias t (the ln_post form of the engine differentiates in place): same-thread read-then-write of each element.
__global__ void __launch_bounds__(256)
tokens_l2_loss_kernel(const float* t, const float* __restrict__ ref, int B, int S, int W, int first, float gscale, float* d32,
                      bf16_t* __restrict__ dlp, int Mp, float* __restrict__ partial) {
    __shared__ float wsum[4];
    const int W8 = W >> 3, nvec = TOK_ROWS * W8;
    const int nch = (S + TOK_ROWS - 1) / TOK_ROWS;
    const int M = B * S;
    if ((int)blockIdx.x >= B * nch) {      // pad rows M .. Mp - 1
        const int row0 = M + ((int)blockIdx.x - B * nch) * TOK_ROWS;
        const float z[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int i = threadIdx.x; i < nvec; i += 256) {
            const int row = row0 + i / W8;
            if (row < Mp) tok_store8(d32, dlp, (long)row * W + ((i % W8) << 3), z);
        }
        return;
    }
    const int b = blockIdx.x / nch, s0 = (blockIdx.x % nch) * TOK_ROWS;
    const int nsel = S - first;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < nvec; i += 256) {
        const int sr = s0 + i / W8, c = (i % W8) << 3;
        if (sr >= S) continue;
        const long off = ((long)b * S + sr) * W + c;
        float v[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (sr >= first) {
            float x[8], r[8];
            tok_load8(t + off, x);
            tok_load8(ref + ((long)b * nsel + (sr - first)) * W + c, r);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float d = x[e] - r[e];
                acc = fmaf(d, d, acc);
                v[e] = 2.0f * d * gscale;
            }
        }
        if (d32 || dlp) tok_store8(d32, dlp, off, v);
    }
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// second stage: per_sample[b] = the image's chunk partials in chunk order; scalar = their sum (/ B for the mean) in image order
__global__ void __launch_bounds__(256)
tokens_l2_finish_kernel(const float* __restrict__ partial, int B, int nch, int mean, float* __restrict__ per_sample,
                        float* __restrict__ scalar, int32_t* flags) {
    __shared__ int bad_any;
    if (threadIdx.x == 0) bad_any = 0;
    __syncthreads();
    for (int b = threadIdx.x; b < B; b += 256) {
        float a = 0.0f;
        for (int j = 0; j < nch; ++j) a += partial[(long)b * nch + j];
        per_sample[b] = a;
        if (!(fabsf(a) <= 3.402823466e38f)) bad_any = 1;      // NaN or Inf (benign race: every writer stores 1)
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (flags && bad_any) atomicOr(flags, RVLM_FLAG_TOKENS_NONFINITE);
        if (scalar) {
            float a = 0.0f;
            for (int b = 0; b < B; ++b) a += per_sample[b];
            *scalar = mean ? a / (float)B : a;
        }
    }
}

// Row cosine of the selected token rows (rows s >= first meet row s - first of ref [B, S - first, W]), F.cosine_similarity's epsilon
// rule as in cosine_rows_kernel (loss_kernels.hip): a.b / sqrt(max(|a|^2 |b|^2, 1e-16)).  One workgroup per (image, chunk of TOK_ROWS
// rows): wave w takes rows 2w and 2w + 1 of the chunk, lane i the 8-column groups i, i + 64, ...; partial[block] = the chunk's
// cosines summed wave by wave, row by row (unselected rows and rows past S add an exact 0).
__global__ void __launch_bounds__(256)
tokens_cosine_kernel(const float* __restrict__ t, const float* __restrict__ ref, int S, int W, int first,
                     float* __restrict__ partial) {
    __shared__ float wsum[4];
    const int W8 = W >> 3, nch = (S + TOK_ROWS - 1) / TOK_ROWS;
    const int b = blockIdx.x / nch, s0 = (blockIdx.x % nch) * TOK_ROWS;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nsel = S - first;
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < TOK_ROWS / 4; ++j) {
        const int sr = s0 + wave * (TOK_ROWS / 4) + j;
        const bool live = sr >= first && sr < S;      // (uniform over the wave)
        float ab = 0.0f, aa = 0.0f, bb = 0.0f;
        if (live) {
            const float* pa = t + ((long)b * S + sr) * W;
            const float* pb = ref + ((long)b * nsel + (sr - first)) * W;
            for (int g = lane; g < W8; g += 64) {
                float x[8], y[8];
                tok_load8(pa + (g << 3), x);
                tok_load8(pb + (g << 3), y);
#pragma unroll
                for (int e = 0; e < 8; ++e) { ab = fmaf(x[e], y[e], ab); aa = fmaf(x[e], x[e], aa); bb = fmaf(y[e], y[e], bb); }
            }
        }
        ab = wave_sum(ab); aa = wave_sum(aa); bb = wave_sum(bb);
        acc += live ? ab / sqrtf(fmaxf(aa * bb, 1e-16f)) : 0.0f;
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partial[blockIdx.x] = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}
// second stage: per_image[b] = (the image's chunk partials in chunk order) / rows; mean = (their sum in image order) / B.  The few
// terms of these two sums are added in double: a mean of O(1) cosines over hundreds of rows keeps its seventh digit.
__global__ void __launch_bounds__(256)
tokens_cosine_finish_kernel(const float* __restrict__ partial, int B, int nch, int rows, float* __restrict__ per_image,
                            float* __restrict__ mean) {
    for (int b = threadIdx.x; b < B; b += 256) {
        double a = 0.0;
        for (int j = 0; j < nch; ++j) a += (double)partial[(long)b * nch + j];
        per_image[b] = (float)(a / (double)rows);
    }
    __syncthreads();
    if (threadIdx.x == 0 && mean) {
        double a = 0.0;
        for (int b = 0; b < B; ++b) a += (double)per_image[b];
        *mean = (float)(a / (double)B);
    }
}

static inline bool aligned16(const void* p) { return ((size_t)p & 15) == 0; }

int tokens_seed(const float* d_tok, const float* cls_add, long ld_cls, float* d32, bf16_t* dlp, int M, int Mp, int S, int W,
                hipStream_t s) {
    RVLM_REQUIRE(d_tok && (d32 || dlp) && M > 0 && Mp >= M && S > 0 && W > 0 && W % 8 == 0, "tokens_seed: bad arguments");
    RVLM_REQUIRE(aligned16(d_tok) && aligned16(cls_add) && aligned16(d32) && aligned16(dlp) && ld_cls % 4 == 0,
                 "tokens_seed: pointers must be 16-byte aligned");
    hipLaunchKernelGGL(tokens_seed_kernel, dim3(cdiv(Mp, TOK_ROWS)), dim3(256), 0, s, d_tok, cls_add, ld_cls, d32, dlp, M, Mp, S, W);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

size_t tokens_l2_scratch_floats(int B, int S) { return (size_t)B * cdiv(S, TOK_ROWS); }

int tokens_l2_loss_grad(const float* t, const float* ref, int B, int S, int W, int select, int reduction, float* d32, bf16_t* dlp,
                        long seed_rows, float* per_sample, float* scalar, float* scratch, int32_t* flags, hipStream_t s) {
    RVLM_REQUIRE(t && ref && per_sample && scratch, "rvlm_tokens_l2_loss_grad: null argument");
    RVLM_REQUIRE(B > 0 && S > 1 && W > 0 && W % 8 == 0, "rvlm_tokens_l2_loss_grad: need B > 0, S > 1 and a width that is a multiple of 8");
    RVLM_REQUIRE(select == RVLM_TOKENS_ALL || select == RVLM_TOKENS_PATCH, "rvlm_tokens_l2_loss_grad: unknown select");
    RVLM_REQUIRE(reduction == RVLM_RED_MEAN || reduction == RVLM_RED_NONE, "rvlm_tokens_l2_loss_grad: unknown reduction");
    RVLM_REQUIRE((long)B * S < (1L << 31) / TOK_ROWS, "rvlm_tokens_l2_loss_grad: too many rows");
    const long M = (long)B * S;
    if (seed_rows == 0) seed_rows = M;
    RVLM_REQUIRE(seed_rows >= M && seed_rows < (1L << 31), "rvlm_tokens_l2_loss_grad: seed_rows must be 0 or >= B * S");
    RVLM_REQUIRE(aligned16(t) && aligned16(ref) && aligned16(d32) && aligned16(dlp),
                 "rvlm_tokens_l2_loss_grad: pointers must be 16-byte aligned");
    const int nch = cdiv(S, TOK_ROWS);
    const int pad_blocks = (d32 || dlp) ? cdiv(seed_rows - M, TOK_ROWS) : 0;
    const float gscale = reduction == RVLM_RED_MEAN ? 1.0f / (float)B : 1.0f;
    hipLaunchKernelGGL(tokens_l2_loss_kernel, dim3(B * nch + pad_blocks), dim3(256), 0, s, t, ref, B, S, W,
                       select == RVLM_TOKENS_PATCH ? 1 : 0, gscale, d32, dlp, (int)seed_rows, scratch);
    RVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(tokens_l2_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)scratch, B, nch,
                       reduction == RVLM_RED_MEAN ? 1 : 0, per_sample, scalar, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

}  // namespace rvlm

using namespace rvlm;

extern "C" int rvlm_tokens_l2_loss_grad(const float* tokens, const float* ref_tokens, int B, int S, int W, int select, int reduction,
                                        float* seed_f32, uint16_t* seed_bf16, long seed_rows, float* loss_per_sample,
                                        float* loss_scalar, float* scratch, int32_t* flags, rvlm_stream_t stream) {
    return tokens_l2_loss_grad(tokens, ref_tokens, B, S, W, select, reduction, seed_f32, (bf16_t*)seed_bf16, seed_rows, loss_per_sample,
                               loss_scalar, scratch, flags, (hipStream_t)stream);
}

extern "C" int rvlm_tokens_cosine(const float* tokens, const float* ref_tokens, int B, int S, int W, int select, float* out_per_image,
                                  float* out_mean, float* scratch, rvlm_stream_t stream) {
    RVLM_REQUIRE(tokens && ref_tokens && out_per_image && scratch, "rvlm_tokens_cosine: null argument");
    RVLM_REQUIRE(B > 0 && S > 1 && W > 0 && W % 8 == 0, "rvlm_tokens_cosine: need B > 0, S > 1 and a width that is a multiple of 8");
    RVLM_REQUIRE(select == RVLM_TOKENS_ALL || select == RVLM_TOKENS_PATCH, "rvlm_tokens_cosine: unknown select");
    RVLM_REQUIRE((long)B * S < (1L << 31) / TOK_ROWS, "rvlm_tokens_cosine: too many rows");
    RVLM_REQUIRE(aligned16(tokens) && aligned16(ref_tokens), "rvlm_tokens_cosine: pointers must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int nch = cdiv(S, TOK_ROWS), first = select == RVLM_TOKENS_PATCH ? 1 : 0;
    hipLaunchKernelGGL(tokens_cosine_kernel, dim3(B * nch), dim3(256), 0, s, tokens, ref_tokens, S, W, first, scratch);
    RVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL(tokens_cosine_finish_kernel, dim3(1), dim3(256), 0, s, (const float*)scratch, B, nch, S - first,
                       out_per_image, out_mean);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
