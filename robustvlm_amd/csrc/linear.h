// What the vision engine (engine_*.hip) and the text tower (text_engine.hip) share on the host side: a handle's device allocations,
// one transformer block's weights, and the linear layer with its dispatch on precision - bf16 MFMA GEMM, split-bf16 ("x3", three bf16
// products behind an fp32 interface, x3_kernels.hip) or the fp32 tiles.  Nothing here knows which tower it serves.
#pragma once
#include <array>
#include <vector>

#include "kernels.h"

namespace rvlm {

// ---- device memory of a handle ----------------------------------------------------------------
struct DeviceArena {
    std::vector<void*> allocs;       // freed by the handle's destroy
    size_t bytes = 0;                // what rvlm_*_workspace_bytes reports
};
// hipMalloc of `bytes` rounded up to 256 (at least 256), zero-filled unless told otherwise, owned by the arena
int dev_alloc(DeviceArena& a, void** p, size_t bytes, bool zero = true);
#define ALLOC(ptr, bytes)                                              \
    do { int _rc = dev_alloc(h->arena, (void**)&(ptr), (bytes)); if (_rc) return _rc; } while (0)
// device-to-device copy of n floats into *dst; alloc: *dst is allocated first (false: refreshed in place).  who: the handle type the
// error message names ("rvlm_vit", "rvlm_text")
int copy_f32(DeviceArena& a, float** dst, const float* src, size_t n, hipStream_t s, bool alloc, const char* who);

// ---- the weights of one transformer block -------------------------------------------------------
struct Layer {
    float *ln1_w, *ln1_b, *ln2_w, *ln2_b, *b_in, *b_out, *b_fc, *b_proj;
    float *w_in, *w_out, *w_fc, *w_proj;                          // fp32 mode (reference layout)
    bf16_t *w_in_nk, *w_in_t, *w_out_nk, *w_out_t, *w_fc_nk, *w_fc_t, *w_proj_nk, *w_proj_t;  // bf16; x3: [N, 3K] / [K, 3N]
                                                                  // (the forward-only text tower leaves the *_t forms null)
};
// The four weight matrices of a block, [rows, cols] in the reference layout, with the slots of their device forms - the order both
// towers' loaders walk them in (in-proj, out-proj, fc1, fc2).  Which forms a handle keeps, and their padding, is the loader's.
struct BlockWeight { float** f32; bf16_t **nk, **t; const float* src; int rows, cols; };
std::array<BlockWeight, 4> block_weights(Layer& y, const rvlm_vit_block_weights& b, int W);
// ... and its eight LayerNorm / bias vectors (copy_f32 of each)
int load_block_vectors(DeviceArena& a, Layer& y, const rvlm_vit_block_weights& b, int W, hipStream_t s, bool alloc, const char* who);

// ---- linear layers (dispatch on precision) ---------------------------------------------------
// What the dispatch reads of the handle that embeds it.  bf16 / x3 / act are written once, at the handle's creation, and are THE
// precision flags of the handle (the walkers read them here; the handles keep no copy).
struct LinearCtx {
    bool bf16 = false;
    bool x3 = false;     // fp32 storage, split-bf16 linears (RVLM_PREC_F32X3, csrc/x3_kernels.hip): w_*_nk / w_*_t hold [N, 3K] / [K, 3N]
    int act = 0;         // RVLM_ACT_* (= the handle's cfg.act)
    bf16_t* a3 = nullptr;        // x3: [Mp, 3 * 4W] bf16, the split copy [hi | hi | lo] of the linear in front of the GEMM
    const void* a3_of = nullptr; // x3: the fp32 buffer whose split a3 ALREADY holds (written by the fused activation + split pass)
    // fp32 slabs of the split-K few-row GEMMs (+ weight-gradient GEMMs when trainable).  The text tower leaves them null / 0 on
    // purpose: every output element is then one k-ordered accumulation whatever M is, so neither the chunking of a batch nor the
    // active length changes the bits of a prompt.
    float* splitk = nullptr;
    size_t splitk_bytes = 0;
};
// every GEMM descriptor carries its handle's split-K slab scratch (no process-wide state: handles coexist)
static inline void with_scratch(const LinearCtx& c, GemmBf16& g) { g.splitk = c.splitk; g.splitk_bytes = c.splitk_bytes; }
// x3 mode: the encoder linears whose shapes the persistent bf16 GEMM takes (everything else - the patch embedding with its
// K = 3 P^2, tiny test models - stays on the fp32 tiles)
static inline bool x3_takes(const LinearCtx& c, int M, int N, int K) {
    return c.x3 && c.a3 && M >= 256 && N % 256 == 0 && K % 128 == 0 && (long)round_up(M, 256) * 3 * K * 2 < (1L << 31);
}

// forward: out[M,N] = epi(A[M,K] @ Wt[N,K]^T + bias): epi EPI_BF16 (plain), EPI_BF16_ACT (activation; out_pre: the pre-activation
// too), EPI_F32 / EPI_F32_RESID (fp32 out, + residual)
// (dact_out, fp32 storage with EPI_BF16_ACT: act'(fc1) in bf16 for the bf16 handle this forward runs for, FwdPass::peer.  It is written
// whenever it is given - on the fp32 tiles from out_pre, which must then be given as well)
template <typename T>
int linear_fwd(LinearCtx& c, hipStream_t s, const void* A, long lda, int M, int N, int K,
               const float* w_f32, const bf16_t* w_nk, const float* bias, int epi, void* out, long ldo,
               void* out_pre, const float* residual, int a_rows = 0, bf16_t* dact_out = nullptr);
// dgrad: out[M,K] = epi(dY[M,N] @ W[N,K])   (w_t = W^T stored [K,N] for the bf16 path)
template <typename T>
int linear_dgrad(LinearCtx& c, hipStream_t s, const void* dY, long lddy, int M, int N, int K,
                 const float* w_f32, long ldw, const bf16_t* w_t, int epi, void* out, long ldo,
                 const void* h_pre, int a_rows = 0);
// (specialised in linear.hip)
template <> int linear_fwd<bf16_t>(LinearCtx&, hipStream_t, const void*, long, int, int, int, const float*, const bf16_t*, const float*, int,
                                   void*, long, void*, const float*, int, bf16_t*);
template <> int linear_fwd<float>(LinearCtx&, hipStream_t, const void*, long, int, int, int, const float*, const bf16_t*, const float*, int,
                                  void*, long, void*, const float*, int, bf16_t*);
template <> int linear_dgrad<bf16_t>(LinearCtx&, hipStream_t, const void*, long, int, int, int, const float*, long, const bf16_t*, int, void*,
                                     long, const void*, int);
template <> int linear_dgrad<float>(LinearCtx&, hipStream_t, const void*, long, int, int, int, const float*, long, const bf16_t*, int, void*,
                                    long, const void*, int);

// x3 mode: the LayerNorm (width W) in front of a linear of N_next outputs writes that linear's split operand itself (a3_of = the fp32
// buffer the linear will be handed, which is then never written: its only other reader is the weight gradient, which this precision
// does not have)
// (false: not taken, the caller runs the LayerNorm kernel; true: *rc = the launch status)
bool ln_into_split(LinearCtx& c, hipStream_t s, const float* x, const float* gamma, const float* beta, const void* ln_out,
                   float* mean, float* rstd, int M, int N_next, int W, int* rc);

}  // namespace rvlm
