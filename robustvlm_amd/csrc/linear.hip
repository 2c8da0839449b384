// Shared by both towers: a handle's device allocations, the block-weight table, and the linear layer's dispatch on precision (linear.h).
#include <algorithm>

#include "linear.h"

namespace rvlm {

int dev_alloc(DeviceArena& a, void** p, size_t bytes, bool zero) {
    bytes = std::max<size_t>((bytes + 255) & ~(size_t)255, 256);
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(RVLM_ERR_HIP, std::string("hipMalloc(") + std::to_string(bytes) + "): " + hipGetErrorString(e));
    if (zero) {
        e = hipMemset(*p, 0, bytes);
        if (e != hipSuccess) return fail(RVLM_ERR_HIP, std::string("hipMemset: ") + hipGetErrorString(e));
    }
    a.allocs.push_back(*p);
    a.bytes += bytes;
    return RVLM_OK;
}

// ---- weights --------------------------------------------------------------------------------
int copy_f32(DeviceArena& a, float** dst, const float* src, size_t n, hipStream_t s, bool alloc, const char* who) {
    if (!src) return fail(RVLM_ERR_ARG, std::string(who) + ": null weight pointer");
    if (alloc) { int rc = dev_alloc(a, (void**)dst, n * 4, false); if (rc) return rc; }
    RVLM_HIP(hipMemcpyAsync(*dst, src, n * 4, hipMemcpyDeviceToDevice, s));
    return RVLM_OK;
}
std::array<BlockWeight, 4> block_weights(Layer& y, const rvlm_vit_block_weights& b, int W) {
    return {{{&y.w_in, &y.w_in_nk, &y.w_in_t, b.attn_in_proj_weight, 3 * W, W}, {&y.w_out, &y.w_out_nk, &y.w_out_t, b.attn_out_proj_weight, W, W},
             {&y.w_fc, &y.w_fc_nk, &y.w_fc_t, b.mlp_c_fc_weight, 4 * W, W}, {&y.w_proj, &y.w_proj_nk, &y.w_proj_t, b.mlp_c_proj_weight, W, 4 * W}}};
}
int load_block_vectors(DeviceArena& a, Layer& y, const rvlm_vit_block_weights& b, int W, hipStream_t s, bool alloc, const char* who) {
    int rc;
#define CP(dst, src, n) if ((rc = copy_f32(a, &(dst), (src), (n), s, alloc, who))) return rc
    CP(y.ln1_w, b.ln_1_weight, W); CP(y.ln1_b, b.ln_1_bias, W);
    CP(y.ln2_w, b.ln_2_weight, W); CP(y.ln2_b, b.ln_2_bias, W);
    CP(y.b_in, b.attn_in_proj_bias, 3 * W); CP(y.b_out, b.attn_out_proj_bias, W);
    CP(y.b_fc, b.mlp_c_fc_bias, 4 * W); CP(y.b_proj, b.mlp_c_proj_bias, W);
#undef CP
    return RVLM_OK;
}

// ---- linear layers (dispatch on precision) ---------------------------------------------------
template <>
int linear_fwd<bf16_t>(LinearCtx& c, hipStream_t s, const void* A, long lda, int M, int N, int K,
                       const float*, const bf16_t* w_nk, const float* bias, int epi, void* out, long ldo,
                       void* out_pre, const float* residual, int a_rows, bf16_t*) {
    GemmBf16 g;
    g.A = (const bf16_t*)A; g.lda = lda; g.Bw = w_nk; g.ldb = K; g.M = M; g.N = N; g.K = K;
    g.a_rows = a_rows > 0 ? a_rows : (int)round_up(M, 128); g.epi = epi; g.bias = bias; g.out = out; g.ldo = ldo;
    g.out_pre = (bf16_t*)out_pre; g.residual = residual; g.act = c.act;
    with_scratch(c, g);
    return gemm_bf16_nt(g, s);
}
template <>
int linear_fwd<float>(LinearCtx& c, hipStream_t s, const void* A, long lda, int M, int N, int K,
                      const float* w_f32, const bf16_t* w_nk, const float* bias, int epi, void* out, long ldo,
                      void* out_pre, const float* residual, int, bf16_t* dact_out) {
    if (x3_takes(c, M, N, K) && w_nk) {
        // split-bf16: A3 = [A_hi | A_hi | A_lo] against W3 = [W_hi | W_lo | W_hi] - one bf16 GEMM of contraction length 3 K with an
        // fp32 epilogue; the activation (fc1) runs as its own pass over the fp32 pre-activation
        int rc = RVLM_OK;
        if (c.a3_of != A && (rc = x3_split_rows((const float*)A, lda, c.a3, M, (int)round_up(M, 256), K, s))) return rc;
        c.a3_of = nullptr;
        const bool act = epi == EPI_BF16_ACT;
        GemmBf16 g;
        g.A = c.a3; g.lda = 3L * K; g.Bw = w_nk; g.ldb = 3L * K; g.M = M; g.N = N; g.K = 3 * K;
        g.a_rows = (int)round_up(M, 256); g.bias = bias; g.residual = residual;
        g.epi = residual ? EPI_F32_RESID : EPI_F32;
        g.out = (act && out_pre) ? out_pre : out; g.ldo = ldo; g.act = c.act;
        with_scratch(c, g);
        if ((rc = gemm_bf16_nt(g, s))) return rc;
        if (act) {
            // act(h) goes straight into the split copy the next linear (fc2: A = `out`, K = N) reads; `out` itself is not written
            // (its only other reader is the weight gradient, which this precision does not have)
            const bool fuse = x3_takes(c, M, K, N);      // fc2's own rule: [M, N] x [K, N]^T
            if ((rc = x3_act((const float*)g.out, ldo, (float*)out, ldo, fuse ? c.a3 : nullptr, M, (int)round_up(M, 256), N, c.act, 0, s,
                             dact_out, ldo)))
                return rc;
            if (fuse) c.a3_of = out;
        }
        return RVLM_OK;
    }
    GemmF32 g;
    g.A = (const float*)A; g.sam = lda; g.sak = 1;
    g.B = w_f32; g.sbn = K; g.sbk = 1;
    g.C = (float*)out; g.scm = ldo; g.scn = 1;
    g.M = M; g.N = N; g.K = K; g.bias = bias; g.residual = residual;
    if (epi == EPI_BF16_ACT) { g.act = c.act; g.C_pre = (float*)out_pre; }
    int rc = gemm_f32(g, s);
    if (rc == RVLM_OK && epi == EPI_BF16_ACT && dact_out && out_pre)      // a forward for a peer on the fp32 tiles: act'(h) for it
        rc = x3_export_bf16((const float*)out_pre, ldo, dact_out, ldo, M, N, c.act, 1, s);
    return rc;
}
template <>
int linear_dgrad<bf16_t>(LinearCtx& c, hipStream_t s, const void* dY, long lddy, int M, int N, int K,
                         const float*, long, const bf16_t* w_t, int epi, void* out, long ldo,
                         const void* h_pre, int a_rows) {
    GemmBf16 g;
    g.A = (const bf16_t*)dY; g.lda = lddy; g.Bw = w_t; g.ldb = N; g.M = M; g.N = K; g.K = N;
    g.a_rows = a_rows > 0 ? a_rows : (int)round_up(M, 128); g.epi = epi; g.out = out; g.ldo = ldo;
    g.h_pre = (const bf16_t*)h_pre; g.act = c.act;
    with_scratch(c, g);
    return gemm_bf16_nt(g, s);
}
template <>
int linear_dgrad<float>(LinearCtx& c, hipStream_t s, const void* dY, long lddy, int M, int N, int K,
                        const float* w_f32, long ldw, const bf16_t* w_t, int epi, void* out, long ldo,
                        const void* h_pre, int) {
    if (x3_takes(c, M, K, N) && w_t) {      // out[M, K] = dY[M, N] W[N, K]: contraction over N, B operand = [W^T_hi | W^T_lo | W^T_hi]
        int rc = RVLM_OK;
        if (c.a3_of != dY && (rc = x3_split_rows((const float*)dY, lddy, c.a3, M, (int)round_up(M, 256), N, s))) return rc;
        c.a3_of = nullptr;
        GemmBf16 g;
        g.A = c.a3; g.lda = 3L * N; g.Bw = w_t; g.ldb = 3L * N; g.M = M; g.N = K; g.K = 3 * N;
        g.a_rows = (int)round_up(M, 256); g.epi = EPI_F32; g.out = out; g.ldo = ldo; g.act = c.act;
        with_scratch(c, g);
        if ((rc = gemm_bf16_nt(g, s))) return rc;
        if (epi == EPI_BF16_DACT) {      // out * act'(h): straight into the split copy the next dgrad (fc1: dY = `out`) reads
            const bool fuse = x3_takes(c, M, N, K);      // the rule of fc1's dgrad: [M, K] x [N, K]^T
            if ((rc = x3_act((const float*)h_pre, ldo, (float*)out, ldo, fuse ? c.a3 : nullptr, M, (int)round_up(M, 256), K, c.act, 1, s)))
                return rc;
            if (fuse) c.a3_of = out;
        }
        return RVLM_OK;
    }
    GemmF32 g;
    g.A = (const float*)dY; g.sam = lddy; g.sak = 1;
    g.B = w_f32; g.sbn = 1; g.sbk = ldw;          // (n = k_out, k = n_in) at n_in*ldw + k_out
    g.C = (float*)out; g.scm = ldo; g.scn = 1;
    g.M = M; g.N = K; g.K = N;
    if (epi == EPI_BF16_DACT) { g.dact_h = (const float*)h_pre; g.dact_kind = c.act; }
    return gemm_f32(g, s);
}

bool ln_into_split(LinearCtx& c, hipStream_t s, const float* x, const float* gamma, const float* beta, const void* ln_out,
                   float* mean, float* rstd, int M, int N_next, int W, int* rc) {
    if (!x3_takes(c, M, N_next, W)) return false;
    if (!x3_layernorm_fwd(x, W, gamma, beta, c.a3, mean, rstd, M, (int)round_up(M, 256), W, s, rc)) return false;
    if (*rc == RVLM_OK) c.a3_of = ln_out;
    return true;
}

}  // namespace rvlm
