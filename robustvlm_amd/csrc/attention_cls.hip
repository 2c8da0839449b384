// Class-token attention of the LAST transformer block, bf16 (shares no helper with the flash kernels of attention_bf16*.hip).
// The encoder's output is ln_post(x[:, 0]) @ proj (open_clip VisionTransformer.forward with pool_type 'tok'), so in the last
// block only the class-token query contributes: every other query row of that block (and everything downstream of it) is
// dead.  One wave per (image, head): q is the class token's query, the keys / values are all S tokens.  fp32 softmax,
// natural-log lse.
//   fwd: o[b, h*64 + d] = sum_j softmax_j(scale * q.k_j) v_j[d]
//   bwd: dV_j = p_j dO, dK_j = dS_j q, dQ_0 = sum_j dS_j k_j with dS_j = scale * p_j (dO.v_j - dO.o); dQ_j = 0 (j > 0)
// HBM-bound: K and V of the block are read once (fwd) / K twice, V once (bwd); dqkv is written in full.
#include "kernels.h"

namespace rvlm {
__device__ __forceinline__ void unpack8(const uint4& v, float (&f)[8]) {
    f[0] = __uint_as_float(v.x << 16); f[1] = __uint_as_float(v.x & 0xffff0000u);
    f[2] = __uint_as_float(v.y << 16); f[3] = __uint_as_float(v.y & 0xffff0000u);
    f[4] = __uint_as_float(v.z << 16); f[5] = __uint_as_float(v.z & 0xffff0000u);
    f[6] = __uint_as_float(v.w << 16); f[7] = __uint_as_float(v.w & 0xffff0000u);
}
__device__ __forceinline__ unsigned pack2(float a, float b) {
    const bf16_t x = (bf16_t)a, y = (bf16_t)b;
    return (unsigned)*(const unsigned short*)&x | ((unsigned)*(const unsigned short*)&y << 16);
}
__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
    float acc = a[0] * b[0];
#pragma unroll
    for (int e = 1; e < 8; ++e) acc = fmaf(a[e], b[e], acc);
    return acc;
}
// sum over the 8 lanes that share lane >> 3 (the 8 sixteen-byte chunks of one 64-wide head row)
__device__ __forceinline__ float chunk_sum(float v) {
    v += __shfl_xor(v, 1);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 4);
    return v;
}
// Lane (g, c) = (lane >> 3, lane & 7): key j = g + 8 i, 16-byte chunk c of its 128-byte head row, so that one wave load
// covers 8 whole rows.  Dot products are reduced over c, the per-group running results over g at the end.

__global__ void __launch_bounds__(256)
attn_cls_fwd_kernel(const bf16_t* __restrict__ qkv, long ld, bf16_t* __restrict__ o, long ldo, float* __restrict__ lse,
                    int H, int S, int W, int total, float scale) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bh = blockIdx.x * 4 + wave;
    if (bh >= total) return;
    const int b = bh / H, hd = bh - b * H, g = lane >> 3, c = lane & 7;
    const bf16_t* base = qkv + (long)b * S * ld + hd * 64 + c * 8;
    float qc[8];
    unpack8(*(const uint4*)base, qc);
#pragma unroll
    for (int e = 0; e < 8; ++e) qc[e] *= scale;
    float m = -INFINITY, l = 0.0f, acc[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] = 0.0f;
    const int iters = (S + 7) >> 3;
    for (int i = 0; i < iters; ++i) {
        const int j = g + 8 * i;
        const bool valid = j < S;
        const bf16_t* row = base + (long)(valid ? j : S - 1) * ld;
        float kf[8], vf[8];
        unpack8(*(const uint4*)(row + W), kf);
        unpack8(*(const uint4*)(row + 2 * W), vf);
        const float sc = chunk_sum(dot8(kf, qc));
        if (valid) {
            const float mn = fmaxf(m, sc);
            const float corr = __expf(m - mn), pj = __expf(sc - mn);
            l = fmaf(l, corr, pj);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[e] = fmaf(acc[e], corr, pj * vf[e]);
            m = mn;
        }
    }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1) {
        const float m2 = __shfl_xor(m, off), l2 = __shfl_xor(l, off);
        const float mn = fmaxf(m, m2);
        const float ca = (m == -INFINITY) ? 0.0f : __expf(m - mn), cb = (m2 == -INFINITY) ? 0.0f : __expf(m2 - mn);
        l = l * ca + l2 * cb;
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[e] = acc[e] * ca + __shfl_xor(acc[e], off) * cb;
        m = mn;
    }
    if (g == 0) {
        const float inv = 1.0f / l;
        uint4 ov;
        ov.x = pack2(acc[0] * inv, acc[1] * inv); ov.y = pack2(acc[2] * inv, acc[3] * inv);
        ov.z = pack2(acc[4] * inv, acc[5] * inv); ov.w = pack2(acc[6] * inv, acc[7] * inv);
        *(uint4*)(o + (long)b * ldo + hd * 64 + c * 8) = ov;
        if (c == 0) lse[bh] = m + __logf(l);
    }
}

__global__ void __launch_bounds__(256)
attn_cls_bwd_kernel(const bf16_t* __restrict__ qkv, long ld, const bf16_t* __restrict__ o, long ldo,
                    const bf16_t* __restrict__ d_o, long lddo, const float* __restrict__ lse,
                    bf16_t* __restrict__ dqkv, long lddq, int H, int S, int W, int total, float scale) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int bh = blockIdx.x * 4 + wave;
    if (bh >= total) return;
    const int b = bh / H, hd = bh - b * H, g = lane >> 3, c = lane & 7;
    const bf16_t* base = qkv + (long)b * S * ld + hd * 64 + c * 8;
    bf16_t* dbase = dqkv + (long)b * S * lddq + hd * 64 + c * 8;
    float qc[8], doc[8], oc[8];
    unpack8(*(const uint4*)base, qc);
    unpack8(*(const uint4*)(d_o + (long)b * lddo + hd * 64 + c * 8), doc);
    unpack8(*(const uint4*)(o + (long)b * ldo + hd * 64 + c * 8), oc);
    const float Dsum = chunk_sum(dot8(doc, oc));
    const float Lse = lse[bh];
    float accq[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) accq[e] = 0.0f;
    const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
    const int iters = (S + 7) >> 3;
    for (int i = 0; i < iters; ++i) {
        const int j = g + 8 * i;
        const bool valid = j < S;
        const long rj = valid ? j : S - 1;
        float kf[8], vf[8];
        unpack8(*(const uint4*)(base + rj * ld + W), kf);
        unpack8(*(const uint4*)(base + rj * ld + 2 * W), vf);
        const float sc = chunk_sum(dot8(kf, qc));
        const float dp = chunk_sum(dot8(vf, doc));
        const float pj = valid ? __expf(scale * sc - Lse) : 0.0f;
        const float dsj = pj * (dp - Dsum) * scale;
#pragma unroll
        for (int e = 0; e < 8; ++e) accq[e] = fmaf(dsj, kf[e], accq[e]);
        if (valid) {
            uint4 kk, vv;
            kk.x = pack2(dsj * qc[0], dsj * qc[1]); kk.y = pack2(dsj * qc[2], dsj * qc[3]);
            kk.z = pack2(dsj * qc[4], dsj * qc[5]); kk.w = pack2(dsj * qc[6], dsj * qc[7]);
            vv.x = pack2(pj * doc[0], pj * doc[1]); vv.y = pack2(pj * doc[2], pj * doc[3]);
            vv.z = pack2(pj * doc[4], pj * doc[5]); vv.w = pack2(pj * doc[6], pj * doc[7]);
            bf16_t* drow = dbase + rj * lddq;
            *(uint4*)(drow + W) = kk;
            *(uint4*)(drow + 2 * W) = vv;
            if (j > 0) *(uint4*)drow = zero;
        }
    }
#pragma unroll
    for (int off = 8; off < 64; off <<= 1)
#pragma unroll
        for (int e = 0; e < 8; ++e) accq[e] += __shfl_xor(accq[e], off);
    if (g == 0) {
        uint4 qq;
        qq.x = pack2(accq[0], accq[1]); qq.y = pack2(accq[2], accq[3]);
        qq.z = pack2(accq[4], accq[5]); qq.w = pack2(accq[6], accq[7]);
        *(uint4*)dbase = qq;
    }
}

int attn_cls_fwd_bf16(const bf16_t* qkv, long ldqkv, bf16_t* o, long ldo, float* lse, int B, int H, int S,
                      hipStream_t s) {
    if (!qkv || !o || !lse || B <= 0 || H <= 0 || S <= 0 || ldqkv % 8 != 0 || ldo % 8 != 0)
        return fail(RVLM_ERR_ARG, "attn_cls_fwd_bf16: bad arguments");
    const int total = B * H;
    hipLaunchKernelGGL(attn_cls_fwd_kernel, dim3(cdiv(total, 4)), dim3(256), 0, s, qkv, ldqkv, o, ldo, lse, H, S, H * 64,
                       total, 0.125f);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
int attn_cls_bwd_bf16(const bf16_t* qkv, long ldqkv, const bf16_t* o, long ldo, const bf16_t* d_o, long lddo,
                      const float* lse, bf16_t* dqkv, long lddqkv, int B, int H, int S, hipStream_t s) {
    if (!qkv || !o || !d_o || !lse || !dqkv || B <= 0 || H <= 0 || S <= 0 || ldqkv % 8 != 0 || lddqkv % 8 != 0 ||
        ldo % 8 != 0 || lddo % 8 != 0)
        return fail(RVLM_ERR_ARG, "attn_cls_bwd_bf16: bad arguments");
    const int total = B * H;
    hipLaunchKernelGGL(attn_cls_bwd_kernel, dim3(cdiv(total, 4)), dim3(256), 0, s, qkv, ldqkv, o, ldo, d_o, lddo, lse, dqkv,
                       lddqkv, H, S, H * 64, total, 0.125f);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

}  // namespace rvlm
