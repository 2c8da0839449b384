// Causal flash attention FORWARD for the CLIP text tower (open_clip TextTransformer: context 77, head_dim 64, additive mask with
// -inf strictly above the diagonal, model.py build_attention_mask), two storage forms:
//   bf16 : v_mfma_f32_32x32x16_bf16, K / V of a head in LDS as swizzled [rows][64] bf16 tiles (precision bf16)
//   fp32 : v_mfma_f32_32x32x2_f32, K rows padded to 68 floats (precisions fp32 and x3)
// One workgroup per (prompt, head), one wave per 32-row query tile (S <= 96: at most three waves; K and V of a head are 24 KiB in
// bf16 and 50 KiB in fp32, so several workgroups share a CU).  Both forms use the swapped orientation of the image tower's kernels
// (attention_bf16.hip, attention_f32.hip): S^T = K Q^T puts one query on a lane, so the running max / sum are per-lane scalars, P^T is
// already the B operand of O^T = V^T P^T, and the causal mask is one compare of a key index against the lane's own query index.
// Wave w walks key tiles 0 .. w only: the tiles above the diagonal are skipped, not masked (6 tile products of 9 at S = 77), the
// diagonal tile is masked by index.  Key 0 is visible to every query, so a row's running max is finite after its first tile.
// Online softmax in the log2 domain, scale 0.125 log2(e).
//
// Active length: only rows < `active` of every prompt are read, evaluated and written.  A causal row never sees a later one, so the
// rows in front of `active` come out bit for bit as they do at full length: a masked score is -inf whatever lies behind it
// (exp2 -> 0, and 0 times the finite value staged in its V row adds nothing).
//
// The bf16 fragment helpers restate the few of attention_bf16.hip this kernel needs (same tile layout and swizzle); that file and
// its instantiations are not touched.
#include "text_kernels.h"

namespace rvlm {
namespace {

typedef __attribute__((address_space(3))) char ca_lds_char;

// [rows][64] bf16 tile, 128-B rows, 16-B chunk index XOR ca_key(row): conflict-free for the row-major ds_read_b128 fragments and
// for the transposing ds_read_b64_tr_b16 reads (row bit 1 on chunk bit 2: rows r and r + 2 land in different 64-B halves)
__device__ __forceinline__ int ca_key(int row) { return (((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 1) | ((row >> 2) & 1); }
__device__ __forceinline__ int ca_off(int row, int chunk) { return row * 128 + ((chunk ^ ca_key(row)) << 4); }

// rows [0, Sp) x 64 bf16 by LDS-DMA (8 rows per wave instruction; the swizzle goes on the per-lane SOURCE address because the DMA
// writes LDS lane-linearly).  Rows >= rows_valid replicate the last valid row: finite data behind a masked score.
__device__ __forceinline__ void ca_stage(char* tile, const bf16_t* src, long ld, int rows_valid, int Sp, int w, int nw, int lane) {
    for (int blk = w; blk < (Sp >> 3); blk += nw) {
        const int row = blk * 8 + (lane >> 3);
        const int lc = (lane & 7) ^ ca_key(row);
        const int rs = min(row, rows_valid - 1);
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(src + (long)rs * ld + lc * 8),
                                         (__attribute__((address_space(3))) void*)(tile + blk * 1024), 16, 0, 0);
    }
}
// per-lane byte offsets inside a 32-row tile (tiles start at multiples of 16 rows, which leaves ca_key unchanged)
struct CaOffs { int rm[4]; int tr[2][2]; };
__device__ __forceinline__ CaOffs ca_offs(int lane) {
    CaOffs o;
    const int l31 = lane & 31, hi = lane >> 5, i = lane & 15, dblk = (lane >> 4) & 1;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) o.rm[kk] = ca_off(l31, kk * 2 + hi);
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 2; ++r) o.tr[dt][r] = ca_off(4 * hi + 8 * r + (i >> 2), dt * 4 + dblk * 2 + ((i & 3) >> 1)) + (i & 1) * 8;
    return o;
}
// V^T fragment: MFMA row = column 32 dt + (lane & 31) of the tile, k index t <-> tile row row0 + 4 hi + (t & 3) + 8 (t >> 2)
__device__ __forceinline__ bf16x8 ca_frag_tr(const char* tile, int row0, const CaOffs& o, int dt) {
    bf16x8 out;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
            (__attribute__((address_space(3))) bf16x4*)((ca_lds_char*)tile + row0 * 128 + o.tr[dt][r]));
        out[4 * r + 0] = v[0]; out[4 * r + 1] = v[1]; out[4 * r + 2] = v[2]; out[4 * r + 3] = v[3];
    }
    return out;
}
// accumulator (row = (reg & 3) + 8 (reg >> 2) + 4 hi) -> B operand of the 16-row k-slice ks
__device__ __forceinline__ bf16x8 ca_pack_b(const f32x16& p, int ks) {
    bf16x8 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) { o[t] = (bf16_t)p[(2 * ks) * 4 + t]; o[4 + t] = (bf16_t)p[(2 * ks + 1) * 4 + t]; }
    return o;
}
__device__ __forceinline__ f32x16 ca_zero16() {
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.0f;
    return z;
}

}  // namespace

// =============================================================================================
// bf16
// =============================================================================================
template <int NT>   // NT = ceil(active / 32) waves
__global__ void __launch_bounds__(NT * 64)
attn_causal_fwd_bf16_kernel(const bf16_t* __restrict__ qkv, long ld, bf16_t* __restrict__ o, long ldo, int H, int S, int A, int W,
                            float scale_log2) {
    constexpr int Sp = NT * 32;
    __shared__ __attribute__((aligned(16))) char smem[2 * Sp * 128];
    char* Kt = smem;
    char* Vt = smem + Sp * 128;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const bf16_t* base = qkv + (long)b * S * ld + h * 64;
    ca_stage(Kt, base + W, ld, A, Sp, w, NT, lane);
    ca_stage(Vt, base + 2 * W, ld, A, Sp, w, NT, lane);
    __syncthreads();

    const CaOffs fo = ca_offs(lane);
    const int q = w * 32 + l31;                 // this lane's query (both lane halves hold the same one)
    const int qc = min(q, A - 1);
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = *(const bf16x8*)(base + (long)qc * ld + (kk * 2 + hi) * 8);
    f32x16 oacc[2] = {ca_zero16(), ca_zero16()};
    float m = -INFINITY, l = 0.0f;
    for (int kt = 0; kt <= w; ++kt) {
        f32x16 st = ca_zero16();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            st = __builtin_amdgcn_mfma_f32_32x32x16_bf16(*(const bf16x8*)(Kt + kt * 32 * 128 + fo.rm[kk]), qf[kk], st, 0, 0, 0);
        if (kt == w) {      // the diagonal tile: key > query -> -inf (this also masks the padded keys >= A for every query < A)
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi > q) st[r] = -INFINITY;
        }
        float tmax = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, st[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * scale_log2;
        // rescale on every tile, per lane (attn_fwd_kernel's wave-uniform lazy rescale would let a row's rounding depend on the
        // other rows of its tile - and so on the active length; with at most three tiles there is nothing to save)
        const float mnew = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        l *= alpha;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
        m = mnew;
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(fmaf(st[r], scale_log2, -m)); psum += st[r]; }
        l += psum;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pb = ca_pack_b(st, ks);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
                oacc[dt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ca_frag_tr(Vt, kt * 32 + ks * 16, fo, dt), pb, oacc[dt], 0, 0, 0);
        }
    }
    if (q < A) {
        const float inv = 1.0f / (l + __shfl_xor(l, 32, 64));
        bf16_t* orow = o + ((long)b * S + q) * ldo + h * 64;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                bf16x4 ov;
#pragma unroll
                for (int e = 0; e < 4; ++e) ov[e] = (bf16_t)(oacc[dt][g * 4 + e] * inv);
                *(bf16x4*)(orow + dt * 32 + 8 * g + 4 * hi) = ov;
            }
    }
}

// =============================================================================================
// fp32
// =============================================================================================
constexpr int CA_KLD = 68;   // K row stride in floats: lane i reads 16 B at i * 272 + c -> 16-B slot (17 i + c / 16) mod 8: conflict-free

template <int NT>
__global__ void __launch_bounds__(NT * 64)
attn_causal_fwd_f32_kernel(const float* __restrict__ qkv, long ld, float* __restrict__ o, long ldo, int H, int S, int A, int W,
                           float scale_log2) {
    constexpr int Sp = NT * 32;
    __shared__ __attribute__((aligned(16))) float Ks[Sp * CA_KLD];
    __shared__ __attribute__((aligned(16))) float Vs[Sp * 64];
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, l31 = lane & 31, hi = lane >> 5;
    const float* base = qkv + (long)b * S * ld + h * 64;
    // rows >= A are zero: their scores are masked, their V rows must be finite
    for (int i = tid; i < Sp * 16; i += NT * 64) {
        const int row = i >> 4, c = (i & 15) * 4;
        float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
        if (row < A) {
            kv = *(const float4*)(base + (long)row * ld + W + c);
            vv = *(const float4*)(base + (long)row * ld + 2 * W + c);
        }
        *(float4*)(Ks + row * CA_KLD + c) = kv;
        *(float4*)(Vs + row * 64 + c) = vv;
    }
    // lane (l31, hi) holds q[32 hi .. 32 hi + 31] of query 32 w + l31, pre-scaled by 0.125 log2(e)
    const int q = w * 32 + l31;
    float qf[32];
    {
        const float* qp = base + (long)min(q, A - 1) * ld + 32 * hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) *(float4*)&qf[4 * j] = *(const float4*)(qp + 4 * j);
#pragma unroll
        for (int j = 0; j < 32; ++j) qf[j] *= scale_log2;
    }
    __syncthreads();
    f32x16 oacc[2];
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 16; ++r) oacc[dt][r] = 0.0f;
    float m = -INFINITY, l = 0.0f;
    for (int kt = 0; kt <= w; ++kt) {
        f32x16 st;
#pragma unroll
        for (int r = 0; r < 16; ++r) st[r] = 0.0f;
        const float* kr = Ks + (kt * 32 + l31) * CA_KLD + 32 * hi;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float4 a = *(const float4*)(kr + 4 * j);
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, qf[4 * j + 0], st, 0, 0, 0);
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, qf[4 * j + 1], st, 0, 0, 0);
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, qf[4 * j + 2], st, 0, 0, 0);
            st = __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, qf[4 * j + 3], st, 0, 0, 0);
        }
        // st[r] = score of key 32 kt + (r & 3) + 8 (r >> 2) + 4 hi against query q
        if (kt == w) {
#pragma unroll
            for (int r = 0; r < 16; ++r)
                if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi > q) st[r] = -INFINITY;
        }
        float tmax = st[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, st[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64));
        const float mnew = fmaxf(m, tmax);
        const float alpha = __builtin_amdgcn_exp2f(m - mnew);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { st[r] = __builtin_amdgcn_exp2f(st[r] - mnew); psum += st[r]; }
        l = fmaf(l, alpha, psum);
        m = mnew;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
        const float* vr = Vs + (kt * 32 + 4 * hi) * 64 + l31;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float* vk = vr + ((r & 3) + 8 * (r >> 2)) * 64;
            oacc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(vk[0], st[r], oacc[0], 0, 0, 0);
            oacc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(vk[32], st[r], oacc[1], 0, 0, 0);
        }
    }
    if (q < A) {
        const float inv = 1.0f / (l + __shfl_xor(l, 32, 64));
        // oacc[dt][4 g + e] = O[q][32 dt + 8 g + 4 hi + e]
        float* orow = o + ((long)b * S + q) * ldo + h * 64 + 4 * hi;
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *(float4*)(orow + 32 * dt + 8 * g) =
                    make_float4(oacc[dt][4 * g] * inv, oacc[dt][4 * g + 1] * inv, oacc[dt][4 * g + 2] * inv, oacc[dt][4 * g + 3] * inv);
    }
}

// =============================================================================================
// launchers
// =============================================================================================
static int attn_causal_check(const void* qkv, const void* o, long ldqkv, long ldo, int B, int H, int S, int active, int align) {
    if (!qkv || !o || B <= 0 || H <= 0) return fail(RVLM_ERR_ARG, "attn_causal_fwd: bad arguments");
    if (S < 1 || S > 96 || active < 1 || active > S) return fail(RVLM_ERR_UNSUPPORTED, "attn_causal_fwd: need 1 <= active <= S <= 96");
    if (ldqkv < 3L * 64 * H || ldo < 64L * H || ldqkv % align || ldo % align || ((size_t)qkv & 15) || ((size_t)o & 15))
        return fail(RVLM_ERR_ARG, "attn_causal_fwd: leading dimensions / alignment");
    return RVLM_OK;
}
static constexpr float CA_SCALE_LOG2 = 0.125f * 1.4426950408889634f;

int attn_causal_fwd_bf16(const bf16_t* qkv, long ldqkv, bf16_t* o, long ldo, int B, int H, int S, int active, hipStream_t s) {
    int rc = attn_causal_check(qkv, o, ldqkv, ldo, B, H, S, active, 8);
    if (rc) return rc;
    const dim3 grid(B * H);
    switch (cdiv(active, 32)) {
        case 1: hipLaunchKernelGGL((attn_causal_fwd_bf16_kernel<1>), grid, dim3(64), 0, s, qkv, ldqkv, o, ldo, H, S, active, 64 * H, CA_SCALE_LOG2); break;
        case 2: hipLaunchKernelGGL((attn_causal_fwd_bf16_kernel<2>), grid, dim3(128), 0, s, qkv, ldqkv, o, ldo, H, S, active, 64 * H, CA_SCALE_LOG2); break;
        default: hipLaunchKernelGGL((attn_causal_fwd_bf16_kernel<3>), grid, dim3(192), 0, s, qkv, ldqkv, o, ldo, H, S, active, 64 * H, CA_SCALE_LOG2); break;
    }
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

int attn_causal_fwd_f32(const float* qkv, long ldqkv, float* o, long ldo, int B, int H, int S, int active, hipStream_t s) {
    int rc = attn_causal_check(qkv, o, ldqkv, ldo, B, H, S, active, 4);
    if (rc) return rc;
    const dim3 grid(B * H);
    switch (cdiv(active, 32)) {
        case 1: hipLaunchKernelGGL((attn_causal_fwd_f32_kernel<1>), grid, dim3(64), 0, s, qkv, ldqkv, o, ldo, H, S, active, 64 * H, CA_SCALE_LOG2); break;
        case 2: hipLaunchKernelGGL((attn_causal_fwd_f32_kernel<2>), grid, dim3(128), 0, s, qkv, ldqkv, o, ldo, H, S, active, 64 * H, CA_SCALE_LOG2); break;
        default: hipLaunchKernelGGL((attn_causal_fwd_f32_kernel<3>), grid, dim3(192), 0, s, qkv, ldqkv, o, ldo, H, S, active, 64 * H, CA_SCALE_LOG2); break;
    }
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

}  // namespace rvlm
