// bf16 flash attention forward / backward for any sequence length whose operands fit LDS (CLIP ViTs: S = 50 / 197 / 577;
// S = 257 goes to attention_bf16_odd.hip), and the dispatchers.  Tile layout and fragment helpers: attention_bf16.h.
//
// Forward: online (running max / sum) softmax; also stores lse2[b,h,q] = m + log2(sum) in the log2 domain of
// (scale*log2e)*q.k for the backward.  Backward = dQ kernel (K,V in LDS; also D = rowsum(dO*O)) + dK/dV kernel (Q,dO in LDS)
// = 7 tile GEMMs instead of the minimal 5; the attention core is ~8 % of the backward FLOPs.
#include "attention_bf16.h"

namespace rvlm {
// LDS of these kernels as functions of the padded row count Sp (byte offsets; tiles are [Sp][64] bf16).  The kernels carve
// smem from them and the launchers request their totals.
struct LdsKV { size_t k, v, total; };                               // forward, dQ: K | V
__host__ __device__ constexpr LdsKV lds_kv(int Sp) {
    return {0, Sp * ATTN_TILE_ROW, 2 * Sp * ATTN_TILE_ROW};
}
struct LdsDkv { size_t q, d_o, k, v, stats, total; };               // dK/dV: Q | dO | [K | V when KV_LDS] | float [2][Sp]: lse2, D
__host__ __device__ constexpr LdsDkv lds_dkv(int Sp, bool kv_lds) {
    const size_t t = Sp * ATTN_TILE_ROW, stats = (kv_lds ? 4 : 2) * t;
    return {0, t, 2 * t, 3 * t, stats, stats + 2 * Sp * sizeof(float)};
}
static_assert(lds_kv(288).total == 288 * 256 && lds_dkv(288, true).total == 288 * 520 && lds_dkv(608, false).total == 608 * 264,
              "the measured LDS requests");
static_assert(lds_kv(ATTN_BF16_MAX_S_FWD).total <= ATTN_LDS_MAX && lds_kv(ATTN_BF16_MAX_S_FWD + 32).total > ATTN_LDS_MAX &&
                  lds_dkv(ATTN_BF16_MAX_S_BWD, false).total <= ATTN_LDS_MAX && lds_dkv(ATTN_BF16_MAX_S_BWD + 32, false).total > ATTN_LDS_MAX,
              "kernels.h: the longest sequences are the ones these layouts fit");
// Q, dO, K, V all LDS-resident in the dK/dV kernel (S <= 315)
static bool dkv_kv_lds(int Sp) { return lds_dkv(Sp, true).total <= ATTN_LDS_MAX; }

// =============================================================================================
// forward
// =============================================================================================
template <bool USE_TR, int MINW>
__global__ void __launch_bounds__(640, MINW)
attn_fwd_kernel(const bf16_t* __restrict__ qkv, long ld, bf16_t* __restrict__ o, long ldo,
                float* __restrict__ lse2, int H, int S, int Sp, int W, float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LdsKV lds = lds_kv(Sp);
    char* Kt = smem + lds.k;
    char* Vt = smem + lds.v;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const bf16_t* base = qkv + (long)b * S * ld + h * 64;
    stage_tile(Kt, base + W, ld, S, Sp, w, nw, lane);
    stage_tile(Vt, base + 2 * W, ld, S, Sp, w, nw, lane);
    __syncthreads();

    const int ntiles = Sp / 32;
    const FragOffs fo = make_offs(lane);
    constexpr float RESCALE_THR = 6.0f;   // log2 units: P stays <= 2^6 between rescales (fp32 accumulate)
    for (int qt = w; qt < ntiles; qt += nw) {
        const int q = qt * 32 + l31;
        const int qc = min(q, S - 1);
        bf16x8 qf[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) qf[kk] = frag_global(base, ld, qc, kk, lane);
        f32x16 oacc[2] = {zero16(), zero16()};
        float m = -INFINITY, l = 0.0f;
        for (int kt = 0; kt < ntiles; ++kt) {
            f32x16 s = zero16();
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) s = MFMA(frag_rm(Kt, kt * 32, fo.rm[kk]), qf[kk], s);
            if (kt * 32 + 32 > S) {   // tail tile: padded keys contribute exp2(-inf) = 0
#pragma unroll
                for (int r = 0; r < 16; ++r)
                    if (kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi >= S) s[r] = -INFINITY;
            }
            float tmax = s[0];
#pragma unroll
            for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, s[r]);
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * scale_log2;
            if (__any(tmax > m + RESCALE_THR)) {   // wave-uniform; always taken on the first tile (m = -inf)
                const float mnew = fmaxf(m, tmax);
                const float alpha = EXP2(m - mnew);
                l *= alpha;
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                    for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
                m = mnew;
            }
            float psum = 0.0f;
#pragma unroll
            for (int r = 0; r < 16; ++r) { s[r] = EXP2(fmaf(s[r], scale_log2, -m)); psum += s[r]; }
            l += psum;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 pb = pack_b(s, ks);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    oacc[dt] = MFMA(frag_t<USE_TR>(Vt, kt * 32 + ks * 16, fo, dt, lane), pb, oacc[dt]);
            }
        }
        const float ltot = l + __shfl_xor(l, 32, 64);
        const float inv = 1.0f / ltot;
        if (q < S) {
            store_row(o + ((long)b * S + q) * ldo + h * 64, oacc, inv, hi);
            if (hi == 0 && lse2) lse2[((long)b * H + h) * Sp + q] = m + log2f(ltot);
        }
    }
}

// =============================================================================================
// backward prep: D[b,h,q] = sum_d dO[q,d] * O[q,d]
// =============================================================================================
__global__ void __launch_bounds__(256)
attn_bwd_prep_kernel(const bf16_t* __restrict__ o, long ldo, const bf16_t* __restrict__ d_o, long lddo,
                     float* __restrict__ dsum, int H, int S, int Sp) {
    const long tok = blockIdx.x;  // b*S + q
    const int b = (int)(tok / S), q = (int)(tok % S);
    const int lane = threadIdx.x & 63;
    for (int h = threadIdx.x >> 6; h < H; h += 4) {
        const float a = (float)o[tok * ldo + h * 64 + lane];
        const float g = (float)d_o[tok * lddo + h * 64 + lane];
        const float v = wave_sum(a * g);
        if (lane == 0) dsum[((long)b * H + h) * Sp + q] = v;
    }
}

// =============================================================================================
// backward dQ: wave owns a query tile, K and V LDS-resident
// =============================================================================================
template <bool USE_TR>
__global__ void __launch_bounds__(640)
attn_bwd_dq_kernel(const bf16_t* __restrict__ qkv, long ld, const bf16_t* __restrict__ o, long ldo,
                   const bf16_t* __restrict__ d_o, long lddo, const float* __restrict__ lse2,
                   float* __restrict__ dsum, bf16_t* __restrict__ dqkv, long lddq, int H, int S, int Sp, int W,
                   float scale, float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LdsKV lds = lds_kv(Sp);
    char* Kt = smem + lds.k;
    char* Vt = smem + lds.v;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const bf16_t* base = qkv + (long)b * S * ld + h * 64;
    stage_tile(Kt, base + W, ld, S, Sp, w, nw, lane);
    stage_tile(Vt, base + 2 * W, ld, S, Sp, w, nw, lane);
    __syncthreads();

    const int ntiles = Sp / 32;
    const FragOffs fo = make_offs(lane);
    for (int qt = w; qt < ntiles; qt += nw) {
        const int q = qt * 32 + l31;
        const int qc = min(q, S - 1);
        bf16x8 qf[4], dof[4];
        // D[q] = sum_d dO[q,d] * O[q,d]  (the "prep" pass of flash backward, fused here: this lane holds
        // 32 of the 64 d's of dO as its MFMA fragments, the other half sits in lane ^ 32)
        float dq_sum = 0.0f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            qf[kk] = frag_global(base, ld, qc, kk, lane);
            dof[kk] = frag_global(d_o + (long)b * S * lddo + h * 64, lddo, qc, kk, lane);
            const bf16x8 of = frag_global(o + (long)b * S * ldo + h * 64, ldo, qc, kk, lane);
#pragma unroll
            for (int e = 0; e < 8; ++e) dq_sum = fmaf((float)dof[kk][e], (float)of[e], dq_sum);
        }
        dq_sum += __shfl_xor(dq_sum, 32, 64);
        if (hi == 0 && q < S) dsum[((long)b * H + h) * Sp + q] = dq_sum;   // consumed by the dK/dV kernel
        const float lq = lse2[((long)b * H + h) * Sp + qc];
        f32x16 acc[2] = {zero16(), zero16()};
        for (int kt = 0; kt < ntiles; ++kt) {
            f32x16 s = zero16(), dp = zero16();
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                s = MFMA(frag_rm(Kt, kt * 32, fo.rm[kk]), qf[kk], s);
                dp = MFMA(frag_rm(Vt, kt * 32, fo.rm[kk]), dof[kk], dp);
            }
            const bool tail = (kt * 32 + 32 > S);
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float p = EXP2(fmaf(s[r], scale_log2, -lq));
                if (tail) {
                    const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
                    if (key >= S) p = 0.0f;
                }
                s[r] = p * (dp[r] - dq_sum);   // dS^T
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 db = pack_b(s, ks);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt)
                    acc[dt] = MFMA(frag_t<USE_TR>(Kt, kt * 32 + ks * 16, fo, dt, lane), db, acc[dt]);
            }
        }
        if (q < S) store_row(dqkv + ((long)b * S + q) * lddq + h * 64, acc, scale, hi);
    }
}

// =============================================================================================
// backward dK, dV: wave owns a key tile, Q and dO LDS-resident
// =============================================================================================
template <bool USE_TR, bool KV_LDS>
__global__ void __launch_bounds__(640)
attn_bwd_dkv_kernel(const bf16_t* __restrict__ qkv, long ld, const bf16_t* __restrict__ d_o, long lddo,
                    const float* __restrict__ lse2, const float* __restrict__ dsum,
                    bf16_t* __restrict__ dqkv, long lddq, int H, int S, int Sp, int W, float scale,
                    float scale_log2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const LdsDkv lds = lds_dkv(Sp, KV_LDS);
    char* Qt = smem + lds.q;
    char* Dt = smem + lds.d_o;
    char* Kt = smem + lds.k;
    char* Vt = smem + lds.v;
    float* Ls = (float*)(smem + lds.stats);
    float* Ds = Ls + Sp;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, nw = blockDim.x >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    const bf16_t* base = qkv + (long)b * S * ld + h * 64;
    stage_tile(Qt, base, ld, S, Sp, w, nw, lane);
    stage_tile(Dt, d_o + (long)b * S * lddo + h * 64, lddo, S, Sp, w, nw, lane);
    if (KV_LDS) {
        stage_tile(Kt, base + W, ld, S, Sp, w, nw, lane);
        stage_tile(Vt, base + 2 * W, ld, S, Sp, w, nw, lane);
    }
    for (int i = tid; i < Sp; i += blockDim.x) {
        Ls[i] = (i < S) ? lse2[((long)b * H + h) * Sp + i] : INFINITY;   // pad rows -> p = 0
        Ds[i] = (i < S) ? dsum[((long)b * H + h) * Sp + i] : 0.0f;
    }
    __syncthreads();

    const int ntiles = Sp / 32;
    const FragOffs fo = make_offs(lane);
    for (int kt = w; kt < ntiles; kt += nw) {
        const int key = kt * 32 + l31;
        const int kc = min(key, S - 1);
        bf16x8 kf[4], vf[4];
        if (!KV_LDS) {
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                kf[kk] = frag_global(base + W, ld, kc, kk, lane);
                vf[kk] = frag_global(base + 2 * W, ld, kc, kk, lane);
            }
        }
        f32x16 dk[2] = {zero16(), zero16()}, dv[2] = {zero16(), zero16()};
        for (int qt = 0; qt < ntiles; ++qt) {
            f32x16 s = zero16(), dp = zero16();
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const bf16x8 kb = KV_LDS ? frag_rm(Kt, kt * 32, fo.rm[kk]) : kf[kk];
                const bf16x8 vb = KV_LDS ? frag_rm(Vt, kt * 32, fo.rm[kk]) : vf[kk];
                s = MFMA(frag_rm(Qt, qt * 32, fo.rm[kk]), kb, s);     // S[q][key]
                dp = MFMA(frag_rm(Dt, qt * 32, fo.rm[kk]), vb, dp);   // dP[q][key]
                __builtin_amdgcn_sched_barrier(0);   // bound the live fragment set (3 waves/SIMD budget)
            }
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 lq = *(const float4*)(Ls + qt * 32 + 8 * g + 4 * hi);
                const float4 dq = *(const float4*)(Ds + qt * 32 + 8 * g + 4 * hi);
                const float lqa[4] = {lq.x, lq.y, lq.z, lq.w};
                const float dqa[4] = {dq.x, dq.y, dq.z, dq.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float p = EXP2(fmaf(s[g * 4 + e], scale_log2, -lqa[e]));
                    s[g * 4 + e] = p;                                   // P   (in place)
                    dp[g * 4 + e] = p * (dp[g * 4 + e] - dqa[e]);       // dS  (in place)
                }
            }
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                const bf16x8 pb = pack_b(s, ks), db = pack_b(dp, ks);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    dv[dt] = MFMA(frag_t<USE_TR>(Dt, qt * 32 + ks * 16, fo, dt, lane), pb, dv[dt]);
                    dk[dt] = MFMA(frag_t<USE_TR>(Qt, qt * 32 + ks * 16, fo, dt, lane), db, dk[dt]);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        if (key < S) {
            bf16_t* krow = dqkv + ((long)b * S + key) * lddq + W + h * 64;
            bf16_t* vrow = krow + W;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {     // (dK and dV interleaved, not two store_row(): the order is part of the code)
                    const bf16x4 ok = acc_bf16x4(dk, dt, g, scale), ov = acc_bf16x4(dv, dt, g, 1.0f);
                    *(bf16x4*)(krow + dt * 32 + 8 * g + 4 * hi) = ok;
                    *(bf16x4*)(vrow + dt * 32 + 8 * g + 4 * hi) = ov;
                }
        }
    }
}

}  // namespace rvlm

// The S = 32 NK + 1 kernels and their launch functions are a file of their own but belong to THIS translation unit: compiled
// apart from the fused backward, every generic kernel above comes out with different code ("source shape").
#include "attention_bf16_odd.hip"

namespace rvlm {
// ---------------------------------------------------------------------------------------------
static bool g_use_tr = true;
void attn_set_use_tr(int on) { g_use_tr = on != 0; }

const AttnEnv& attn_env() {
    static const AttnEnv e = {env_int("RVLM_ATTN_OCC", 5),     env_int("RVLM_ATTN_FWD_ODD", 1), env_int("RVLM_ATTN_FUSED", 1),
                              env_int("RVLM_ATTN_PERSIST", 1), env_int("RVLM_ATTN_TRACE", 0),   env_int("RVLM_ATTN_DESYNC", 0)};
    return e;
}

static int attn_block_threads(int ntiles) {
    // one 32-row tile per wave and round, up to 10 waves: the fewest rounds, then the fewest waves that give them
    // (S = 257 -> 9 tiles -> 9 waves; S = 577 -> 19 tiles -> 2 rounds of 10 waves - with 9 waves it took 3 rounds, 27 wave
    // slots for 19 tiles of work; 10 waves still are at most 3 per SIMD, the register budget of 9)
    const int rounds = (ntiles + 9) / 10;
    return ((ntiles + rounds - 1) / rounds) * 64;
}

template <bool TR, int MINW>
static int launch_fwd(const bf16_t* qkv, long ldqkv, bf16_t* o, long ldo, float* lse, int B, int H, int S, hipStream_t s) {
    const int Sp = (int)round_up(S, 32);
    const size_t lds = lds_kv(Sp).total;
    if (int rc = set_lds(attn_fwd_kernel<TR, MINW>, lds)) return rc;
    hipLaunchKernelGGL((attn_fwd_kernel<TR, MINW>), dim3(B * H), dim3(attn_block_threads(Sp / 32)), lds, s, qkv, ldqkv, o, ldo,
                       lse, H, S, Sp, H * 64, 0.125f * 1.4426950408889634f);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

int attn_fwd_bf16(const bf16_t* qkv, long ldqkv, bf16_t* o, long ldo, float* lse, int B, int H,
                  int S, hipStream_t s) {
    if (S > ATTN_BF16_MAX_S_FWD) return fail(RVLM_ERR_UNSUPPORTED, "attention: sequence too long for LDS-resident K/V");
    if (attn_env().fwd_odd && g_use_tr && S == ATTN_ODD_S) return attn_fwd_odd_launch(qkv, ldqkv, o, ldo, lse, B, H, s);
    if (!g_use_tr) return launch_fwd<false, 1>(qkv, ldqkv, o, ldo, lse, B, H, S, s);
    // MINW = 5 caps the kernel at 96 VGPRs so that two 9-wave workgroups (2 x 74 KiB LDS) share a CU:
    // one workgroup's K/V staging then hides under the other's MFMA/softmax phase.
    // (two workgroups share a CU only if their K / V tiles fit twice: at S = 577 the 96-register cap would buy nothing)
    if (attn_env().occ == 5 && 2 * lds_kv((int)round_up(S, 32)).total <= ATTN_LDS_MAX)
        return launch_fwd<true, 5>(qkv, ldqkv, o, ldo, lse, B, H, S, s);
    return launch_fwd<true, 1>(qkv, ldqkv, o, ldo, lse, B, H, S, s);
}

// the two-kernel backward; both kernels' LDS requests are checked before the first one is enqueued
template <bool TR, bool KV_LDS>
static int launch_bwd(const bf16_t* qkv, long ldqkv, const bf16_t* o, long ldo, const bf16_t* d_o, long lddo, const float* lse,
                      float* dsum_scratch, bf16_t* dqkv, long lddqkv, int B, int H, int S, hipStream_t s) {
    const int Sp = (int)round_up(S, 32), W = H * 64, nt = attn_block_threads(Sp / 32);
    const float scale = 0.125f, sl2 = 0.125f * 1.4426950408889634f;
    const size_t lds_q = lds_kv(Sp).total, lds_k = lds_dkv(Sp, KV_LDS).total;
    if (int rc = set_lds(attn_bwd_dq_kernel<TR>, lds_q)) return rc;
    if (int rc = set_lds(attn_bwd_dkv_kernel<TR, KV_LDS>, lds_k)) return rc;
    hipLaunchKernelGGL((attn_bwd_dq_kernel<TR>), dim3(B * H), dim3(nt), lds_q, s, qkv, ldqkv, o, ldo, d_o, lddo, lse,
                       dsum_scratch, dqkv, lddqkv, H, S, Sp, W, scale, sl2);
    RVLM_CHECK_LAUNCH();
    hipLaunchKernelGGL((attn_bwd_dkv_kernel<TR, KV_LDS>), dim3(B * H), dim3(nt), lds_k, s, qkv, ldqkv, d_o, lddo, lse,
                       dsum_scratch, dqkv, lddqkv, H, S, Sp, W, scale, sl2);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

int attn_bwd_bf16(const bf16_t* qkv, long ldqkv, const bf16_t* o, long ldo, const bf16_t* d_o,
                  long lddo, const float* lse, float* dsum_scratch, bf16_t* dqkv, long lddqkv,
                  int B, int H, int S, hipStream_t s) {
    if (S > ATTN_BF16_MAX_S_BWD) return fail(RVLM_ERR_UNSUPPORTED, "attention: sequence too long for the LDS-resident backward");
    if (attn_env().fused && g_use_tr && S == ATTN_ODD_S)
        return attn_bwd_fused_launch(qkv, ldqkv, o, ldo, d_o, lddo, lse, dsum_scratch, dqkv, lddqkv, B, H, s);
    const bool kv_lds = dkv_kv_lds((int)round_up(S, 32));
    auto* launch = g_use_tr ? (kv_lds ? launch_bwd<true, true> : launch_bwd<true, false>)
                            : (kv_lds ? launch_bwd<false, true> : launch_bwd<false, false>);
    return launch(qkv, ldqkv, o, ldo, d_o, lddo, lse, dsum_scratch, dqkv, lddqkv, B, H, S, s);
}

// occupancy (workgroups per CU) the runtime reports for the three kernels at sequence length S
int attn_occupancy(int S, int* out3) {
    const int Sp = (int)round_up(S, 32);
    const int nt = attn_block_threads(Sp / 32);
    const size_t lds = lds_kv(Sp).total;
    int rc;
    if ((rc = set_lds(attn_fwd_kernel<true, 5>, lds))) return rc;
    if ((rc = set_lds(attn_fwd_kernel<true, 1>, lds))) return rc;
    if ((rc = set_lds(attn_bwd_dq_kernel<true>, lds))) return rc;
    RVLM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out3[0], attn_fwd_kernel<true, 5>, nt, lds));
    RVLM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out3[1], attn_fwd_kernel<true, 1>, nt, lds));
    RVLM_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&out3[2], attn_bwd_dq_kernel<true>, nt, lds));
    return RVLM_OK;
}

}  // namespace rvlm
