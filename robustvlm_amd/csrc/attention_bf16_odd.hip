// bf16 flash attention for S = 32 NK + 1 (CLIP ViTs at 224 px: 257 = 256 patch tokens + the class token), the kernels the
// headline runs: NK waves own one 32-row tile each, no padded tiles; the odd token is folded in on the side.
// Tile layout and fragment helpers: attention_bf16.h.  Not a translation unit of its own: attention_bf16.hip includes this file
// (the generic kernels' code depends on the fused backward being compiled with them) and its dispatchers call the two launch
// functions at the end.
#include "attention_bf16.h"

namespace rvlm {
// =============================================================================================
// forward, S = 32 NK + 1 (257 = 256 patch tokens + the class token): NK waves, no padded tiles.
// The generic kernel pads S to NK + 1 tiles each way: 81 MFMA/softmax blocks for 64.5 blocks of work, and its 9th
// wave (one valid query) makes 9 waves share 4 SIMDs.  Here wave w owns query tile w and walks the NK full key
// tiles; the odd key (token S-1) is folded in with VALU dot products (one score per query: 32 FMAs + a shuffle, no
// MFMA block); the odd query (row S-1) is split over the waves - wave w evaluates it against key tile w - and the NK
// partial (max, sum, O) triples are merged through 2 KiB of LDS.
// =============================================================================================
// LDS: K | V | mrg [NK][66] floats (m, sum, O[64] of the odd query per key tile) | pst [NK][32] bf16 (p of the odd query,
// staged into B-operand order).  The kernel carves smem from it, the launcher requests TOTAL.
template <int NK>
struct FwdOddLds {
    static constexpr int Sp = 32 * NK + 32;
    static constexpr size_t K = 0, V = K + Sp * ATTN_TILE_ROW, MRG = V + Sp * ATTN_TILE_ROW, PST = MRG + NK * 66 * sizeof(float),
                            TOTAL = PST + NK * 32 * sizeof(bf16_t);
    static_assert(TOTAL <= ATTN_LDS_MAX, "K and V do not fit LDS");
};
static_assert(FwdOddLds<8>::TOTAL == 288 * 256 + 8 * 66 * 4 + 8 * 64, "the measured LDS request");

// One (image, head) with K and V staged in LDS (Kt / Vt).  Ends with the workgroup barrier + wave 0's merge of the odd query.
template <int NK>
__device__ __forceinline__ void attn_fwd_odd_head(const char* Kt, const char* Vt, float* mrg, bf16_t* pst_all, const bf16_t* base, long ld,
                                                  bf16_t* obase, long ldo, float* lse_bh, float scale_log2, int lane, int w) {
    constexpr int S = 32 * NK + 1;
    const int l31 = lane & 31, hi = lane >> 5;
    const FragOffs fo = make_offs(lane);
    constexpr float RESCALE_THR = 6.0f;
    // row S-1 = 32 NK of a tile: swz_key(row) == 0, i.e. its chunks are not swizzled
    const char* kl = Kt + (S - 1) * 128;
    const char* vl = Vt + (S - 1) * 128;

    auto rescale = [&](float tmax, float& m, float& l, f32x16 (&oacc)[2]) {
        if (__any(tmax > m + RESCALE_THR)) {
            const float mnew = fmaxf(m, tmax);
            const float alpha = EXP2(m - mnew);
            l *= alpha;
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int r = 0; r < 16; ++r) oacc[dt][r] *= alpha;
            m = mnew;
        }
    };
    auto block = [&](const bf16x8 (&qf)[4], int kt, float& m, float& l, f32x16 (&oacc)[2]) {
        f32x16 sc = zero16();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) sc = MFMA(frag_rm(Kt, kt * 32, fo.rm[kk]), qf[kk], sc);
        float tmax = sc[0];
#pragma unroll
        for (int r = 1; r < 16; ++r) tmax = fmaxf(tmax, sc[r]);
        tmax = fmaxf(tmax, __shfl_xor(tmax, 32, 64)) * scale_log2;
        rescale(tmax, m, l, oacc);
        float psum = 0.0f;
#pragma unroll
        for (int r = 0; r < 16; ++r) { sc[r] = EXP2(fmaf(sc[r], scale_log2, -m)); psum += sc[r]; }
        l += psum;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pb = pack_b(sc, ks);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) oacc[dt] = MFMA(frag_tr(Vt, kt * 32 + ks * 16, fo, dt), pb, oacc[dt]);
        }
    };
    // the odd key: one score per query (this lane holds 32 of its query's 64 dims, lane ^ 32 the others)
    auto odd_key = [&](const bf16x8 (&qf)[4], float& m, float& l, f32x16 (&oacc)[2]) {
        float sc = 0.0f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            const bf16x8 kv = *(const bf16x8*)(kl + (kk * 2 + hi) * 16);
#pragma unroll
            for (int e = 0; e < 8; ++e) sc = fmaf((float)qf[kk][e], (float)kv[e], sc);
        }
        sc += __shfl_xor(sc, 32, 64);
        rescale(sc * scale_log2, m, l, oacc);
        const float pj = EXP2(fmaf(sc, scale_log2, -m));
        if (hi == 0) l += pj;                       // l is a per-lane partial (summed over the two halves at the end)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const bf16x4 vv = *(const bf16x4*)(vl + (dt * 32 + 8 * g + 4 * hi) * 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) oacc[dt][g * 4 + e] = fmaf(pj, (float)vv[e], oacc[dt][g * 4 + e]);
            }
    };

    {   // ---- this wave's 32 queries ----
        const int q = w * 32 + l31;
        bf16x8 qf[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) qf[kk] = frag_global(base, ld, q, kk, lane);
        f32x16 oacc[2] = {zero16(), zero16()};
        float m = -INFINITY, l = 0.0f;
        // (Two score tiles in flight - the S MFMAs of key tile kt + 1 issued in front of the softmax arithmetic of tile kt, T15 of
        // the guide - measured SLOWER here, 75-77 against 72-74 us on one box, profiles/r05_attn_ab_fwd_two_tiles_in_flight.log: with
        // four waves per SIMD the partner waves already fill the gaps, and the form costs 13 registers and a recomputed last tile.)
#pragma unroll 1
        for (int kt = 0; kt < NK; ++kt) block(qf, kt, m, l, oacc);
        odd_key(qf, m, l, oacc);
        const float ltot = l + __shfl_xor(l, 32, 64);
        const float inv = 1.0f / ltot;
        bf16_t* orow = obase + (long)q * ldo;
        // A lane holds 4 consecutive d per (dt, g) and its partner lane ^ 32 the next 4: v_permlane32_swap pairs the two
        // 8-byte halves of the even chunk on the lower lanes and of the odd chunk on the upper lanes, so that the row leaves
        // as four 16-byte stores per lane instead of eight 8-byte ones (the store tail of this kernel is issue-bound).
#pragma unroll
        for (int dt = 0; dt < 2; ++dt)
#pragma unroll
            for (int pr = 0; pr < 2; ++pr) {
                bf16x4 ev, od;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    ev[e] = (bf16_t)(oacc[dt][(2 * pr) * 4 + e] * inv);
                    od[e] = (bf16_t)(oacc[dt][(2 * pr + 1) * 4 + e] * inv);
                }
                typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
                typedef unsigned u32x4v __attribute__((ext_vector_type(4)));
                const u32x2v e2 = __builtin_bit_cast(u32x2v, ev), o2 = __builtin_bit_cast(u32x2v, od);
                // (vdst, src) -> vdst keeps its lower lanes and takes src's lower lanes into its upper half; src takes
                // vdst's upper lanes into its lower half
                const auto r0 = __builtin_amdgcn_permlane32_swap(e2[0], o2[0], false, false);
                const auto r1 = __builtin_amdgcn_permlane32_swap(e2[1], o2[1], false, false);
                const u32x4v out = {r0[0], r1[0], r0[1], r1[1]};
                *(u32x4v*)(orow + dt * 32 + 16 * pr + 8 * hi) = out;
            }
        if (hi == 0 && lse_bh) lse_bh[q] = m + log2f(ltot);
    }
    {   // ---- the odd query against key tile w, in the TRANSPOSED orientation: S = q K^T has the keys on the lanes and the
        // (identical) query rows on the registers, so the softmax costs one exp per lane instead of sixteen; p goes
        // through 64 B of LDS into the B-operand layout of the P.V product ----
        bf16x8 qf[4];
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) qf[kk] = frag_global(base, ld, S - 1, kk, lane);
        f32x16 st = zero16();
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) st = MFMA(qf[kk], frag_rm(Kt, w * 32, fo.rm[kk]), st);
        const float sc = st[0] * scale_log2;                  // key w*32 + l31 (same value on both lane halves)
        float m = sc;
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
        const float pj = EXP2(sc - m);
        float l = pj;
#pragma unroll
        for (int off = 1; off < 32; off <<= 1) l += __shfl_xor(l, off, 64);
        bf16_t* pst = pst_all + w * 32;
        if (hi == 0) pst[l31] = (bf16_t)pj;
        f32x16 oacc[2] = {zero16(), zero16()};
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x4 lo = *(const bf16x4*)(pst + 16 * ks + 4 * hi), up = *(const bf16x4*)(pst + 16 * ks + 8 + 4 * hi);
            bf16x8 pb;
#pragma unroll
            for (int t = 0; t < 4; ++t) { pb[t] = lo[t]; pb[4 + t] = up[t]; }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) oacc[dt] = MFMA(frag_tr(Vt, w * 32 + ks * 16, fo, dt), pb, oacc[dt]);
        }
        if (w == 0) odd_key(qf, m, l, oacc);                  // l is the wave total here: lane 0's copy is the one kept
        if (l31 == 0) {
            float* dst = mrg + w * 66;
            if (hi == 0) { dst[0] = m; dst[1] = l; }
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g)
#pragma unroll
                    for (int e = 0; e < 4; ++e) dst[2 + dt * 32 + 8 * g + 4 * hi + e] = oacc[dt][g * 4 + e];
        }
    }
    __syncthreads();
    if (w == 0) {   // merge: lane = head dim
        float M = -INFINITY;
#pragma unroll
        for (int i = 0; i < NK; ++i) M = fmaxf(M, mrg[i * 66]);
        float L = 0.0f, O = 0.0f;
#pragma unroll
        for (int i = 0; i < NK; ++i) {
            const float c = EXP2(mrg[i * 66] - M);
            L = fmaf(mrg[i * 66 + 1], c, L);
            O = fmaf(mrg[i * 66 + 2 + lane], c, O);
        }
        obase[(long)(S - 1) * ldo + lane] = (bf16_t)(O / L);
        if (lane == 0 && lse_bh) lse_bh[S - 1] = M + log2f(L);
    }
}

template <int NK>
__global__ void __launch_bounds__(NK * 64, 4)    // 4 waves per SIMD = two 8-wave workgroups per CU (128 VGPRs)
attn_fwd_odd_kernel(const bf16_t* __restrict__ qkv, long ld, bf16_t* __restrict__ o, long ldo,
                    float* __restrict__ lse2, int H, long W, float scale_log2, AttnLayout lay) {
    using Lds = FwdOddLds<NK>;
    constexpr int S = 32 * NK + 1, Sp = Lds::Sp;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Kt = smem + Lds::K;
    char* Vt = smem + Lds::V;
    const int b = blockIdx.x / H, h = blockIdx.x % H;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const bf16_t* base = qkv + (long)b * lay.qkv_b + (long)h * lay.qkv_h;   // (W = element offset from Q to K, K to V)
    stage_tile(Kt, base + W, ld, S, Sp, w, NK, lane);
    stage_tile(Vt, base + 2 * W, ld, S, Sp, w, NK, lane);
    __syncthreads();
    attn_fwd_odd_head<NK>(Kt, Vt, (float*)(smem + Lds::MRG), (bf16_t*)(smem + Lds::PST), base, ld,
                          o + (long)b * lay.o_b + (long)h * lay.o_h, ldo, lse2 ? lse2 + ((long)b * H + h) * Sp : nullptr,
                          scale_log2, lane, w);
}

// =============================================================================================
// backward, FUSED (dQ, dK, dV in one kernel) for sequence lengths S = 32*NK + 1 (CLIP ViTs at 224 px: 257 = 8*32 + 1)
//
// The two-kernel backward of attention_bf16.hip evaluates P and dS twice (once per kernel: exp2 + ~8 VALU per score, the bound of both
// kernels) and runs 9 waves on 4 SIMDs (one SIMD carries 3).  Here NK = 8 waves (2 per SIMD, <= 256 VGPRs each) own one
// 32-key tile each - K, V fragments and the dK, dV accumulators stay in registers - and walk the 9 query tiles in
// lockstep, ONE barrier per tile:
//     S, dP (8 MFMA 32x32x16) -> P, dS once, in registers -> the wave's dS tile [32 keys][32 q] to LDS -> barrier ->
//     dV, dK from the registers (8 MFMA) ; dQ: wave w OWNS the 16 (d) x 16 (q) block (w >> 1, w & 1) of the tile's dQ^T
//     and contracts it over ALL 256 keys - K^T fragments of the NK key tiles held in registers against the NK waves'
//     dS tiles read back through ds_read_b64_tr_b16 (NK v_mfma_f32_16x16x32_bf16) -> 8-byte stores of finished dQ.
// = 5 tile GEMMs per (query tile, key tile), P / dS evaluated once, and NO partial sums cross waves: round 1 summed eight
// fp32 32x64 partials per tile through 64 KiB of LDS with two barriers (3.8 k cycles per tile, now 2.7 k).  The dS tiles
// are double-buffered by tile parity, which is what makes one barrier per tile enough.  The result is a deterministic
// function of the inputs (fixed MFMA accumulation order).  dK / dV leave through a wave-private LDS transpose as 16-byte
// full-line stores (the row-per-lane 8-byte store tail was 10 % of the kernel, now 4 %).
//
// The odd key (index S-1, the "+1") is handled up front (phase "fragments") in the transposed orientation, where it is ONE
// accumulator register instead of a 32-wide tile: S^T, dP^T by MFMA against the padded last key tile, p and dS for that
// key on one register per lane, dK/dV of that key by MFMA against a one-column B operand; its rank-1 contribution to dQ
// (dS[q] * k) joins the owner's block before the store.  The odd QUERY rides in the ninth query tile (31 padded rows,
// lse = +inf -> P = 0); its rows as 64-wide vectors are requested under the staging.
//
// LDS: BwdFusedLds below.  Measured (MI355X, B = 128, 16 heads; profiles/r02_attn_bwd_*.log): 262 -> 206 us per launch.
// =============================================================================================
constexpr int DS_KEY_SHIFT = 1;  // dS-tile swizzle: 8-B chunk index XOR ((key >> DS_KEY_SHIFT) & 7), see the tile loop

// LDS map of the fused backward (byte offsets; S = 257: Q 36 KiB | dO 36 KiB | area 72 KiB | small arrays 9.6 KiB).  The area
// holds the K and V tiles until the fragments are in registers, then the dS tiles with the store staging behind them.
template <int NK>
struct BwdFusedLds {
    static constexpr int NT = NK + 1, Sp = NT * 32;            // query tiles, padded rows
    static constexpr size_t TILE = Sp * ATTN_TILE_ROW;
    static constexpr int DS_TILE = 2048, STAGE_TILE = 4096;    // one wave's dS tile [32 keys][32 q] bf16; its dK / dV store staging
    static constexpr size_t Q = 0, DO = Q + TILE, AREA = DO + TILE,
                            K = AREA, V = K + TILE,                          // phases 0-1
                            DS = AREA, STAGE = DS + 2 * NK * DS_TILE,        // phases 2-3: [2][NK] dS tiles | [NK] staging tiles
                            LSE = AREA + 2 * TILE,                           // float [Sp] each: lse2, D, p[q][odd key], dS[q][odd key]
                            D = LSE + Sp * sizeof(float), PE = D + Sp * sizeof(float), DE = PE + Sp * sizeof(float),
                            KE = DE + Sp * sizeof(float),                    // float [64]: k[odd key]
                            KVE = KE + 64 * sizeof(float),                   // float [NK + 1][2][64]: dK / dV of the odd key per wave
                                                                             // (+ the odd query's)
                            UNUSED = KVE + (NK + 1) * 128 * sizeof(float),   // 512 bytes nothing touches (the removed next-head
                            TOTAL = UNUSED + 512;                            // prefetch kept the odd token's rows here): the
                                                                             // request stays the measured one
    static_assert(STAGE + NK * STAGE_TILE <= LSE, "dS tiles + store staging outgrow the K / V area");
    static_assert(TOTAL <= ATTN_LDS_MAX, "the fused backward does not fit LDS");
};
static_assert(BwdFusedLds<8>::TOTAL == 288 * 512 + (4 * 288 + 64 + 9 * 128) * 4 + 4 * 128, "the measured LDS request");

template <int NK>
__global__ void __launch_bounds__(NK * 64)
attn_bwd_fused_kernel(const bf16_t* __restrict__ qkv, long ld, const bf16_t* __restrict__ o, long ldo,
                      const bf16_t* __restrict__ d_o, long lddo, const float* __restrict__ lse2,
                      bf16_t* __restrict__ dqkv, long lddq, int H, int S, long W, float scale, float scale_log2,
                      unsigned long long* __restrict__ trace, int desync, AttnLayout lay, int nbh) {
    // Phase offset: every CU would otherwise stage its head at the same moment (6 TB/s-bound, 22 % of the kernel spent
    // waiting for HBM) and compute at the same moment (HBM idle).  The first workgroup of each CU starts up to 7 x desync
    // kilo-cycles late; the stagger then persists, one CU's staging hides under the others' compute.  (RVLM_ATTN_DESYNC,
    // default 0 since round 3: worth 5 % on the one-head-per-workgroup kernel of round 1, but the persistent kernel requests
    // the next head's Q / dO under its tile loop and then the late start only costs its tail - in-pipeline attention
    // backward 46.5 ms per step at 5, 44.9 at 0, 49.3 at 9; two phases 4-8 k cycles apart: 195 vs 202 us in the micro-benchmark,
    // 44.5 vs 44.7 ms in the pipeline; profiles/r03_ab_attn_desync.log)
    const int trace_mode = desync >> 8;       // (RVLM_ATTN_TRACE=2: per-wave duration of the fragments phase instead of the phase stamps)
    desync &= 255;
    if (desync > 0 && blockIdx.x < 256) {
        for (int i = 0; i < (int)((blockIdx.x >> 3) & 7) * desync; ++i) __builtin_amdgcn_s_sleep(16);   // 16 x 64 cycles
    }
    using Lds = BwdFusedLds<NK>;
    constexpr int NT = Lds::NT, Sp = Lds::Sp, SE = NK * 32, DS_TILE = Lds::DS_TILE;   // query tiles, padded rows, index of the odd key
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* Qt = smem + Lds::Q;
    char* Dt = smem + Lds::DO;
    char* Kt = smem + Lds::K;
    char* Vt = smem + Lds::V;
    float* Ls = (float*)(smem + Lds::LSE);
    float* Ds = (float*)(smem + Lds::D);
    float* Pe = (float*)(smem + Lds::PE);
    float* De = (float*)(smem + Lds::DE);
    float* Ke = (float*)(smem + Lds::KE);
    float* KVe = (float*)(smem + Lds::KVE);
    // PERSISTENT over the (image, head) pairs bh = blockIdx.x, + gridDim.x, ... (the launcher gives <= 256 workgroups when
    // RVLM_ATTN_PERSIST is on): while a head's query-tile loop runs, the NEXT head's Q and dO tiles are requested into the
    // LDS tile slots the loop has finished with (one 1-KiB DMA per wave and step, through inline asm: a compiler-visible
    // LDS-DMA would make hipcc drain vmcnt in front of every LDS read that might alias it).  A CU pulls HBM misses at only
    // ~12 B per clock, so the 144 KB staging of a head cost 27 % of the kernel; half of it now arrives under the loop.
    bool have_qd = false;       // Q / dO of the head about to start are already in LDS
    for (int bh = blockIdx.x; bh < nbh; bh += gridDim.x) {
    // (opaque per iteration: otherwise every lane-derived offset of the phases below is hoisted out of this loop, lives
    // across the whole head - 256 VGPRs, 52 spilled dwords - and the kernel ran 40 % slower than its one-head form)
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    const int lane = tid & 63, w = tid >> 6;
    const int l31 = lane & 31, hi = lane >> 5;
    // optional phase timeline (RVLM_ATTN_TRACE=1: 5 s_memtime stamps per head into the dsum scratch buffer)
    auto stamp = [&](int k) {
        if (trace && trace_mode < 2 && tid == 0) trace[(long)bh * 8 + k] = __builtin_amdgcn_s_memtime();
    };
    stamp(0);
    const int b = bh / H, h = bh % H;
    const int nxt = bh + (int)gridDim.x;
    const bool prefetch_next = nxt < nbh;
    const bf16_t* base = qkv + (long)b * lay.qkv_b + (long)h * lay.qkv_h;
    const bf16_t* dob = d_o + (long)b * lay.o_b + (long)h * lay.o_h;
    const bf16_t* ob = o + (long)b * lay.o_b + (long)h * lay.o_h;
    // the next head's Q / dO blocks (8 rows = one DMA instruction): wave w < 4 takes block 4 t + w of Q, the others of dO
    const bf16_t* nsrc = nullptr;
    if (prefetch_next) {
        const int nb = nxt / H, nh = nxt % H;
        nsrc = w < 4 ? qkv + (long)nb * lay.qkv_b + (long)nh * lay.qkv_h : d_o + (long)nb * lay.o_b + (long)nh * lay.o_h;
    }
    const long nld = w < 4 ? ld : lddo;
    // ==== phase 0, STAGE: Q, dO (unless they came in under the previous head's loop), K, V; lse =============================
    if (!have_qd) {
        stage_tile(Qt, base, ld, S, Sp, w, NK, lane);
        stage_tile(Dt, dob, lddo, S, Sp, w, NK, lane);
    }
    bf16x8 ofr[4];   // O rows of this wave's query tile (for D = rowsum(dO * O)): requested under the staging
    stage_tile(Kt, base + W, ld, S, Sp, w, NK, lane);
    stage_tile(Vt, base + 2 * W, ld, S, Sp, w, NK, lane);
    for (int i = tid; i < Sp; i += NK * 64) Ls[i] = (i < S) ? lse2[((long)b * H + h) * Sp + i] : INFINITY;
    if (tid < 64) Ke[tid] = (float)base[(long)SE * ld + W + tid];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) ofr[kk] = frag_global(ob, ldo, w * 32 + (lane & 31), kk, lane);
    // the odd query's rows as 64-wide vectors (ONE wave), requested under the staging as well: fetched in the next phase they put
    // an HBM round trip on the path to the phase's barrier.  That wave is wave 0: per-wave stamps (RVLM_ATTN_TRACE=2) put
    // the first-dispatched waves 0-3 at the phase's barrier after 4.3 k cycles, waves 4-6 after 5.6 k, and the wave that
    // carries these 1.7 k cycles of serial shuffles on top - it used to be the last one - after 7.3 k
    constexpr int ODD_Q_WAVE = 0;
    float odd_do = 0.0f, odd_o = 0.0f, odd_q = 0.0f, odd_v = 0.0f;
    if (w == ODD_Q_WAVE) {
        odd_do = (float)dob[(long)SE * lddo + lane]; odd_o = (float)ob[(long)SE * ldo + lane];
        odd_q = (float)base[(long)SE * ld + lane]; odd_v = (float)base[(long)SE * ld + 2 * W + lane];
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");     // (the inline-asm requests of the previous head's loop)
    __syncthreads();
    stamp(1);
    const unsigned long long t_p1 = (trace && trace_mode == 2) ? __builtin_amdgcn_s_memtime() : 0ull;

    const FragOffs fo = make_offs(lane);
    // ==== phase 1, FRAGMENTS + ODD KEY: this wave's key tile in registers; D for its query tile; the odd key ===============
    bf16x8 kf[4], vf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) { kf[kk] = frag_rm(Kt, w * 32, fo.rm[kk]); vf[kk] = frag_rm(Vt, w * 32, fo.rm[kk]); }
    // dQ ownership: wave w computes the 16 (d) x 16 (q) block (db, qb) of every query tile's dQ^T over ALL keys, so no
    // partial sums cross waves.  Its A operands K^T[16 d][32 keys] of the NK key tiles stay in registers
    // (v_mfma_f32_16x16x32_bf16: lane <-> d = 16 db + (lane & 15), k = 8 (lane >> 4) + 0..7 <-> key).
    const int db = w >> 1, qb = w & 1, G = lane >> 4, i16 = lane & 15;
    bf16x8 kq[NK];     // (not read_tr_pair(): it changes this kernel's code, see DESIGN.md "source shape")
#pragma unroll
    for (int j = 0; j < NK; ++j)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int row = j * 32 + 8 * G + 4 * r + (i16 >> 2);
            const bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16(
                (__attribute__((address_space(3))) bf16x4*)((lds_char*)Kt + swz_off(row, 2 * db + ((i16 & 3) >> 1)) + (i16 & 1) * 8));
            kq[j][4 * r + 0] = v[0]; kq[j][4 * r + 1] = v[1]; kq[j][4 * r + 2] = v[2]; kq[j][4 * r + 3] = v[3];
        }
    if (trace) { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); stamp(5); }     // K / V / K^T fragments in registers
    {
        f32x16 dke[2] = {zero16(), zero16()}, dve[2] = {zero16(), zero16()};
        {
            const int qe = w;   // query tiles 0..NK-1: one per wave (the odd query, tile NK, takes the vector path below)
            const int q = qe * 32 + l31;
            bf16x8 qf[4], dof[4];
            float dsum = 0.0f;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                qf[kk] = frag_rm(Qt, qe * 32, fo.rm[kk]);
                dof[kk] = frag_rm(Dt, qe * 32, fo.rm[kk]);
                const bf16x8 of = ofr[kk];
#pragma unroll
                for (int e = 0; e < 8; ++e) dsum = fmaf((float)dof[kk][e], (float)of[e], dsum);
            }
            dsum += __shfl_xor(dsum, 32, 64);
            // S^T / dP^T against the last (padded) key tile: lane <-> query, register 0 of the hi = 0 lanes <-> odd key
            f32x16 sT = zero16(), dpT = zero16();
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                sT = MFMA(frag_rm(Kt, SE, fo.rm[kk]), qf[kk], sT);
                dpT = MFMA(frag_rm(Vt, SE, fo.rm[kk]), dof[kk], dpT);
            }
            const float pe = EXP2(fmaf(sT[0], scale_log2, -Ls[q]));
            if (hi == 0) { Ds[q] = dsum; Pe[q] = pe; De[q] = pe * (dpT[0] - dsum); }
            if (trace) stamp(6);                                                       // D, p and dS of the odd key
            // dV, dK of the odd key: B operand with the single column n = 0 (lanes 0 and 32), k <-> the 32 queries
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 pb, db;
#pragma unroll
                for (int half = 0; half < 2; ++half) {     // k index t = 4 half + e <-> query qe*32 + ks*16 + 4 hi + 8 half + e
                    const int q0 = qe * 32 + ks * 16 + 4 * hi + 8 * half;
                    const float4 p4 = *(const float4*)(Pe + q0), d4 = *(const float4*)(De + q0);
                    const float pa[4] = {p4.x, p4.y, p4.z, p4.w}, da[4] = {d4.x, d4.y, d4.z, d4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        pb[4 * half + e] = (bf16_t)(l31 == 0 ? pa[e] : 0.0f);
                        db[4 * half + e] = (bf16_t)(l31 == 0 ? da[e] : 0.0f);
                    }
                }
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    dve[dt] = MFMA(frag_tr(Dt, qe * 32 + ks * 16, fo, dt), pb, dve[dt]);
                    dke[dt] = MFMA(frag_tr(Qt, qe * 32 + ks * 16, fo, dt), db, dke[dt]);
                }
            }
        }
        if (l31 == 0) {   // column 0: rows d = dt*32 + 8*g + 4*hi + 0..3 in registers 4 g .. 4 g + 3
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int d = dt * 32 + 8 * g + 4 * hi;
                    *(float4*)(KVe + (w * 2 + 0) * 64 + d) = make_float4(dke[dt][4 * g], dke[dt][4 * g + 1], dke[dt][4 * g + 2], dke[dt][4 * g + 3]);
                    *(float4*)(KVe + (w * 2 + 1) * 64 + d) = make_float4(dve[dt][4 * g], dve[dt][4 * g + 1], dve[dt][4 * g + 2], dve[dt][4 * g + 3]);
                }
        }
    }
    if (w == ODD_Q_WAVE) {
        // the odd QUERY (row SE) against the odd key, as 64-wide vectors (lane <-> d): D, p, dS, and its dK / dV terms
        const float dov = odd_do, ov = odd_o, qv = odd_q, kv = Ke[lane], vv = odd_v;
        const float dsum = wave_sum(dov * ov), sc = wave_sum(qv * kv), dpe = wave_sum(dov * vv);
        const float pe = EXP2(fmaf(sc, scale_log2, -Ls[SE]));
        const float de = pe * (dpe - dsum);
        if (lane < 32) { Ds[SE + lane] = (lane == 0) ? dsum : 0.0f; Pe[SE + lane] = (lane == 0) ? pe : 0.0f; De[SE + lane] = (lane == 0) ? de : 0.0f; }
        KVe[(NK * 2 + 0) * 64 + lane] = de * qv;
        KVe[(NK * 2 + 1) * 64 + lane] = pe * dov;
    }
    if (trace) stamp(7);                                                               // this wave's part of the phase done
    if (trace && trace_mode == 2 && lane == 0) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        trace[(long)bh * 8 + w] = __builtin_amdgcn_s_memtime() - t_p1;
    }
    __syncthreads();   // K / V tiles are dead: the area becomes the dS tiles + store staging; Ds / Pe / De are complete
    stamp(2);
    // ==== phase 2, TILE LOOP: lockstep walk over the query tiles ============================================================
    // Per tile: S, dP (8 MFMA) -> P, dS in registers -> dS tile to LDS -> ONE barrier -> dV, dK from the registers
    // (8 MFMA) and this wave's dQ^T block from the NK waves' dS tiles (NK v_mfma_f32_16x16x32_bf16) -> dQ stored.
    // The dS tiles are double-buffered by tile parity: a wave that writes tile qt + 1 has passed barrier qt, which
    // every wave reaches only after its reads of tile qt - 1 - one barrier per tile is enough.
    lds_char* dsb = (lds_char*)(smem + Lds::DS);                        // [2][NK] tiles of DS_TILE bytes: [32 keys][32 q] bf16
    // write: this lane's key row (64-B rows), 8-B chunk (4 consecutive q) index XOR ((key >> 1) & 7): the 8 same-parity
    // rows of a 16-lane ds_write_b64 group get 8 different keys, and the two rows r, r + 8 that share a bank phase in
    // the transposing read below differ in key bit 2 = the other 32-B half of the row (round 2 XORed (key >> 2) & 7: 2-way
    // conflicts on every write and every read, 24 extra LDS cycles per query tile and wave in scripts/lds_bank_model.py)
    const int st_w = w * DS_TILE + l31 * 64;
    const int st_sw = (l31 >> DS_KEY_SHIFT) & 7;
    // read (B operand of the 16x16x32 MFMA, lane <-> q = 16 qb + (lane & 15), k <-> key = 8 G + 0..7): transposing read of
    // the 4 (keys) x 16 (q) block; lane i of a 16-lane group addresses key row 8 G + 4 r + (i >> 2), 8-B chunk 4 qb + (i & 3)
    int rd[2];
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        const int row = 8 * G + 4 * r + (i16 >> 2);
        rd[r] = row * 64 + (((4 * qb + (i16 & 3)) ^ ((row >> DS_KEY_SHIFT) & 7)) << 3);
    }
    const float4 ke4 = *(const float4*)(Ke + 16 * db + 4 * G);        // k[odd key][d], d = 16 db + 4 G + 0..3
    bf16_t* dq_out = dqkv + (long)b * lay.qkv_b + (long)h * lay.qkv_h + 16 * db + 4 * G;
    f32x16 dk[2] = {zero16(), zero16()}, dv[2] = {zero16(), zero16()};
    // the next head's tile t of Q / dO into the slot of this head's tile t: legal once every wave has passed the barrier of
    // step t (its fragment reads of the tile are waited for before that barrier).  Issued BEFORE the barrier of step t + 1:
    // the request stalls its wave for a couple of hundred cycles in the texture queue, which the early waves would
    // otherwise spend waiting at that barrier
    auto prefetch_tile = [&](int t) {
        const int blk = 4 * t + (w & 3), row = blk * 8 + (lane >> 3);
        const bf16_t* gp = nsrc + (long)min(row, S - 1) * nld + ((lane & 7) ^ swz_key(row)) * 8;
        const unsigned dst = __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_char*)((w < 4 ? Qt : Dt) + blk * 1024));
        lds_dma16(gp, dst);
    };
    // Two SGPRs held at zero across an empty asm: all that is left of the removed next-head prefetch form (its request masks).
    // Nothing reads them, but without the statement hipcc allocates and schedules the tile loop differently (a kernel nobody
    // has measured; DESIGN.md, "source shape"), so it stays until the next performance change of this loop.
    unsigned pin0 = 0u, pin1 = 0u;
    asm volatile("" : "+s"(pin0), "+s"(pin1));
    for (int qt = 0; qt < NT; ++qt) {
        f32x16 s = zero16(), dp = zero16();
        // Round 5: the tile's 32 lse / D values (8 x 16 B per lane, two distinct addresses per instruction: broadcasts) are
        // requested HERE, in front of the S / dP MFMAs.  hipcc placed each of the eight reads directly in front of its four
        // exp / dS evaluations, followed by its own s_waitcnt lgkmcnt(0): eight exposed LDS round trips (~100+ cycles each
        // with eight waves on the LDS) in the middle of the softmax arithmetic of every tile and wave - a third of the
        // 3.0 k cycles a tile took?  Measured (profiles/r05_attn_ab_bwd_variants_fwd_persistent.log, same box, three
        // alternations): tile loop 27.3 k -> 25.5 k cycles per head (-6 %), kernel 199-203 -> 191-199 us.  The sched_barrier pins
        // them; the MFMA phase (>= 256 cycles) covers their latency, and the 32 registers are free at this point of the step
        // (dO^T / Q^T / dS fragments are not live yet).  Also requesting the step's eight row-major Q / dO fragments in one batch
        // behind them measured no better (196-201 us): removed.
        float4 lq4[4], dq4[4];
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            lq4[g] = *(const float4*)(Ls + qt * 32 + 8 * g + 4 * hi);
            dq4[g] = *(const float4*)(Ds + qt * 32 + 8 * g + 4 * hi);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
            s = MFMA(frag_rm(Qt, qt * 32, fo.rm[kk]), kf[kk], s);      // S[q][key]: lane <-> key, regs <-> q
            dp = MFMA(frag_rm(Dt, qt * 32, fo.rm[kk]), vf[kk], dp);    // dP[q][key]
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const float4 lq = lq4[g], dq = dq4[g];
            const float lqa[4] = {lq.x, lq.y, lq.z, lq.w};
            const float dqa[4] = {dq.x, dq.y, dq.z, dq.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float pv = EXP2(fmaf(s[g * 4 + e], scale_log2, -lqa[e]));
                s[g * 4 + e] = pv;                                  // P   (in place)
                dp[g * 4 + e] = pv * (dp[g * 4 + e] - dqa[e]);      // dS  (in place)
            }
        }
        lds_char* buf = dsb + (qt & 1) * (NK * DS_TILE);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            bf16x4 v4;
#pragma unroll
            for (int e = 0; e < 4; ++e) v4[e] = (bf16_t)dp[g * 4 + e];
            *(__attribute__((address_space(3))) bf16x4*)(buf + st_w + (((2 * g + hi) ^ st_sw) << 3)) = v4;
        }
        // operands of dV / dK (dO^T, Q^T of this query tile): independent of the other waves.  (Requesting them ahead of
        // the softmax arithmetic measured 1 % slower: 256 VGPRs and a spill.)
        bf16x8 dot[2][2], qtr[2][2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                dot[ks][dt] = frag_tr(Dt, qt * 32 + ks * 16, fo, dt);
                qtr[ks][dt] = frag_tr(Qt, qt * 32 + ks * 16, fo, dt);
            }
        if (prefetch_next && qt > 0) prefetch_tile(qt - 1);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");          // the dS tile is in LDS
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        bf16x8 dsq[NK];
#pragma unroll
        for (int j = 0; j < NK; ++j) dsq[j] = read_tr_pair(buf + j * DS_TILE, rd[0], rd[1]);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            const bf16x8 pb = pack_b(s, ks), dbv = pack_b(dp, ks);
#pragma unroll
            for (int dt = 0; dt < 2; ++dt) {
                dv[dt] = MFMA(dot[ks][dt], pb, dv[dt]);
                dk[dt] = MFMA(qtr[ks][dt], dbv, dk[dt]);
            }
        }
        f32x4 dq0 = {0.0f, 0.0f, 0.0f, 0.0f}, dq1 = {0.0f, 0.0f, 0.0f, 0.0f};   // dQ^T block: lane <-> q, regs <-> d
#pragma unroll
        for (int j = 0; j < NK; j += 2) {
            dq0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kq[j], dsq[j], dq0, 0, 0, 0);
            dq1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kq[j + 1], dsq[j + 1], dq1, 0, 0, 0);
        }
        {
            const int q = qt * 32 + 16 * qb + i16;
            const float de = De[q];                                 // dS[q][odd key]: its rank-1 term dS * k joins here
            if (q < S) {
                bf16x4 ov;
                ov[0] = (bf16_t)(fmaf(de, ke4.x, dq0[0] + dq1[0]) * scale); ov[1] = (bf16_t)(fmaf(de, ke4.y, dq0[1] + dq1[1]) * scale);
                ov[2] = (bf16_t)(fmaf(de, ke4.z, dq0[2] + dq1[2]) * scale); ov[3] = (bf16_t)(fmaf(de, ke4.w, dq0[3] + dq1[3]) * scale);
                *(bf16x4*)(dq_out + (long)q * lddq) = ov;
            }
        }
    }

    if (prefetch_next) prefetch_tile(NT - 1);
    stamp(3);
    // ==== phase 3, STORES: dK, dV of this wave's keys; the odd key ==========================================================
    // Through a wave-private 4 KiB LDS tile ([32 keys][64 d] bf16, 16-B chunk index XOR (key & 7)), so that the global
    // stores are 16 B per lane and 8 whole 128-B rows per instruction instead of row-per-lane 8-byte stores (4 + 4
    // dwordx4 stores instead of 16 + 16 dwordx2; the store tail was 10 % of the kernel, issue-bound).  The tile lives
    // behind the dS buffers, which slower waves may still be reading.
    {
        lds_char* tile = (lds_char*)(smem + Lds::STAGE) + w * Lds::STAGE_TILE;
        const int r8 = lane >> 3, c8 = lane & 7;
        bf16_t* kbase = dqkv + (long)b * lay.qkv_b + (long)h * lay.qkv_h + (long)(w * 32) * lddq + W + c8 * 8;
#pragma unroll
        for (int which = 0; which < 2; ++which) {
#pragma unroll
            for (int dt = 0; dt < 2; ++dt)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    bf16x4 ov;
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        ov[e] = which == 0 ? (bf16_t)(dk[dt][g * 4 + e] * scale) : (bf16_t)dv[dt][g * 4 + e];
                    *(__attribute__((address_space(3))) bf16x4*)(tile + l31 * 128 + (((dt * 4 + g) ^ (l31 & 7)) << 4) + hi * 8) = ov;
                }
            bf16x8 t[4];
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int row = it * 8 + r8;
                t[it] = *(const __attribute__((address_space(3))) bf16x8*)(tile + row * 128 + ((c8 ^ (row & 7)) << 4));
            }
#pragma unroll
            for (int it = 0; it < 4; ++it)
                *(bf16x8*)(kbase + (long)(it * 8 + r8) * lddq + which * W) = t[it];
        }
    }
    if (w == 0) {
        float ak = 0.0f, av = 0.0f;
#pragma unroll
        for (int ww = 0; ww <= NK; ++ww) { ak += KVe[(ww * 2 + 0) * 64 + lane]; av += KVe[(ww * 2 + 1) * 64 + lane]; }
        bf16_t* krow = dqkv + (long)b * lay.qkv_b + (long)h * lay.qkv_h + (long)SE * lddq + W;
        krow[lane] = (bf16_t)(ak * scale);
        krow[W + lane] = (bf16_t)av;
    }
    stamp(4);
    have_qd = prefetch_next;
    __syncthreads();   // the next head's staging overwrites the K / V area (dS tiles, store transposes) and the small arrays
    }
}


// ---------------------------------------------------------------------------------------------
int attn_fwd_odd_launch(const bf16_t* qkv, long ldqkv, bf16_t* o, long ldo, float* lse, int B, int H, hipStream_t s) {
    constexpr int NK = ATTN_ODD_NK;
    constexpr size_t lds = FwdOddLds<NK>::TOTAL;
    if (int rc = set_lds(attn_fwd_odd_kernel<NK>, lds)) return rc;
    hipLaunchKernelGGL((attn_fwd_odd_kernel<NK>), dim3(B * H), dim3(NK * 64), lds, s, qkv, ldqkv, o, ldo, lse, H, (long)H * 64,
                       0.125f * 1.4426950408889634f, attn_token_major(ATTN_ODD_S, ldqkv, ldo));
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

int attn_bwd_fused_launch(const bf16_t* qkv, long ldqkv, const bf16_t* o, long ldo, const bf16_t* d_o, long lddo,
                          const float* lse, float* dsum_scratch, bf16_t* dqkv, long lddqkv, int B, int H, hipStream_t s) {
    constexpr int NK = ATTN_ODD_NK;
    constexpr size_t lds = BwdFusedLds<NK>::TOTAL;
    if (int rc = set_lds(attn_bwd_fused_kernel<NK>, lds)) return rc;
    const AttnEnv& env = attn_env();
    const int nbh = B * H, grid = env.persist ? std::min(nbh, 256) : nbh;
    unsigned long long* tr = env.trace ? (unsigned long long*)dsum_scratch : nullptr;
    hipLaunchKernelGGL((attn_bwd_fused_kernel<NK>), dim3(grid), dim3(NK * 64), lds, s, qkv, ldqkv, o, ldo, d_o, lddo, lse, dqkv,
                       lddqkv, H, ATTN_ODD_S, (long)H * 64, 0.125f, 0.125f * 1.4426950408889634f, tr, env.desync | (env.trace << 8),
                       attn_token_major(ATTN_ODD_S, ldqkv, ldo), nbh);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

}  // namespace rvlm
