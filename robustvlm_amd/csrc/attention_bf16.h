// bf16 flash attention on gfx950 (head_dim = 64, no mask, no dropout): what the kernel files share.
//   attention_bf16.hip      any S: forward, prep, dQ, dK/dV; the dispatchers attn_fwd_bf16 / attn_bwd_bf16
//   attention_bf16_odd.hip  S = 32 NK + 1 (257): the forward and the fused backward that the headline runs
//   attention_cls.hip       class-token attention of the last block (shares nothing with the rest)
//
// One workgroup per (image, head).  A whole head's K and V (S x 64 bf16 = 32 KiB each at S = 257)
// are LDS-resident, so there is no K/V streaming loop over HBM: every wave owns 32-row tiles and
// walks the LDS-resident operand in 32-row tiles, v_mfma_f32_32x32x16_bf16 throughout.
//
// Layout tricks
//  * LDS tiles are [rows][64] bf16 (128-B rows), 16-B chunk index XOR swz_key(row) (a permutation of row bits 1-3):
//    ds_read_b128 fragment reads AND the ds_read_b64_tr_b16 transposing reads are bank-conflict free.
//  * "Swapped" products: S^T = K.Q^T puts one query per lane (lane&31), so softmax row statistics are
//    per-lane scalars and P^T / dS^T are already in the B-operand register layout of the next MFMA
//    (the k index is permuted identically on both operands, so no cross-lane exchange is needed).
//  * The operand that needs a transpose (V^T in fwd, K^T / Q^T / dO^T in bwd) comes from the same
//    row-major LDS tile through ds_read_b64_tr_b16 (hardware transpose read, 4 rows x 16 cols per
//    16-lane group).  USE_TR=false builds the same fragment with scalar LDS reads (validation).
#pragma once
#include "kernels.h"

namespace rvlm {
// element strides of the (image, head) blocks.  The library builds the token-major form only ([B][S][3W]: b = S*ld, h = 64);
// it stays a kernel argument because taking it out changes the S = 32 NK + 1 kernels' code.
struct AttnLayout { long qkv_b, qkv_h, o_b, o_h; };
static inline AttnLayout attn_token_major(int S, long ldqkv, long ldo) { return {(long)S * ldqkv, 64L, (long)S * ldo, 64L}; }

// ---- host side ------------------------------------------------------------------------------------------------
constexpr size_t ATTN_LDS_MAX = 160 * 1024;
constexpr size_t ATTN_TILE_ROW = 128;                       // bytes of one row of a [rows][64] bf16 LDS tile
constexpr int ATTN_ODD_NK = 8, ATTN_ODD_S = 32 * ATTN_ODD_NK + 1;   // the sequence length attention_bf16_odd.hip is built for

// the RVLM_ATTN_* switches, read once on first use
struct AttnEnv {
    int occ;        // RVLM_ATTN_OCC      5: the generic forward capped at 96 VGPRs where two workgroups fit a CU
    int fwd_odd;    // RVLM_ATTN_FWD_ODD  0: generic padded-tile forward at S = 257
    int fused;      // RVLM_ATTN_FUSED    0: generic two-kernel backward at S = 257
    int persist;    // RVLM_ATTN_PERSIST  0: one workgroup per (image, head) in the fused backward
    int trace;      // RVLM_ATTN_TRACE    1: phase stamps of the fused backward into the dsum scratch, 2: per-wave phase-1 times
    int desync;     // RVLM_ATTN_DESYNC   phase offset between the fused backward's workgroups (see the kernel)
};
const AttnEnv& attn_env();

// opt in to `bytes` of dynamic LDS; fails before anything is enqueued
template <typename K>
static int set_lds(K kernel, size_t bytes) {
    if (bytes > ATTN_LDS_MAX) return fail(RVLM_ERR_UNSUPPORTED, "attention: sequence too long for LDS-resident K/V");
    hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return fail(RVLM_ERR_HIP, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
    return RVLM_OK;
}

// attention_bf16_odd.hip, S = ATTN_ODD_S (called from the dispatchers)
int attn_fwd_odd_launch(const bf16_t* qkv, long ldqkv, bf16_t* o, long ldo, float* lse, int B, int H, hipStream_t s);
int attn_bwd_fused_launch(const bf16_t* qkv, long ldqkv, const bf16_t* o, long ldo, const bf16_t* d_o, long lddo,
                          const float* lse, float* dsum_scratch, bf16_t* dqkv, long lddqkv, int B, int H, hipStream_t s);

// ---- device side ----------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) char lds_char;

// Swizzle key of a tile row: row bits (1, 3, 2) -> chunk bits (2, 1, 0).  Any bijection of those three row bits keeps the
// row-major ds_read_b128 fragments conflict-free (the 8 same-parity rows of a 16-lane group get 8 different keys); the
// TRANSPOSING reads (ds_read_b64_tr_b16: a 32-lane half reads 4 consecutive rows x one 64-B half row) additionally need
// rows r and r + 2 - same bank parity - to land in DIFFERENT 64-B halves, i.e. row bit 1 on chunk bit 2.  Round 2 used
// (row >> 1) & 7: every transposing read was a 2-way bank conflict (scripts/lds_bank_model.py: 16 of 40 extra LDS cycles
// per query tile and wave; PMC: 32.5 % of the backward's LDS-active cycles in conflicts, profiles/r02_pmc_attention.json).
__device__ __forceinline__ int swz_key(int row) {
    return (((row >> 1) & 1) << 2) | (((row >> 3) & 1) << 1) | ((row >> 2) & 1);
}
__device__ __forceinline__ int swz_off(int row, int chunk) {  // byte offset inside a [rows][64] bf16 tile
    return row * 128 + ((chunk ^ swz_key(row)) << 4);
}

// cooperative stage of rows [0,Sp) x 64 bf16 from global (row stride ld elements) into a swizzled tile
// by LDS-DMA (global_load_lds_dwordx4: 8 rows = 1 KiB per wave instruction, asynchronous, no VGPR
// round trip).  The DMA writes LDS lane-linearly, so the swizzle goes on the per-lane source address.
// Rows >= S replicate row S-1 (finite data); every consumer masks them (scores -> -inf / p = 0).
__device__ __forceinline__ void stage_tile(char* tile, const bf16_t* src, long ld, int S, int Sp,
                                           int w, int nw, int lane) {
    for (int blk = w; blk < (Sp >> 3); blk += nw) {
        const int row = blk * 8 + (lane >> 3);
        const int lc = (lane & 7) ^ swz_key(row);
        const int rs = min(row, S - 1);
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void*)(src + (long)rs * ld + lc * 8),
            (__attribute__((address_space(3))) void*)(tile + blk * 1024), 16, 0, 0);
    }
}

// One LDS-DMA request of 16 bytes per lane (1 KiB per wave) to the LDS byte address dst (wave-uniform), as inline asm: a
// compiler-visible request (stage_tile) makes hipcc drain vmcnt in front of every later LDS read that might alias it, which a
// kernel that requests the NEXT head's tiles under its own tile loop cannot afford.  The caller waits (s_waitcnt vmcnt) itself.
__device__ __forceinline__ void lds_dma16(const void* gp, unsigned dst) {
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" :: "v"(gp), "s"(dst) : "memory", "m0");
}

// A/B operand fragment with k along the 64-wide (contiguous) dim, straight from global: row, k-chunk kk
__device__ __forceinline__ bf16x8 frag_global(const bf16_t* src, long ld, int row, int kk, int lane) {
    return *(const bf16x8*)(src + (long)row * ld + (kk * 2 + (lane >> 5)) * 8);
}

// two transposing reads (ds_read_b64_tr_b16: 4 rows x 16 columns per 16-lane group each) at base + off0 / off1 = the 8 k-values
// of one MFMA operand
__device__ __forceinline__ bf16x8 read_tr_pair(const lds_char* base, int off0, int off1) {
    bf16x8 out;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
        bf16x4 v = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((__attribute__((address_space(3))) bf16x4*)(base + (r ? off1 : off0)));
        out[4 * r + 0] = v[0]; out[4 * r + 1] = v[1]; out[4 * r + 2] = v[2]; out[4 * r + 3] = v[3];
    }
    return out;
}

// Per-lane byte offsets that do not depend on the tile index (32-row tiles start at multiples of 16
// rows, which leaves the swz_key(row) swizzle term unchanged): address = tile + row0*128 + offset.
struct FragOffs {
    int rm[4];      // row-major fragment, k-chunk kk:      row0 = first row of the 32-row tile
    int tr[2][2];   // transposed fragment [dt][r]:          row0 = first row of the 16-row k-slice
};
__device__ __forceinline__ FragOffs make_offs(int lane) {
    FragOffs o;
    const int l31 = lane & 31, hi = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) o.rm[kk] = swz_off(l31, kk * 2 + hi);
    const int i = lane & 15, dblk = (lane >> 4) & 1;
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
            const int x = 4 * hi + 8 * r + (i >> 2);
            o.tr[dt][r] = swz_off(x, dt * 4 + dblk * 2 + ((i & 3) >> 1)) + (i & 1) * 8;
        }
    return o;
}
// row-major fragment: MFMA row = row0 + lane&31, k-chunk of offset `off` (FragOffs::rm)
__device__ __forceinline__ bf16x8 frag_rm(const char* tile, int row0, int off) {
    return *(const bf16x8*)(tile + row0 * 128 + off);
}
// Transposed fragment X^T: MFMA row index = column (dt*32 + lane&31) of the LDS tile, k index t'
// (0..7) <-> tile row  row0 + 4*hi + (t'&3) + 8*(t'>>2)   (the permutation pack_b() uses).
__device__ __forceinline__ bf16x8 frag_tr(const char* tile, int row0, const FragOffs& o, int dt) {
    return read_tr_pair((lds_char*)tile + row0 * 128, o.tr[dt][0], o.tr[dt][1]);
}
template <bool USE_TR>
__device__ __forceinline__ bf16x8 frag_t(const char* tile, int row0, const FragOffs& o, int dt, int lane) {
    if (USE_TR) return frag_tr(tile, row0, o, dt);
    bf16x8 out;     // the same fragment by scalar LDS reads
    const int col = dt * 32 + (lane & 31), hi = lane >> 5;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const int row = row0 + 4 * hi + (t & 3) + 8 * (t >> 2);
        out[t] = *(const bf16_t*)(tile + swz_off(row, col >> 3) + (col & 7) * 2);
    }
    return out;
}

// accumulator (D layout: row = (reg&3)+8*(reg>>2)+4*hi) -> B operand for k-slice ks (16 rows)
__device__ __forceinline__ bf16x8 pack_b(const f32x16& p, int ks) {
    bf16x8 o;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        o[t] = (bf16_t)p[(2 * ks) * 4 + t];
        o[4 + t] = (bf16_t)p[(2 * ks + 1) * 4 + t];
    }
    return o;
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int e = 0; e < 16; ++e) z[e] = 0.0f;
    return z;
}

// the four values (dt, g) of a 32 x 64 accumulator pair, times f, as bf16: the lane's d = dt*32 + 8*g + 4*hi + 0..3 of its row
__device__ __forceinline__ bf16x4 acc_bf16x4(const f32x16 (&acc)[2], int dt, int g, float f) {
    bf16x4 v;
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = (bf16_t)(acc[dt][g * 4 + e] * f);
    return v;
}
// row-store epilogue of the generic kernels: the lane's row of acc * f as eight 8-byte stores (row -> its 64 head dims)
__device__ __forceinline__ void store_row(bf16_t* row, const f32x16 (&acc)[2], float f, int hi) {
#pragma unroll
    for (int dt = 0; dt < 2; ++dt)
#pragma unroll
        for (int g = 0; g < 4; ++g) *(bf16x4*)(row + dt * 32 + 8 * g + 4 * hi) = acc_bf16x4(acc, dt, g, f);
}

#define MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0)
// raw v_exp_f32 (2^x): arguments here are <= ~6 and results below 2^-126 may flush to 0, which is what
// softmax wants; exp2f() would wrap every call in denormal-range fix-ups (~6 VALU instead of 1)
#define EXP2(x) __builtin_amdgcn_exp2f(x)

}  // namespace rvlm
