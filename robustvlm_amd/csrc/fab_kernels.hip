// FAB / FAB-T, L-inf (autoattack/fab_base.py, fab_projections.py:7-58): the device arithmetic of one iteration.
//
// projection_linf, restated.  For a point t in [0,1]^D, a hyperplane w.z = b and c = b - w.t: the perturbation d with the
// smallest max_i |d_i| such that w.(t + d) = b and t + d stays in the box moves every coordinate with w_i != 0 in the
// direction dir_i = sign(c) sign(w_i) by the SAME amount lambda, except where the box face is nearer:
//     d_i = dir_i min(lambda, room_i),   room_i = distance from t_i to the face in direction dir_i (0 where w_i = 0),
//     f(lambda) := sum_i |w_i| min(lambda, room_i) = |c|.
// f is non-decreasing, piecewise linear and concave; if f(max_i room_i) < |c| the hyperplane misses the box and every moving
// coordinate goes to its face.  The reference finds the segment of f with an argsort of room and cumulative sums; here the
// solution is located WITHOUT a sort, by a 16-ary search over the BIT PATTERN of lambda (non-negative floats order like their
// bits): one pass over the row evaluates f at 15 thresholds between the current bounds, the bracket shrinks 16-fold, and
// FAB_PASSES = 8 passes cover all 2^32 patterns - the result is the smallest fp32 lambda with f(lambda) >= |c|, i.e. the exact
// solution rounded up by less than one ulp.  Every term |w_i| min(thr, room_i) and every fixed-order fp32 sum of them is
// monotone in thr, so the search is consistent in floating point as well.
//
// Mapping: ONE workgroup of 1024 threads owns one row - in the fused step one IMAGE, i.e. the two points x1 and x0 that
// share w and b (fab_base.py:189-197 projects both), so w is read once per pass for the pair.  A row's inputs (w, x1, x0 at
// D = 150 528: 1.8 MB) are walked 10 times by the same workgroup: the first walk comes from HBM, the others from the L2 of
// the XCD the workgroup sits on / the Infinity Cache.  No cross-workgroup combine, no atomics: every sum is lane-strided
// partials, wave shuffles, 16 wave partials in LDS in a fixed order - bit-reproducible run to run.
// Every loop has a compile-time or D-derived trip count; NaN / Inf in w, t or b falls through the same passes, raises
// RVLM_FLAG_FAB_NONFINITE and gives that row lambda = 0 (d = 0).
#include "kernels.h"

namespace rvlm {

constexpr int FAB_THREADS = 1024;
constexpr int FAB_WAVES = FAB_THREADS / 64;
constexpr int FAB_J = 15;        // thresholds per pass (16-ary search)
constexpr int FAB_PASSES = 8;    // 16^8 = 2^32 >= every non-negative float bit pattern

// Four consecutive elements of a row.  vec: the row is 16-byte aligned (D % 4 == 0) -> one 16-byte load; otherwise scalar
// loads with the tail padded by `fill` (w is padded with 0: such an element contributes to no sum and never moves).
__device__ __forceinline__ f32x4 fab_load4(const float* __restrict__ row, int u, int D, bool vec, float fill) {
    if (vec) return *reinterpret_cast<const f32x4*>(row + 4 * (size_t)u);
    f32x4 v;
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = (4 * u + k < D) ? row[4 * (size_t)u + k] : fill;
    return v;
}
__device__ __forceinline__ void fab_store4(float* __restrict__ row, int u, int D, bool vec, f32x4 v) {
    if (vec) { *reinterpret_cast<f32x4*>(row + 4 * (size_t)u) = v; return; }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (4 * u + k < D) row[4 * (size_t)u + k] = v[k];
}
__device__ __forceinline__ bool fab_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

// deterministic block sums of N values: wave shuffles, then the 16 wave partials in wave order.  red: FAB_WAVES * N + N floats
template <int N>
__device__ __forceinline__ void fab_block_sum(float (&v)[N], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = wave_sum(v[j]);
    __syncthreads();                                   // red may still be read from the previous reduction
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) red[wave * N + j] = v[j];
    }
    __syncthreads();
    if (threadIdx.x < N) {
        float s = 0.0f;
#pragma unroll
        for (int w = 0; w < FAB_WAVES; ++w) s += red[w * N + threadIdx.x];
        red[FAB_WAVES * N + threadIdx.x] = s;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = red[FAB_WAVES * N + j];
}
template <int N>
__device__ __forceinline__ void fab_block_max(float (&v)[N], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < N; ++j) v[j] = wave_max(v[j]);
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < N; ++j) red[wave * N + j] = v[j];
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < N; ++j) {
        float m = red[j];
#pragma unroll
        for (int w = 1; w < FAB_WAVES; ++w) m = fmaxf(m, red[w * N + j]);
        v[j] = m;
    }
}

// room of one coordinate: up = the coordinate moves towards 1 (c > 0 and w > 0, or c <= 0 and w < 0; the reference's
// sign flip, fab_projections.py:11-13, counts c = 0 as negative)
__device__ __forceinline__ float fab_room(float w, float t, bool cpos) {
    const bool up = cpos ? (w > 0.0f) : (w < 0.0f);
    const float r = (w == 0.0f) ? 0.0f : (up ? 1.0f - t : t);
    return fmaxf(r, 0.0f);
}
__device__ __forceinline__ float fab_dir(float w, bool cpos) {
    const float s = (w > 0.0f ? 1.0f : 0.0f) - (w < 0.0f ? 1.0f : 0.0f);
    return cpos ? s : -s;
}

// The search for NP points t[p] that share the normal w: returns lambda[p] (already min'ed with the largest room: the row
// maximum of |d|) and whether the row held a NaN / Inf.  c = b - w.t is formed here from b (standalone) or from df (fused:
// b = -df + w.x1, fab_base.py:186-187).
template <int NP>
__device__ __forceinline__ void fab_solve(const float* __restrict__ w, const float* const (&t)[NP], int D, bool vec, bool fused,
                                          float b_or_df, float* red, float (&lam)[NP], bool (&cpos)[NP], bool& bad) {
    const int units = (D + 3) >> 2;
    // ---- walk 0: w.t per point (and the non-finite check) ----
    float acc0[NP + 1];
#pragma unroll
    for (int p = 0; p <= NP; ++p) acc0[p] = 0.0f;
    for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
        const f32x4 wv = fab_load4(w, u, D, vec, 0.0f);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const f32x4 tv = fab_load4(t[p], u, D, vec, 0.0f);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                acc0[p] = fmaf(wv[k], tv[k], acc0[p]);
                if (!fab_finite(tv[k])) acc0[NP] = 1.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (!fab_finite(wv[k])) acc0[NP] = 1.0f;
    }
    fab_block_sum<NP + 1>(acc0, red);
    float c[NP];
    const float b = fused ? (-b_or_df + acc0[0]) : b_or_df;        // fused: b = -df + (dg * x1).sum()
    bad = acc0[NP] != 0.0f || !fab_finite(b_or_df);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const float cs = b - acc0[p];
        bad = bad || !fab_finite(cs);
        cpos[p] = cs > 0.0f;
        c[p] = fabsf(cs);
    }
    // ---- walks 1 .. FAB_PASSES: 16-ary search over the bit pattern of lambda ----
    unsigned lo[NP], hi[NP];
    float rmax[NP];
#pragma unroll
    for (int p = 0; p < NP; ++p) { lo[p] = 0u; hi[p] = 0x7f7fffffu; rmax[p] = 0.0f; }
#pragma unroll 1
    for (int pass = 0; pass < FAB_PASSES; ++pass) {
        unsigned key[NP * FAB_J];                      // wave-uniform: the thresholds of this pass, lo < key <= hi
        float f[NP * FAB_J];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const unsigned l = __builtin_amdgcn_readfirstlane(lo[p]), h = __builtin_amdgcn_readfirstlane(hi[p]);
            unsigned s = (h - l + 15u) >> 4;
            s = s < 1u ? 1u : s;
#pragma unroll
            for (int j = 0; j < FAB_J; ++j) {
                const unsigned q = l + (unsigned)(j + 1) * s;
                key[p * FAB_J + j] = q < h ? q : h;
            }
        }
#pragma unroll
        for (int j = 0; j < NP * FAB_J; ++j) f[j] = 0.0f;
        for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
            const f32x4 wv = fab_load4(w, u, D, vec, 0.0f);
#pragma unroll
            for (int p = 0; p < NP; ++p) {
                const f32x4 tv = fab_load4(t[p], u, D, vec, 0.0f);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float aw = fabsf(wv[k]);
                    const float room = fab_room(wv[k], tv[k], cpos[p]);
                    if (pass == 0) rmax[p] = fmaxf(rmax[p], room);
#pragma unroll
                    for (int j = 0; j < FAB_J; ++j)
                        f[p * FAB_J + j] = fmaf(aw, fminf(__uint_as_float(key[p * FAB_J + j]), room), f[p * FAB_J + j]);
                }
            }
        }
        fab_block_sum<NP * FAB_J>(f, red);
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            unsigned nlo = lo[p], nhi = hi[p];
            bool below = true;                         // f is monotone: once a threshold reaches |c| the later ones do too
#pragma unroll
            for (int j = 0; j < FAB_J; ++j) {
                below = below && (f[p * FAB_J + j] < c[p]);
                if (below) nlo = key[p * FAB_J + j];
                else if (key[p * FAB_J + j] < nhi) nhi = key[p * FAB_J + j];
            }
            lo[p] = nlo < nhi ? nlo : nhi;
            hi[p] = nhi;
        }
    }
    fab_block_max<NP>(rmax, red);
#pragma unroll
    for (int p = 0; p < NP; ++p) {
        const float l = fminf(__uint_as_float(hi[p]), rmax[p]);     // hyperplane misses the box: hi stays at the top -> faces
        lam[p] = (c[p] > 0.0f && !bad) ? l : 0.0f;
    }
}

// standalone projection (the kernel tests' entry): d[r] = projection_linf(t[r], w[r], b[r])
__global__ void __launch_bounds__(FAB_THREADS)
fab_projection_linf_kernel(const float* __restrict__ t, const float* __restrict__ w, const float* __restrict__ b, int D,
                           float* __restrict__ d, float* __restrict__ lambda_out, int32_t* __restrict__ flags) {
    __shared__ float red[(FAB_WAVES + 1) * FAB_J];
    const size_t base = (size_t)blockIdx.x * D;
    const bool vec = (D & 3) == 0;
    const float* const tp[1] = {t + base};
    float lam[1];
    bool cpos[1], bad;
    fab_solve<1>(w + base, tp, D, vec, false, b[blockIdx.x], red, lam, cpos, bad);
    if (threadIdx.x == 0) {
        if (lambda_out) lambda_out[blockIdx.x] = lam[0];
        if (bad && flags) atomicOr(flags, RVLM_FLAG_FAB_NONFINITE);
    }
    const int units = (D + 3) >> 2;
    for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
        const f32x4 wv = fab_load4(w + base, u, D, vec, 0.0f);
        const f32x4 tv = fab_load4(t + base, u, D, vec, 0.0f);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) o[k] = fab_dir(wv[k], cpos[0]) * fminf(lam[0], fab_room(wv[k], tv[k], cpos[0]));
        fab_store4(d + base, u, D, vec, o);
    }
}

// fused FAB step of one image (fab_base.py:186-226): b = -df + dg.x1, the projections of x1 and x0 onto dg.z = b, the
// convex combination and the clamp; d1 / d0 are recomputed from lambda on the fly and never stored
__global__ void __launch_bounds__(FAB_THREADS)
fab_linf_step_kernel(float* __restrict__ x1, const float* __restrict__ x0, const float* __restrict__ dg,
                     const float* __restrict__ df, int D, float alpha_max, float eta, float* __restrict__ lambda_out,
                     int32_t* __restrict__ flags) {
    __shared__ float red[(FAB_WAVES + 1) * 2 * FAB_J];
    const size_t base = (size_t)blockIdx.x * D;
    const bool vec = (D & 3) == 0;
    const float* const tp[2] = {x1 + base, x0 + base};
    float lam[2];
    bool cpos[2], bad;
    fab_solve<2>(dg + base, tp, D, vec, true, df[blockIdx.x], red, lam, cpos, bad);
    if (threadIdx.x == 0) {
        if (lambda_out) { lambda_out[2 * blockIdx.x] = lam[0]; lambda_out[2 * blockIdx.x + 1] = lam[1]; }
        if (bad && flags) atomicOr(flags, RVLM_FLAG_FAB_NONFINITE);
    }
    // the row maximum of |d| is lambda (fab_base.py:209-212); alpha of :217-222
    const float a1 = fmaxf(lam[0], 1e-8f), a0 = fmaxf(lam[1], 1e-8f);
    const float alpha = fminf(fmaxf(a1 / (a1 + a0), 0.0f), alpha_max);
    const int units = (D + 3) >> 2;
    for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
        const f32x4 wv = fab_load4(dg + base, u, D, vec, 0.0f);
        const f32x4 p1 = fab_load4(x1 + base, u, D, vec, 0.0f);
        const f32x4 p0 = fab_load4(x0 + base, u, D, vec, 0.0f);
        f32x4 o;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float d1 = fab_dir(wv[k], cpos[0]) * fminf(lam[0], fab_room(wv[k], p1[k], cpos[0]));
            const float d0 = fab_dir(wv[k], cpos[1]) * fminf(lam[1], fab_room(wv[k], p0[k], cpos[1]));
            const float v = (p1[k] + eta * d1) * (1.0f - alpha) + (p0[k] + d0 * eta) * alpha;      // :223-224
            o[k] = fminf(fmaxf(v, 0.0f), 1.0f);
        }
        fab_store4(x1 + base, u, D, vec, o);
    }
}

// bookkeeping after the prediction forward (fab_base.py:228-252), one workgroup per image: for a misclassified x1,
// t = max|x1 - x0|; t < res2 -> adv = x1, res2 = t; then the backward step x1 = x0 + (x1 - x0) * beta
__global__ void __launch_bounds__(FAB_THREADS)
fab_track_best_kernel(float* __restrict__ x1, const float* __restrict__ x0, float* __restrict__ adv, float* __restrict__ res2,
                      const uint8_t* __restrict__ pred_eq, float beta, int D) {
    __shared__ float red[FAB_WAVES];
    if (pred_eq[blockIdx.x]) return;                   // still classified correctly (uniform per workgroup)
    const size_t base = (size_t)blockIdx.x * D;
    const bool vec = (D & 3) == 0;
    const int units = (D + 3) >> 2;
    float m[1] = {0.0f};
    for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
        const f32x4 a = fab_load4(x1 + base, u, D, vec, 0.0f), o = fab_load4(x0 + base, u, D, vec, 0.0f);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[0] = fmaxf(m[0], fabsf(a[k] - o[k]));
    }
    fab_block_max<1>(m, red);
    const float old = res2[blockIdx.x];
    const bool better = m[0] < old;
    __syncthreads();                                   // every thread has read res2 before thread 0 replaces it
    if (better && threadIdx.x == 0) res2[blockIdx.x] = m[0];
    for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
        const f32x4 a = fab_load4(x1 + base, u, D, vec, 0.0f), o = fab_load4(x0 + base, u, D, vec, 0.0f);
        if (better) fab_store4(adv + base, u, D, vec, a);
        f32x4 n;
#pragma unroll
        for (int k = 0; k < 4; ++k) n[k] = o[k] + (a[k] - o[k]) * beta;
        fab_store4(x1 + base, u, D, vec, n);
    }
}

// untargeted FAB, one class k of the streamed Jacobian (fab_pt.py:76-98 + fab_base.py:166-184): w = dg_k - dg_y,
// dist = |df_k| / (1e-12 + |w|_1); kept when strictly smaller than the best so far (first minimum wins, like min(dim=1)[1])
__global__ void __launch_bounds__(FAB_THREADS)
fab_jacobian_argmin_kernel(const float* __restrict__ g_k, const float* __restrict__ g_y, const float* __restrict__ df_k,
                           const int64_t* __restrict__ y, int k, int D, float* __restrict__ best_dist,
                           float* __restrict__ best_df, float* __restrict__ best_w) {
    __shared__ float red[FAB_WAVES + 1];
    if (y[blockIdx.x] == (int64_t)k) return;           // the reference masks the true class with df = 1e10
    const size_t base = (size_t)blockIdx.x * D;
    const bool vec = (D & 3) == 0;
    const int units = (D + 3) >> 2;
    float s[1] = {0.0f};
    for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
        const f32x4 a = fab_load4(g_k + base, u, D, vec, 0.0f), o = fab_load4(g_y + base, u, D, vec, 0.0f);
#pragma unroll
        for (int q = 0; q < 4; ++q) s[0] += fabsf(a[q] - o[q]);
    }
    fab_block_sum<1>(s, red);
    const float dist = fabsf(df_k[blockIdx.x]) / (1e-12f + s[0]);
    const bool take = dist < best_dist[blockIdx.x];
    __syncthreads();                                   // every thread has read best_dist before thread 0 replaces it
    if (!take) return;
    if (threadIdx.x == 0) { best_dist[blockIdx.x] = dist; best_df[blockIdx.x] = df_k[blockIdx.x]; }
    for (int u = threadIdx.x; u < units; u += FAB_THREADS) {
        const f32x4 a = fab_load4(g_k + base, u, D, vec, 0.0f), o = fab_load4(g_y + base, u, D, vec, 0.0f);
        f32x4 n;
#pragma unroll
        for (int q = 0; q < 4; ++q) n[q] = a[q] - o[q];
        fab_store4(best_w + base, u, D, vec, n);
    }
}

static inline bool fab_dim_ok(size_t n) { return n > 0 && n <= ((size_t)1 << 30); }
static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace rvlm

using namespace rvlm;

extern "C" int rvlm_fab_projection_linf(const float* t, const float* w, const float* b, int R, size_t D, float* d,
                                        float* lambda, int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(t && w && b && d && R > 0 && fab_dim_ok(D), "rvlm_fab_projection_linf: bad arguments");
    RVLM_REQUIRE((D & 3) != 0 || (aligned16(t) && aligned16(w) && aligned16(d)),
                 "rvlm_fab_projection_linf: rows must be 16-byte aligned");
    hipLaunchKernelGGL(fab_projection_linf_kernel, dim3(R), dim3(FAB_THREADS), 0, (hipStream_t)stream, t, w, b, (int)D, d,
                       lambda, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_fab_linf_step(float* x1, const float* x0, const float* dg, const float* df, int B, size_t n_per_sample,
                                  float alpha_max, float eta, float* lambda, int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(x1 && x0 && dg && df && B > 0 && fab_dim_ok(n_per_sample), "rvlm_fab_linf_step: bad arguments");
    RVLM_REQUIRE((n_per_sample & 3) != 0 || (aligned16(x1) && aligned16(x0) && aligned16(dg)),
                 "rvlm_fab_linf_step: images must be 16-byte aligned");
    hipLaunchKernelGGL(fab_linf_step_kernel, dim3(B), dim3(FAB_THREADS), 0, (hipStream_t)stream, x1, x0, dg, df,
                       (int)n_per_sample, alpha_max, eta, lambda, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_fab_track_best(float* x1, const float* x0, float* adv, float* res2, const uint8_t* pred_eq, float beta,
                                   int B, size_t n_per_sample, rvlm_stream_t stream) {
    RVLM_REQUIRE(x1 && x0 && adv && res2 && pred_eq && B > 0 && fab_dim_ok(n_per_sample), "rvlm_fab_track_best: bad arguments");
    RVLM_REQUIRE((n_per_sample & 3) != 0 || (aligned16(x1) && aligned16(x0) && aligned16(adv)),
                 "rvlm_fab_track_best: images must be 16-byte aligned");
    hipLaunchKernelGGL(fab_track_best_kernel, dim3(B), dim3(FAB_THREADS), 0, (hipStream_t)stream, x1, x0, adv, res2, pred_eq,
                       beta, (int)n_per_sample);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_fab_jacobian_argmin(const float* g_k, const float* g_y, const float* df_k, const int64_t* y, int k, int B,
                                        size_t n_per_sample, float* best_dist, float* best_df, float* best_w,
                                        rvlm_stream_t stream) {
    RVLM_REQUIRE(g_k && g_y && df_k && y && best_dist && best_df && best_w && B > 0 && k >= 0 && fab_dim_ok(n_per_sample),
                 "rvlm_fab_jacobian_argmin: bad arguments");
    RVLM_REQUIRE((n_per_sample & 3) != 0 || (aligned16(g_k) && aligned16(g_y) && aligned16(best_w)),
                 "rvlm_fab_jacobian_argmin: gradients must be 16-byte aligned");
    hipLaunchKernelGGL(fab_jacobian_argmin_kernel, dim3(B), dim3(FAB_THREADS), 0, (hipStream_t)stream, g_k, g_y, df_k, y, k,
                       (int)n_per_sample, best_dist, best_df, best_w);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
