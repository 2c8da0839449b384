// What the attack loops run around the step: the input range check, the standalone helpers of vlm_eval/attacks/utils.py, the APGD
// controller and select (train/apgd_train.py:301-355 without its nonzero() syncs), the two random starts and the Square kernels (L-inf and L2).
// The PGD update and the APGD step themselves - every caller's, masked or not - are in vlm_attack_kernels.hip.
// Arithmetic follows SURVEY.md Appendix A exactly: one IEEE fp32 rounding per reference op, no FMA contraction (this file is
// built with -ffp-contract=off).  NaN / range asserts become bits of a device flag word that the host reads once after the loop.
#include "attack_common.h"

namespace rvlm {

// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256)
check_range_kernel(const float* __restrict__ x, size_t n, int32_t* flags) {
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (size_t)gridDim.x * blockDim.x) {
        float v = x[i];
        bad |= !(v < 1.000001f && v > -1e-6f);
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(flags, RVLM_FLAG_INPUT_RANGE);
}

// ---- the standalone helpers of vlm_eval/attacks/utils.py:8-26 as device kernels (robustvlm_amd/attack_utils.py) ----
__global__ void __launch_bounds__(256)
ew_clamp_kernel(const float* __restrict__ x, float lo, float hi, size_t n, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float v = x[i];
        out[i] = (v != v) ? v : fminf(fmaxf(v, lo), hi);         // torch.clamp propagates NaN
    }
}
__global__ void __launch_bounds__(256)
ew_sign_kernel(const float* __restrict__ x, size_t n, float* __restrict__ out) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        out[i] = sgnf(x[i]);                                      // sign(+-0) = 0, sign(NaN) = 0 like torch.sign
}
// mode 0: F.normalize(x.view(B, -1), p=2, dim=1): x / max(|x|_2, 1e-12);  mode 1: torch.renorm(x, 2, 0, maxnorm):
// rows with |x|_2 > maxnorm scaled by maxnorm / (|x|_2 + 1e-7)
__global__ void __launch_bounds__(1024)
row_l2_scale_kernel(const float* __restrict__ x, size_t n_per, int mode, float maxnorm, float* __restrict__ out) {
    __shared__ float red[16];
    const size_t base = (size_t)blockIdx.x * n_per;
    float acc = 0.0f;
    for (size_t i = threadIdx.x; i < n_per; i += 1024) acc = fmaf(x[base + i], x[base + i], acc);
    const float nrm = sqrtf(block_sum_1024(acc, red));
    if (mode == 0) {
        const float d = fmaxf(nrm, 1e-12f);
        for (size_t i = threadIdx.x; i < n_per; i += 1024) out[base + i] = x[base + i] / d;
    } else {
        const float sc = nrm > maxnorm ? maxnorm / (nrm + 1e-7f) : 1.0f;
        for (size_t i = threadIdx.x; i < n_per; i += 1024) out[base + i] = x[base + i] * sc;
    }
}

__global__ void apgd_controller_kernel(int i, int B, int n_iter, int k, int do_check, double rho,
                                       const float* __restrict__ loss_i,
                                       const uint8_t* __restrict__ pred, float* loss_steps,
                                       float* loss_best, float* loss_best_last_check,
                                       float* reduced_last_check, float* step, uint8_t* acc,
                                       uint8_t* f_notpred, uint8_t* f_improved,
                                       uint8_t* f_reduced) {
    for (int b = blockIdx.x * blockDim.x + threadIdx.x; b < B; b += gridDim.x * blockDim.x) {
        float y1 = loss_i[b];
        uint8_t p = pred[b];
        acc[b] = acc[b] < p ? acc[b] : p;                        // apgd_train.py:302
        f_notpred[b] = p ? 0 : 1;                                // :304-305
        loss_steps[(size_t)i * B + b] = y1;                      // :322
        int imp = y1 > loss_best[b];                             // :323
        float lb = imp ? y1 : loss_best[b];
        loss_best[b] = lb;
        f_improved[b] = (uint8_t)imp;
        int red = 0;
        if (do_check) {                                          // :331
            float t = 0.0f;
            for (int c = 0; c < k; ++c) {                        // check_oscillation :117-122
                int r0 = i - c, r1 = i - c - 1;
                if (r0 < 0) r0 += n_iter;                        // negative index wraps
                if (r1 < 0) r1 += n_iter;
                float l0 = (r0 == i) ? y1 : loss_steps[(size_t)r0 * B + b];
                float l1 = loss_steps[(size_t)r1 * B + b];
                t += (l0 > l1) ? 1.0f : 0.0f;
            }
            float thr = (float)((double)k * rho);               // `k * k3` in double, then * ones_like(t) (fp32)
            float osc = (t <= thr) ? 1.0f : 0.0f;
            float noimp = (1.0f - reduced_last_check[b]) *
                          ((loss_best_last_check[b] >= lb) ? 1.0f : 0.0f);   // :337-338
            float r = fmaxf(osc, noimp);
            reduced_last_check[b] = r;
            loss_best_last_check[b] = lb;
            if (r > 0.0f) { step[b] = step[b] / 2.0f; red = 1; }            // :346-348
        }
        f_reduced[b] = (uint8_t)red;
    }
}

__global__ void __launch_bounds__(256)
apgd_select_kernel(float* __restrict__ x_adv, float* __restrict__ grad, float* __restrict__ x_best,
                   float* __restrict__ grad_best, float* __restrict__ x_best_adv,
                   const uint8_t* __restrict__ f_notpred, const uint8_t* __restrict__ f_improved,
                   const uint8_t* __restrict__ f_reduced, size_t n_per) {
    const int b = blockIdx.y;
    const bool np = f_notpred[b], im = f_improved[b], rd = f_reduced[b];
    if (!(np || im || rd)) return;
    const size_t base = (size_t)b * n_per;
    for (size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_per;
         j += (size_t)gridDim.x * blockDim.x) {
        size_t i = base + j;
        float xa = x_adv[i], gr = grad[i];
        if (np) x_best_adv[i] = xa;                              // apgd_train.py:305
        float xb, gb;
        if (im) { xb = xa; gb = gr; x_best[i] = xb; grad_best[i] = gb; }   // :324-325
        else if (rd) { xb = x_best[i]; gb = grad_best[i]; }
        if (rd) { x_adv[i] = xb; grad[i] = gb; }                 // :351-352
    }
}

// per-sample max|t| then x + eps * (t / (max + 1e-12))   (autopgd_base.py:180-183, 210-214)
__global__ void __launch_bounds__(256)
linf_random_start_kernel(const float* __restrict__ x, const float* __restrict__ t, float eps,
                         size_t n_per, float* __restrict__ x_adv) {
    __shared__ float red[4];
    const int b = blockIdx.x;
    const size_t base = (size_t)b * n_per;
    float m = 0.0f;
    for (size_t j = threadIdx.x; j < n_per; j += blockDim.x) m = fmaxf(m, fabsf(t[base + j]));
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float den = m + 1e-12f;
    for (size_t j = threadIdx.x; j < n_per; j += blockDim.x) {
        float q = t[base + j] / den;
        float e = eps * 1.0f;            // eps * ones_like(x)
        x_adv[base + j] = x[base + j] + e * q;
    }
}

// L2 random start of APGDAttack (autopgd_base.py:184-185, 215-218): x + eps * (t / (|t|_2 + 1e-12)), t ~ N(0, 1) drawn by the
// caller; one workgroup per sample, the norm a deterministic fp32 sum in this kernel's own order
__global__ void __launch_bounds__(1024)
l2_random_start_kernel(const float* __restrict__ x, const float* __restrict__ t, float eps, size_t n_per,
                       float* __restrict__ x_adv) {
    __shared__ float red[16];
    const size_t base = (size_t)blockIdx.x * n_per;
    float acc = 0.0f;
    for (size_t j = threadIdx.x; j < n_per; j += 1024) acc = fmaf(t[base + j], t[base + j], acc);
    const float den = sqrtf(block_sum_1024(acc, red)) + 1e-12f;
    for (size_t j = threadIdx.x; j < n_per; j += 1024) x_adv[base + j] = x[base + j] + eps * (t[base + j] / den);
}

}  // namespace rvlm

using namespace rvlm;

// ---- Square Attack, L-inf (autoattack/square.py:256-263, 288-291) --------------------------------------------------
// One query: candidates for the n_active still-robust images idx[a], written compactly (the model runs on them next):
//   x_new[a] = clamp(min(max(x_best[idx[a]] + window, x[idx[a]] - eps), x[idx[a]] + eps), 0, 1)
// window = two_eps * sign[c] on rows [vh, vh+s) x columns [vw, vw+s) of every channel c, 0 elsewhere - ONE window per
// query for the whole batch, as in the reference.  Same fp32 operations in the same order (no contraction).
__global__ void __launch_bounds__(256)
square_linf_propose_kernel(const float* __restrict__ x, const float* __restrict__ x_best, const long long* __restrict__ idx,
                           int C, int H, int W, int vh, int vw, int s, float eps, float two_eps,
                           const float* __restrict__ sign, float* __restrict__ x_new) {
    const long n_img = (long)C * H * W;
    const long src = (long)idx[blockIdx.y] * n_img, dst = (long)blockIdx.y * n_img;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_img; e += (long)gridDim.x * blockDim.x) {
        const int col = (int)(e % W), row = (int)((e / W) % H), c = (int)(e / ((long)W * H));
        const bool in = row >= vh && row < vh + s && col >= vw && col < vw + s;
        const float w = in ? two_eps * sign[c] : 0.0f;
        const float xv = x[src + e];
        float v = x_best[src + e] + w;
        v = fminf(fmaxf(v, xv - eps), xv + eps);
        x_new[dst + e] = fminf(fmaxf(v, 0.0f), 1.0f);
    }
}
// accepted candidates replace the incumbent: x_best[idx[a]] = x_new[a] where take[a] != 0
__global__ void __launch_bounds__(256)
square_accept_kernel(float* __restrict__ x_best, const float* __restrict__ x_new, const long long* __restrict__ idx,
                     const float* __restrict__ take, long n_img) {
    if (take[blockIdx.y] == 0.0f) return;
    const long dst = (long)idx[blockIdx.y] * n_img, src = (long)blockIdx.y * n_img;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < n_img; e += (long)gridDim.x * blockDim.x)
        x_best[dst + e] = x_new[src + e];
}

// ---- Square Attack, L2 (autoattack/square.py:339-379) ---------------------------------------------------------------
// One query in one launch, one workgroup of 1024 threads per still-robust image idx[a].  With delta = x_best - x (never stored):
//   pass A, the image:    per channel sum delta^2 over window 1, over window 1 u window 2, and over the rest
//   pass B, window 1:     raw = eta * sign[a, c] + delta / (1e-12 + |delta[win1]|_c), per channel sum raw^2
//   pass C, window 1:     new = raw / (1e-12 + |raw|_c) * sqrt(max(eps^2 - |delta|^2, 0) / C + |delta[win1 u win2]|_c^2), sum new^2
//   pass D, the image:    delta' = new on window 1, else 0 on window 2, else delta;  x_new = clamp(x + delta' / (|delta'| + 1e-12) * eps, 0, 1)
// with |delta'|^2 = (pass A's rest) + (pass C's sums), a sum of non-negative terms.  Every sum is four lane partials -> wave
// shuffles -> the 16 wave partials in LDS added in wave order: the same bits on every run, no atomics.  An image whose sums are
// not finite (NaN / Inf in x, x_best, eta or sign: the reference's asserts, square.py:416-417) raises
// RVLM_FLAG_SQUARE_NONFINITE and its row of x_new is x_best.  W % 4 == 0 and 16-byte pointers: 16-byte accesses; else scalar.
constexpr int SQ_MAXC = 16;

template <int N>
__device__ __forceinline__ void sq_block_sum(float (&v)[N], float* red) {   // red: N * 16 floats; the totals land in every thread
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = wave_sum(v[k]);
    __syncthreads();                                   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) red[k * 16 + (threadIdx.x >> 6)] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) {
        float t = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += red[k * 16 + i];
        v[k] = t;
    }
}
__device__ __forceinline__ bool sq_inside(int row, int col, int r0, int c0, int s) {
    return row >= r0 && row < r0 + s && col >= c0 && col < c0 + s;
}
__device__ __forceinline__ bool sq_finite(float v) { return fabsf(v) <= 3.402823466e+38f; }

__global__ void __launch_bounds__(1024)
square_l2_propose_kernel(const float* __restrict__ x, const float* __restrict__ x_best, const long long* __restrict__ idx,
                         int C, int H, int W, int vh, int vw, int vh2, int vw2, int s, float eps,
                         const float* __restrict__ eta, const float* __restrict__ sign, float* __restrict__ x_new,
                         int32_t* flags, int vec) {
    __shared__ float red[3 * 16];
    __shared__ float s_w1[SQ_MAXC], s_ws[SQ_MAXC], s_rest[SQ_MAXC], s_raw[SQ_MAXC], s_new[SQ_MAXC];
    const int tid = threadIdx.x, HW = H * W, ss = s * s;
    const long D = (long)C * HW;
    const float* __restrict__ xs = x + (long)idx[blockIdx.x] * D;
    const float* __restrict__ xb = x_best + (long)idx[blockIdx.x] * D;
    float* __restrict__ xo = x_new + (long)blockIdx.x * D;
    const float* __restrict__ sg = sign + (long)blockIdx.x * C;

    // ---- pass A
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ pa = xs + (long)c * HW;
        const float* __restrict__ pb = xb + (long)c * HW;
        float a1[4] = {0.0f, 0.0f, 0.0f, 0.0f}, au[4] = {0.0f, 0.0f, 0.0f, 0.0f}, ar[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (vec) {
            for (int u = tid; u < HW / 4; u += 1024) {
                const f32x4 va = *reinterpret_cast<const f32x4*>(pa + 4 * u);
                const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + 4 * u);
                const int row = (4 * u) / W, col = 4 * u - row * W;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float d = vb[k] - va[k], q = d * d;
                    const bool in1 = sq_inside(row, col + k, vh, vw, s), in2 = sq_inside(row, col + k, vh2, vw2, s);
                    a1[k] += in1 ? q : 0.0f;
                    au[k] += (in1 || in2) ? q : 0.0f;
                    ar[k] += (in1 || in2) ? 0.0f : q;
                }
            }
        } else {
            for (int e = tid; e < HW; e += 1024) {
                const float d = pb[e] - pa[e], q = d * d;
                const int row = e / W, col = e - row * W;
                const bool in1 = sq_inside(row, col, vh, vw, s), in2 = sq_inside(row, col, vh2, vw2, s);
                a1[0] += in1 ? q : 0.0f;
                au[0] += (in1 || in2) ? q : 0.0f;
                ar[0] += (in1 || in2) ? 0.0f : q;
            }
        }
        float v[3] = {(a1[0] + a1[1]) + (a1[2] + a1[3]), (au[0] + au[1]) + (au[2] + au[3]), (ar[0] + ar[1]) + (ar[2] + ar[3])};
        sq_block_sum<3>(v, red);
        if (tid == 0) { s_w1[c] = v[0]; s_ws[c] = v[1]; s_rest[c] = v[2]; }
    }
    __syncthreads();
    float img = 0.0f, rest = 0.0f;
    for (int c = 0; c < C; ++c) { img += s_ws[c] + s_rest[c]; rest += s_rest[c]; }
    const float nimg = sqrtf(img);
    const float room = fmaxf(eps * eps - nimg * nimg, 0.0f) / (float)C;

    // ---- pass B
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ pa = xs + (long)c * HW;
        const float* __restrict__ pb = xb + (long)c * HW;
        const float den1 = 1e-12f + sqrtf(s_w1[c]), sgc = sg[c];
        float v[1] = {0.0f};
        for (int t = tid; t < ss; t += 1024) {
            const int i = t / s, j = t - i * s, off = (vh + i) * W + vw + j;
            const float raw = eta[t] * sgc + (pb[off] - pa[off]) / den1;
            v[0] += raw * raw;
        }
        sq_block_sum<1>(v, red);
        if (tid == 0) s_raw[c] = v[0];
    }
    __syncthreads();
    // ---- pass C
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ pa = xs + (long)c * HW;
        const float* __restrict__ pb = xb + (long)c * HW;
        const float den1 = 1e-12f + sqrtf(s_w1[c]), sgc = sg[c], den2 = 1e-12f + sqrtf(s_raw[c]);
        const float nws = sqrtf(s_ws[c]), fac = sqrtf(room + nws * nws);
        float v[1] = {0.0f};
        for (int t = tid; t < ss; t += 1024) {
            const int i = t / s, j = t - i * s, off = (vh + i) * W + vw + j;
            const float raw = eta[t] * sgc + (pb[off] - pa[off]) / den1;
            const float nw = raw / den2 * fac;
            v[0] += nw * nw;
        }
        sq_block_sum<1>(v, red);
        if (tid == 0) s_new[c] = v[0];
    }
    __syncthreads();
    float total = rest;
    bool bad = !sq_finite(img);
    for (int c = 0; c < C; ++c) { total += s_new[c]; bad |= !sq_finite(s_raw[c]); }
    bad |= !sq_finite(total);
    if (bad) {                                                   // uniform over the workgroup
        for (long e = tid; e < D; e += 1024) xo[e] = xb[e];
        if (tid == 0 && flags) atomicOr(flags, RVLM_FLAG_SQUARE_NONFINITE);
        return;
    }
    const float denf = sqrtf(total) + 1e-12f;

    // ---- pass D
    for (int c = 0; c < C; ++c) {
        const float* __restrict__ pa = xs + (long)c * HW;
        const float* __restrict__ pb = xb + (long)c * HW;
        float* __restrict__ po = xo + (long)c * HW;
        const float den1 = 1e-12f + sqrtf(s_w1[c]), sgc = sg[c], den2 = 1e-12f + sqrtf(s_raw[c]);
        const float nws = sqrtf(s_ws[c]), fac = sqrtf(room + nws * nws);
        if (vec) {
            for (int u = tid; u < HW / 4; u += 1024) {
                const f32x4 va = *reinterpret_cast<const f32x4*>(pa + 4 * u);
                const f32x4 vb = *reinterpret_cast<const f32x4*>(pb + 4 * u);
                const int row = (4 * u) / W, col = 4 * u - row * W;
                f32x4 o;
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float d = vb[k] - va[k];
                    if (sq_inside(row, col + k, vh, vw, s))
                        d = (eta[(row - vh) * s + (col + k - vw)] * sgc + d / den1) / den2 * fac;
                    else if (sq_inside(row, col + k, vh2, vw2, s))
                        d = 0.0f;
                    o[k] = fminf(fmaxf(va[k] + d / denf * eps, 0.0f), 1.0f);
                }
                *reinterpret_cast<f32x4*>(po + 4 * u) = o;
            }
        } else {
            for (int e = tid; e < HW; e += 1024) {
                const int row = e / W, col = e - row * W;
                const float xv = pa[e];
                float d = pb[e] - xv;
                if (sq_inside(row, col, vh, vw, s))
                    d = (eta[(row - vh) * s + (col - vw)] * sgc + d / den1) / den2 * fac;
                else if (sq_inside(row, col, vh2, vw2, s))
                    d = 0.0f;
                po[e] = fminf(fmaxf(xv + d / denf * eps, 0.0f), 1.0f);
            }
        }
    }
}

extern "C" int rvlm_check_image_range(const float* x, size_t n, int32_t* flags,
                                      rvlm_stream_t stream) {
    RVLM_REQUIRE(x && flags, "rvlm_check_image_range: null pointer");
    hipLaunchKernelGGL(check_range_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, (hipStream_t)stream,
                       x, n, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_project_perturbation(const float* pert, size_t n_per_sample, int B, int norm_kind, float eps, float* out,
                                         rvlm_stream_t stream) {
    RVLM_REQUIRE(pert && out && B > 0 && n_per_sample > 0, "rvlm_project_perturbation: bad arguments");
    const size_t n = n_per_sample * (size_t)B;
    if (norm_kind == 0)
        hipLaunchKernelGGL(ew_clamp_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, (hipStream_t)stream, pert, -eps, eps, n, out);
    else if (norm_kind == 2)
        hipLaunchKernelGGL(row_l2_scale_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, pert, n_per_sample, 1, eps, out);
    else
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_project_perturbation: norm must be L-inf (0) or L2 (2)");
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
extern "C" int rvlm_normalize_grad(const float* grad, size_t n_per_sample, int B, int norm_kind, float* out,
                                   rvlm_stream_t stream) {
    RVLM_REQUIRE(grad && out && B > 0 && n_per_sample > 0, "rvlm_normalize_grad: bad arguments");
    const size_t n = n_per_sample * (size_t)B;
    if (norm_kind == 0)
        hipLaunchKernelGGL(ew_sign_kernel, dim3(ew_grid(n, 1)), dim3(256), 0, (hipStream_t)stream, grad, n, out);
    else if (norm_kind == 2)
        hipLaunchKernelGGL(row_l2_scale_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, grad, n_per_sample, 0, 0.0f, out);
    else
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_normalize_grad: norm must be L-inf (0) or L2 (2)");
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_apgd_controller_rho(int i, int B, int n_iter, int k, int do_check, double rho,
                                        const float* loss_i, const uint8_t* pred, float* loss_steps,
                                        float* loss_best, float* loss_best_last_check,
                                        float* reduced_last_check, float* step, uint8_t* acc,
                                        uint8_t* f_notpred, uint8_t* f_improved, uint8_t* f_reduced,
                                        rvlm_stream_t stream) {
    RVLM_REQUIRE(loss_i && pred && loss_steps && loss_best && loss_best_last_check &&
                     reduced_last_check && step && acc && f_notpred && f_improved && f_reduced,
                 "rvlm_apgd_controller: null pointer");
    RVLM_REQUIRE(i >= 0 && i < n_iter && k >= 1 && B > 0, "rvlm_apgd_controller: bad sizes");
    RVLM_REQUIRE(rho == rho, "rvlm_apgd_controller: rho is NaN");
    hipLaunchKernelGGL(apgd_controller_kernel, dim3(cdiv(B, 256)), dim3(256), 0,
                       (hipStream_t)stream, i, B, n_iter, k, do_check, rho, loss_i, pred, loss_steps,
                       loss_best, loss_best_last_check, reduced_last_check, step, acc, f_notpred,
                       f_improved, f_reduced);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_apgd_controller(int i, int B, int n_iter, int k, int do_check,
                                    const float* loss_i, const uint8_t* pred, float* loss_steps,
                                    float* loss_best, float* loss_best_last_check,
                                    float* reduced_last_check, float* step, uint8_t* acc,
                                    uint8_t* f_notpred, uint8_t* f_improved, uint8_t* f_reduced,
                                    rvlm_stream_t stream) {
    return rvlm_apgd_controller_rho(i, B, n_iter, k, do_check, 0.75, loss_i, pred, loss_steps, loss_best,
                                    loss_best_last_check, reduced_last_check, step, acc, f_notpred, f_improved,
                                    f_reduced, stream);
}

extern "C" int rvlm_apgd_select(float* x_adv, float* grad, float* x_best, float* grad_best,
                                float* x_best_adv, const uint8_t* f_notpred,
                                const uint8_t* f_improved, const uint8_t* f_reduced,
                                size_t n_per_sample, int B, rvlm_stream_t stream) {
    RVLM_REQUIRE(x_adv && grad && x_best && grad_best && x_best_adv && f_notpred && f_improved &&
                     f_reduced && B > 0, "rvlm_apgd_select: bad args");
    int gx = (int)((n_per_sample + 1023) / 1024);
    if (gx > 64) gx = 64;
    hipLaunchKernelGGL(apgd_select_kernel, dim3(gx, B), dim3(256), 0, (hipStream_t)stream, x_adv,
                       grad, x_best, grad_best, x_best_adv, f_notpred, f_improved, f_reduced,
                       n_per_sample);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_linf_random_start(const float* x, const float* t, float eps,
                                      size_t n_per_sample, int B, float* x_adv,
                                      rvlm_stream_t stream) {
    RVLM_REQUIRE(x && t && x_adv && B > 0, "rvlm_linf_random_start: bad args");
    hipLaunchKernelGGL(linf_random_start_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, x, t,
                       eps, n_per_sample, x_adv);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_l2_random_start(const float* x, const float* t, float eps, size_t n_per_sample, int B, float* x_adv,
                                    rvlm_stream_t stream) {
    RVLM_REQUIRE(x && t && x_adv && B > 0 && n_per_sample > 0, "rvlm_l2_random_start: bad args");
    hipLaunchKernelGGL(l2_random_start_kernel, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, t, eps, n_per_sample, x_adv);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_square_linf_propose(const float* x, const float* x_best, const int64_t* idx, int n_active, int C,
                                        int H, int W, int vh, int vw, int s, float eps, const float* sign,
                                        float* x_new, rvlm_stream_t stream) {
    RVLM_REQUIRE(x && x_best && idx && sign && x_new && n_active > 0 && C > 0 && H > 0 && W > 0,
                 "rvlm_square_linf_propose: bad args");
    RVLM_REQUIRE(s >= 1 && vh >= 0 && vw >= 0 && vh + s <= H && vw + s <= W, "rvlm_square_linf_propose: window outside the image");
    const long n_img = (long)C * H * W;
    const int gx = (int)std::min<long>((n_img + 255) / 256, 64);
    hipLaunchKernelGGL(square_linf_propose_kernel, dim3(gx, n_active), dim3(256), 0, (hipStream_t)stream, x, x_best,
                       (const long long*)idx, C, H, W, vh, vw, s, eps, 2.0f * eps, sign, x_new);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
extern "C" int rvlm_square_l2_propose(const float* x, const float* x_best, const int64_t* idx, int n_active, int C, int H,
                                      int W, int vh, int vw, int vh2, int vw2, int s, float eps, const float* eta,
                                      const float* sign, float* x_new, int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(x && x_best && idx && eta && sign && x_new && n_active > 0 && C > 0 && H > 0 && W > 0 &&
                     (long)H * W <= 0x7fffffffL, "rvlm_square_l2_propose: bad args");
    if (C > SQ_MAXC) return fail(RVLM_ERR_UNSUPPORTED, "rvlm_square_l2_propose: more than 16 channels");
    RVLM_REQUIRE(s >= 1 && vh >= 0 && vw >= 0 && vh + s <= H && vw + s <= W && vh2 >= 0 && vw2 >= 0 && vh2 + s <= H && vw2 + s <= W,
                 "rvlm_square_l2_propose: window outside the image");
    RVLM_REQUIRE(eps > 0.0f && eps <= 3.402823466e+38f, "rvlm_square_l2_propose: eps must be finite and positive");
    const int vec = W % 4 == 0 && (((uintptr_t)x | (uintptr_t)x_best | (uintptr_t)x_new) & 15) == 0;
    hipLaunchKernelGGL(square_l2_propose_kernel, dim3(n_active), dim3(1024), 0, (hipStream_t)stream, x, x_best,
                       (const long long*)idx, C, H, W, vh, vw, vh2, vw2, s, eps, eta, sign, x_new, flags, vec);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
extern "C" int rvlm_square_accept(float* x_best, const float* x_new, const int64_t* idx, const float* take, int n_active,
                                  size_t n_per_image, rvlm_stream_t stream) {
    RVLM_REQUIRE(x_best && x_new && idx && take && n_active > 0 && n_per_image > 0, "rvlm_square_accept: bad args");
    const int gx = (int)std::min<size_t>((n_per_image + 255) / 256, 64);
    hipLaunchKernelGGL(square_accept_kernel, dim3(gx, n_active), dim3(256), 0, (hipStream_t)stream, x_best, x_new,
                       (const long long*)idx, take, (long)n_per_image);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
