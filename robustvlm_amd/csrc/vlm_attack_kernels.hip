// The PGD update and the APGD step, L-inf and L2, for every caller: the pooled-embedding attacks (train/pgd_train.py:38-63,
// train/apgd_train.py:205-254; rvlm_pgd_linf_update, rvlm_pgd_l2_update, rvlm_apgd_linf_step, rvlm_apgd_l2_step) and the masked
// VLM-side attacks (vlm_eval/attacks/pgd.py, apgd.py; RVLM_HAS_VLM_ATTACKS).  One kernel per formula: the pooled entries are its
// mask-less case, mask == NULL and n_img == 1.
//
// The attacked tensor is [B, n_img, P] fp32 (P = elements of one image: the reference's [B, n_img, 1, 3, H, W] with everything
// behind axis 1 flattened) and the reference's full-size 0/1 mask is constant behind axis 1, so it travels as uint8 mask[n_img]
// (1 = attacked, 0 = masked out; NULL = every image attacked).  Per iteration:
//   PGD.perturb  pgd.py:39-65   -> rvlm_pgd_masked_update                        (1 launch; the reference: ~20 + 2 host asserts)
//   apgd         apgd.py:240-266 -> rvlm_apgd_masked_step                        (1 launch)
//                apgd.py:321-351 -> rvlm_apgd_masked_bookkeeping                 (2 launches, no nonzero() read-back)
// Arithmetic: SURVEY.md Appendix A - one IEEE fp32 rounding per reference op in the reference's order, no contraction
// (-ffp-contract=off).  Clamps propagate NaN like torch.clamp / torch.min / torch.max do (so a NaN reaches the flag the reference's
// assert stands for); NaN / range asserts become bits of a device flag word that the host reads once after the loop.
// A masked gradient is `g * 0` as in the reference, not a skipped element: NaN / Inf under a 0 of the mask becomes NaN there too.
//
// Masked images and bit-identity.  The reference never skips a masked image, it steps it along a zero gradient and projects it
// with the rest of its sample; so do these kernels.  What comes out is bit-identical to what went in
//   L-inf: whenever the image already lies in the eps-ball and in [0,1] (every output of these kernels does, and so does the
//          start clamp(x, 0, 1) of an x in [0,1]) and, for APGD, x_adv_old == x_adv there (it always is: the image never moved);
//   L2:    whenever the image equals x there (no pert_init on it): the sample-wide rescale multiplies an exact 0.
// With a pert_init on a masked image the reference itself re-rounds (L2) or projects (L-inf, outside the ball) that image.
//
// L-inf kernels: blockIdx.y = b * n_img + image, the mask byte is uniform per workgroup, 16-byte accesses when P % 4 == 0 and
// every pointer is 16-byte aligned, the scalar instantiation otherwise (image bases are then not 16-byte aligned).  L2 kernels:
// one workgroup of 1024 threads owns one sample and walks it once per dependent norm (the later walks are L2-cache reads: the
// four tensors of a 3 x 224 x 224 sample are 2.4 MB); sums are fp32 in a fixed order - lane partials over (image, element) in
// ascending order, wave shuffles, 16 wave partials in LDS added in wave order - so results are bit-reproducible run to run, equal
// to torch's to fp32 rounding of the norms.  The only atomic is the OR into the flags word, whose value does not depend on order.
#include "attack_common.h"

namespace rvlm {
namespace {

// torch.clamp / torch.min / torch.max return NaN for a NaN operand (fminf / fmaxf would drop it)
__device__ __forceinline__ float clampn(float v, float lo, float hi) { return (v != v) ? v : fminf(fmaxf(v, lo), hi); }
__device__ __forceinline__ float maskg(float g, bool on) { return on ? g : g * 0.0f; }   // mask * gradient
__device__ __forceinline__ bool out_of_image(float s) { return !(s < 1.000001f && s > -1e-6f); }   // pgd.py:62-64

template <int V> __device__ __forceinline__ void ld(const float* p, float (&r)[V]) {
    if constexpr (V == 4) *(float4*)r = *(const float4*)p; else r[0] = *p;
}
template <int V> __device__ __forceinline__ void st(float* p, const float (&r)[V]) {
    if constexpr (V == 4) *(float4*)p = *(const float4*)r; else *p = r[0];
}
__device__ __forceinline__ void raise_flags(int32_t* flags, int f) {
    if (!flags) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) f |= __shfl_xor(f, o, 64);
    if (f && (threadIdx.x & 63) == 0) atomicOr(flags, f);
}
// one sample [n_img, P] by a workgroup of 1024 threads: f(offset in the sample, image attacked?) on V consecutive elements
template <int V, typename F>
__device__ __forceinline__ void for_sample(int n_img, size_t P, const uint8_t* __restrict__ mask, F&& f) {
    for (int im = 0; im < n_img; ++im) {
        const bool on = !mask || mask[im];
        const size_t off = (size_t)im * P;
        for (size_t j = (size_t)threadIdx.x * V; j < P; j += (size_t)1024 * V) f(off + j, on);
    }
}

// ---- rvlm_mask_grad: out = mask * grad (apgd.py:223-224, pgd.py:40) ----------------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256)
mask_grad_kernel(const float* __restrict__ grad, const uint8_t* __restrict__ mask, int n_img, size_t P, float* __restrict__ out,
                 int32_t* flags) {
    const bool on = !mask || mask[blockIdx.y % n_img];
    const size_t base = (size_t)blockIdx.y * P;
    int f = 0;
    for (size_t j = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; j < P; j += (size_t)gridDim.x * 256 * V) {
        float g[V];
        ld<V>(grad + base + j, g);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            g[e] = maskg(g[e], on);
            if (g[e] != g[e]) f |= RVLM_FLAG_NAN_GRAD;
        }
        st<V>(out + base + j, g);
    }
    raise_flags(flags, f);
}

// ---- rvlm_pgd_masked_update, L-inf (pgd.py:39-65 with utils.py:9-11,20-21) ---------------------------------------------------
template <int V>
__global__ void __launch_bounds__(256)
pgd_masked_linf_kernel(const float* __restrict__ x, const float* __restrict__ grad, float* __restrict__ delta,
                       float* __restrict__ vel, const uint8_t* __restrict__ mask, int n_img, size_t P, float eps, float step,
                       float mom, int mode_max, int image_space, float* __restrict__ x_adv_out, int32_t* flags) {
    const bool on = !mask || mask[blockIdx.y % n_img];
    const size_t base = (size_t)blockIdx.y * P;
    int f = 0;
    for (size_t j = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; j < P; j += (size_t)gridDim.x * 256 * V) {
        const size_t i = base + j;
        float xv[V], gv[V], dv[V], vv[V], xa[V];
        ld<V>(x + i, xv); ld<V>(grad + i, gv); ld<V>(delta + i, dv); ld<V>(vel + i, vv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float gi = maskg(gv[e], on);                                   // :40
            if (gi != gi) { gi = 0.0f; f |= RVLM_FLAG_NAN_GRAD; }          // :41-43
            const float s = sgnf(gi);                                      // :45
            const float v = sgnf(mom * vv[e] + s);                         // :47-48
            const float sv = step * v;
            float d = mode_max ? (dv[e] + sv) : (dv[e] - sv);              // :50-53
            d = clampn(d, -eps, eps);                                      // :57
            if (image_space) {
                d = clampn(xv[e] + d, 0.0f, 1.0f) - xv[e];                 // :59-61
                if (out_of_image(xv[e] + d)) f |= RVLM_FLAG_ADV_RANGE;     // :62-64
            }
            if (d != d) f |= RVLM_FLAG_NAN_DELTA;                          // :65
            dv[e] = d; vv[e] = v; xa[e] = xv[e] + d;                       // :71,73
        }
        st<V>(delta + i, dv); st<V>(vel + i, vv);
        if (x_adv_out) st<V>(x_adv_out + i, xa);
    }
    raise_flags(flags, f);
}

// ---- rvlm_pgd_masked_update, L2 (utils.py:12-14,22-26): three dependent per-sample norms, one workgroup per sample -----------
//   g = mask * g; NaN -> 0; g /= max(|g|_2, 1e-12)                (the norm is over the MASKED gradient)
//   v = mom * v + g;  v /= max(|v|_2, 1e-12)
//   d = d +- step * v;  d *= eps / (|d|_2 + 1e-7) if |d|_2 > eps   torch.renorm(d, p=2, dim=0, maxnorm=eps)
//   image_space: d = clamp(x + d, 0, 1) - x
template <int V>
__global__ void __launch_bounds__(1024)
pgd_masked_l2_kernel(const float* __restrict__ x, const float* __restrict__ grad, float* __restrict__ delta,
                     float* __restrict__ vel, const uint8_t* __restrict__ mask, int n_img, size_t P, float eps, float step,
                     float mom, int mode_max, int image_space, float* __restrict__ x_adv_out, int32_t* flags) {
    __shared__ float red[16];
    const size_t base = (size_t)blockIdx.x * n_img * P;
    const float* xs = x + base;
    const float* gs = grad + base;
    float* ds = delta + base;
    float* vs = vel + base;
    int f = 0;
    float acc = 0.0f;
    for_sample<V>(n_img, P, mask, [&](size_t i, bool on) {
        float g[V];
        ld<V>(gs + i, g);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float gi = maskg(g[e], on);
            if (gi != gi) { gi = 0.0f; f |= RVLM_FLAG_NAN_GRAD; }
            acc = fmaf(gi, gi, acc);
        }
    });
    const float gn = fmaxf(sqrtf(block_sum_1024(acc, red)), 1e-12f);
    acc = 0.0f;
    for_sample<V>(n_img, P, mask, [&](size_t i, bool on) {
        float g[V], v[V];
        ld<V>(gs + i, g); ld<V>(vs + i, v);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float gi = maskg(g[e], on);
            if (gi != gi) gi = 0.0f;
            v[e] = mom * v[e] + gi / gn;                 // un-normalised for now (the same thread re-reads it below)
            acc = fmaf(v[e], v[e], acc);
        }
        st<V>(vs + i, v);
    });
    const float vn = fmaxf(sqrtf(block_sum_1024(acc, red)), 1e-12f);
    acc = 0.0f;
    for_sample<V>(n_img, P, mask, [&](size_t i, bool) {
        float v[V], d[V];
        ld<V>(vs + i, v); ld<V>(ds + i, d);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            v[e] = v[e] / vn;
            const float sv = step * v[e];
            d[e] = mode_max ? (d[e] + sv) : (d[e] - sv);
            acc = fmaf(d[e], d[e], acc);
        }
        st<V>(vs + i, v); st<V>(ds + i, d);
    });
    const float dn = sqrtf(block_sum_1024(acc, red));
    const float sc = dn > eps ? eps / (dn + 1e-7f) : 1.0f;
    for_sample<V>(n_img, P, mask, [&](size_t i, bool) {
        float xv[V], d[V], xa[V];
        ld<V>(xs + i, xv); ld<V>(ds + i, d);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float di = d[e] * sc;
            if (image_space) {
                di = clampn(xv[e] + di, 0.0f, 1.0f) - xv[e];
                if (out_of_image(xv[e] + di)) f |= RVLM_FLAG_ADV_RANGE;
            }
            if (di != di) f |= RVLM_FLAG_NAN_DELTA;
            d[e] = di; xa[e] = xv[e] + di;
        }
        st<V>(ds + i, d);
        if (x_adv_out) st<V>(x_adv_out + base + i, xa);
    });
    raise_flags(flags, f);
}

// ---- rvlm_apgd_masked_step, L-inf (apgd.py:243-255) ---------------------------------------------------------------------------
__device__ __forceinline__ float box_linf(float v, float lo, float hi) {     // clamp(min(max(v, x - eps), x + eps), 0, 1)
    return (v != v) ? v : fminf(fmaxf(fminf(fmaxf(v, lo), hi), 0.0f), 1.0f);
}
template <int V>
__global__ void __launch_bounds__(256)
apgd_masked_linf_kernel(const float* __restrict__ x, float* __restrict__ x_adv, float* __restrict__ x_adv_old,
                        const float* __restrict__ grad, const uint8_t* __restrict__ mask, const float* __restrict__ step,
                        float a, float one_minus_a, float eps, int n_img, size_t P, int32_t* flags) {
    const bool on = !mask || mask[blockIdx.y % n_img];
    const float stp = step[blockIdx.y / n_img];
    const size_t base = (size_t)blockIdx.y * P;
    int f = 0;
    for (size_t j = ((size_t)blockIdx.x * 256 + threadIdx.x) * V; j < P; j += (size_t)gridDim.x * 256 * V) {
        const size_t i = base + j;
        float xc[V], xa[V], xo[V], g[V];
        ld<V>(x + i, xc); ld<V>(x_adv + i, xa); ld<V>(x_adv_old + i, xo); ld<V>(grad + i, g);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float gi = maskg(g[e], on);                              // :223-224, :303-304
            if (gi != gi) f |= RVLM_FLAG_NAN_GRAD;
            const float grad2 = xa[e] - xo[e];                             // :243
            const float lo = xc[e] - eps, hi = xc[e] + eps;
            float z = xa[e] + stp * sgnf(gi);                              // :250
            z = box_linf(z, lo, hi);                                       // :251-252
            const float t1 = (z - xa[e]) * a;
            const float t2 = grad2 * one_minus_a;
            xo[e] = xa[e];                                                 // :244
            xa[e] = box_linf((xa[e] + t1) + t2, lo, hi);                   // :253-255
        }
        st<V>(x_adv_old + i, xo); st<V>(x_adv + i, xa);
    }
    raise_flags(flags, f);
}

// ---- rvlm_apgd_masked_step, L2 (apgd.py:257-266): one workgroup per sample, three per-sample norms ----------------------------
//   grad2 = x_adv - x_adv_old;  x_adv_old = x_adv
//   z = x_adv + (step * g) / (|g|_2 + 1e-12)                          g = mask * grad
//   z = clamp(x + (z - x) / (|z - x|_2 + 1e-12) * min(eps, |z - x|_2), 0, 1)
//   u = x_adv + (z - x_adv) * a + grad2 * (1 - a)
//   x_adv = clamp(x + (u - x) / (|u - x|_2 + 1e-12) * min(eps, |u - x|_2), 0, 1)
// z is recomputed instead of stored (x_adv and x_adv_old are rewritten only in the third walk).
template <int V>
__global__ void __launch_bounds__(1024)
apgd_masked_l2_kernel(const float* __restrict__ x, float* __restrict__ x_adv, float* __restrict__ x_adv_old,
                      const float* __restrict__ grad, const uint8_t* __restrict__ mask, const float* __restrict__ step,
                      float a, float one_minus_a, float eps, int n_img, size_t P, int32_t* flags) {
    __shared__ float red[16];
    const size_t base = (size_t)blockIdx.x * n_img * P;
    const float* xs = x + base;
    const float* gs = grad + base;
    float* xas = x_adv + base;
    float* xos = x_adv_old + base;
    const float stp = step[blockIdx.x];
    int f = 0;
    float acc = 0.0f;
    for_sample<V>(n_img, P, mask, [&](size_t i, bool on) {
        float g[V];
        ld<V>(gs + i, g);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float gi = maskg(g[e], on);
            if (gi != gi) f |= RVLM_FLAG_NAN_GRAD;
            acc = fmaf(gi, gi, acc);
        }
    });
    const float gd = sqrtf(block_sum_1024(acc, red)) + 1e-12f;
    acc = 0.0f;
    for_sample<V>(n_img, P, mask, [&](size_t i, bool on) {
        float g[V], xa[V], xc[V];
        ld<V>(gs + i, g); ld<V>(xas + i, xa); ld<V>(xs + i, xc);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            const float z = xa[e] + (stp * maskg(g[e], on)) / gd;
            const float d = z - xc[e];
            acc = fmaf(d, d, acc);
        }
    });
    const float n1 = sqrtf(block_sum_1024(acc, red));
    const float d1 = n1 + 1e-12f, m1 = fminf(eps, n1);
    acc = 0.0f;
    for_sample<V>(n_img, P, mask, [&](size_t i, bool on) {
        float g[V], xa[V], xc[V], xo[V];
        ld<V>(gs + i, g); ld<V>(xas + i, xa); ld<V>(xs + i, xc); ld<V>(xos + i, xo);
#pragma unroll
        for (int e = 0; e < V; ++e) {
            float z = xa[e] + (stp * maskg(g[e], on)) / gd;
            z = clampn(xc[e] + (z - xc[e]) / d1 * m1, 0.0f, 1.0f);
            const float g2 = xa[e] - xo[e];
            const float u = (xa[e] + (z - xa[e]) * a) + g2 * one_minus_a;
            xo[e] = xa[e];
            xa[e] = u;                                    // finished in the last walk
            const float d = u - xc[e];
            acc = fmaf(d, d, acc);
        }
        st<V>(xos + i, xo); st<V>(xas + i, xa);
    });
    const float n2 = sqrtf(block_sum_1024(acc, red));
    const float d2 = n2 + 1e-12f, m2 = fminf(eps, n2);
    for_sample<V>(n_img, P, mask, [&](size_t i, bool) {
        float xa[V], xc[V];
        ld<V>(xas + i, xa); ld<V>(xs + i, xc);
#pragma unroll
        for (int e = 0; e < V; ++e) xa[e] = clampn(xc[e] + (xa[e] - xc[e]) / d2 * m2, 0.0f, 1.0f);
        st<V>(xas + i, xa);
    });
    raise_flags(flags, f);
}

inline bool aligned16(std::initializer_list<const void*> ps) {
    for (const void* p : ps)
        if ((uintptr_t)p & 15) return false;
    return true;
}
// grid of the per-image kernels: x = chunks of one image (at most 64: 256 threads x 4 floats x 64 covers 65 536 elements per
// trip of the grid-stride loop), y = b * n_img + image
inline dim3 image_grid(size_t P, int v, long images) {
    size_t gx = (P / v + 255) / 256;
    gx = gx < 1 ? 1 : (gx > 64 ? 64 : gx);
    return dim3((unsigned)gx, (unsigned)images);
}
inline int shape_ok(int B, int n_img, size_t P) {
    return B > 0 && n_img > 0 && P > 0 && (long)B * n_img <= 65535 && P <= ((size_t)1 << 40);
}

}  // namespace
}  // namespace rvlm

using namespace rvlm;

extern "C" int rvlm_mask_grad(const float* grad, const uint8_t* mask, int B, int n_img, size_t P, float* out, int32_t* flags,
                              rvlm_stream_t stream) {
    RVLM_REQUIRE(grad && out, "rvlm_mask_grad: null pointer");
    RVLM_REQUIRE(shape_ok(B, n_img, P), "rvlm_mask_grad: B, n_img, P out of range (B * n_img <= 65535)");
    const long images = (long)B * n_img;
    if (P % 4 == 0 && aligned16({grad, out}))
        hipLaunchKernelGGL(mask_grad_kernel<4>, image_grid(P, 4, images), dim3(256), 0, (hipStream_t)stream, grad, mask, n_img, P,
                           out, flags);
    else
        hipLaunchKernelGGL(mask_grad_kernel<1>, image_grid(P, 1, images), dim3(256), 0, (hipStream_t)stream, grad, mask, n_img, P,
                           out, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_pgd_masked_update(const float* x, const float* grad, float* delta, float* velocity, const uint8_t* mask,
                                      int B, int n_img, size_t P, int norm_kind, float eps, float stepsize, float momentum,
                                      int mode_max, int image_space, float* x_adv_out, int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(x && grad && delta && velocity, "rvlm_pgd_masked_update: null pointer");
    RVLM_REQUIRE(shape_ok(B, n_img, P), "rvlm_pgd_masked_update: B, n_img, P out of range (B * n_img <= 65535)");
    if (norm_kind != 0 && norm_kind != 2)
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_pgd_masked_update: norm must be L-inf (0) or L2 (2)");
    const bool vec = P % 4 == 0 && aligned16({x, grad, delta, velocity, x_adv_out});
    const long images = (long)B * n_img;
#define RVLM_PGD_MASKED_ARGS x, grad, delta, velocity, mask, n_img, P, eps, stepsize, momentum, mode_max, image_space, x_adv_out, flags
    if (norm_kind == 0) {
        if (vec)
            hipLaunchKernelGGL(pgd_masked_linf_kernel<4>, image_grid(P, 4, images), dim3(256), 0, (hipStream_t)stream,
                               RVLM_PGD_MASKED_ARGS);
        else
            hipLaunchKernelGGL(pgd_masked_linf_kernel<1>, image_grid(P, 1, images), dim3(256), 0, (hipStream_t)stream,
                               RVLM_PGD_MASKED_ARGS);
    } else {
        if (vec)
            hipLaunchKernelGGL(pgd_masked_l2_kernel<4>, dim3(B), dim3(1024), 0, (hipStream_t)stream, RVLM_PGD_MASKED_ARGS);
        else
            hipLaunchKernelGGL(pgd_masked_l2_kernel<1>, dim3(B), dim3(1024), 0, (hipStream_t)stream, RVLM_PGD_MASKED_ARGS);
    }
#undef RVLM_PGD_MASKED_ARGS
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

extern "C" int rvlm_apgd_masked_step(const float* x, float* x_adv, float* x_adv_old, const float* grad, const uint8_t* mask,
                                     const float* step, float a, float eps, int B, int n_img, size_t P, int norm_kind,
                                     int32_t* flags, rvlm_stream_t stream) {
    RVLM_REQUIRE(x && x_adv && x_adv_old && grad && step, "rvlm_apgd_masked_step: null pointer");
    RVLM_REQUIRE(shape_ok(B, n_img, P), "rvlm_apgd_masked_step: B, n_img, P out of range (B * n_img <= 65535)");
    if (norm_kind != 0 && norm_kind != 2)
        return fail(RVLM_ERR_UNSUPPORTED, "rvlm_apgd_masked_step: norm must be L-inf (0) or L2 (2)");
    const bool vec = P % 4 == 0 && aligned16({x, x_adv, x_adv_old, grad});
    const long images = (long)B * n_img;
    const float oma = (float)(1.0 - (double)a);
#define RVLM_APGD_MASKED_ARGS x, x_adv, x_adv_old, grad, mask, step, a, oma, eps, n_img, P, flags
    if (norm_kind == 0) {
        if (vec)
            hipLaunchKernelGGL(apgd_masked_linf_kernel<4>, image_grid(P, 4, images), dim3(256), 0, (hipStream_t)stream,
                               RVLM_APGD_MASKED_ARGS);
        else
            hipLaunchKernelGGL(apgd_masked_linf_kernel<1>, image_grid(P, 1, images), dim3(256), 0, (hipStream_t)stream,
                               RVLM_APGD_MASKED_ARGS);
    } else {
        if (vec)
            hipLaunchKernelGGL(apgd_masked_l2_kernel<4>, dim3(B), dim3(1024), 0, (hipStream_t)stream, RVLM_APGD_MASKED_ARGS);
        else
            hipLaunchKernelGGL(apgd_masked_l2_kernel<1>, dim3(B), dim3(1024), 0, (hipStream_t)stream, RVLM_APGD_MASKED_ARGS);
    }
#undef RVLM_APGD_MASKED_ARGS
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

// ---- the pooled-embedding entries: the same kernels without a mask, one image per sample --------------------------------------
extern "C" int rvlm_pgd_linf_update(const float* x, const float* grad, float* delta, float* velocity, size_t n, float eps,
                                    float stepsize, float momentum, int mode_max, float* x_adv_out, int32_t* flags,
                                    rvlm_stream_t stream) {
    RVLM_REQUIRE(x && grad && delta && velocity, "rvlm_pgd_linf_update: null pointer");
    // elementwise over the whole batch: ONE row of n elements on the flat grid (image_grid's 64 workgroups per row would leave
    // three quarters of the CUs idle at a batch's 19 M elements)
    if (n % 4 == 0 && aligned16({x, grad, delta, velocity, x_adv_out}))
        hipLaunchKernelGGL(pgd_masked_linf_kernel<4>, dim3(ew_grid(n, 4)), dim3(256), 0, (hipStream_t)stream, x, grad, delta,
                           velocity, nullptr, 1, n, eps, stepsize, momentum, mode_max, 1, x_adv_out, flags);
    else
        hipLaunchKernelGGL(pgd_masked_linf_kernel<1>, dim3(ew_grid(n, 1)), dim3(256), 0, (hipStream_t)stream, x, grad, delta,
                           velocity, nullptr, 1, n, eps, stepsize, momentum, mode_max, 1, x_adv_out, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

// The two pooled L2 entries always take the scalar walk, V = 1: lane t sums elements t, t + 1024, ... - the order their norms
// have always had, so their outputs keep their bits.  The 16-byte walk would be faster and would change the last bits of every
// norm: a change of its own.
extern "C" int rvlm_pgd_l2_update(const float* x, const float* grad, float* delta, float* velocity, size_t n_per_sample, int B,
                                  float eps, float stepsize, float momentum, int mode_max, float* x_adv_out, int32_t* flags,
                                  rvlm_stream_t stream) {
    RVLM_REQUIRE(x && grad && delta && velocity && n_per_sample > 0 && B > 0, "rvlm_pgd_l2_update: bad arguments");
    hipLaunchKernelGGL(pgd_masked_l2_kernel<1>, dim3(B), dim3(1024), 0, (hipStream_t)stream, x, grad, delta, velocity, nullptr, 1,
                       n_per_sample, eps, stepsize, momentum, mode_max, 1, x_adv_out, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

// The two pooled APGD steps with the flag word of the masked entry (RVLM_FLAG_NAN_GRAD): what the public entries below launch with
// flags == NULL, and what the token APGD loop (engine_attacks.hip) launches with its own.  The flag word changes no output bit.
namespace rvlm {
int apgd_step_pooled(int norm_kind, const float* x, float* x_adv, float* x_adv_old, const float* grad, const float* step, float a,
                     float eps, size_t n_per_sample, int B, int32_t* flags, hipStream_t stream) {
    const float oma = (float)(1.0 - (double)a);
    if (norm_kind == 2)
        hipLaunchKernelGGL(apgd_masked_l2_kernel<1>, dim3(B), dim3(1024), 0, stream, x, x_adv, x_adv_old, grad, nullptr, step, a, oma,
                           eps, 1, n_per_sample, flags);
    else if (n_per_sample % 4 == 0 && aligned16({x, x_adv, x_adv_old, grad}))
        hipLaunchKernelGGL(apgd_masked_linf_kernel<4>, image_grid(n_per_sample, 4, B), dim3(256), 0, stream, x, x_adv, x_adv_old, grad,
                           nullptr, step, a, oma, eps, 1, n_per_sample, flags);
    else
        hipLaunchKernelGGL(apgd_masked_linf_kernel<1>, image_grid(n_per_sample, 1, B), dim3(256), 0, stream, x, x_adv, x_adv_old, grad,
                           nullptr, step, a, oma, eps, 1, n_per_sample, flags);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
}  // namespace rvlm

extern "C" int rvlm_apgd_l2_step(const float* x, float* x_adv, float* x_adv_old, const float* grad, const float* step, float a,
                                 float eps, size_t n_per_sample, int B, rvlm_stream_t stream) {
    RVLM_REQUIRE(x && x_adv && x_adv_old && grad && step && B > 0 && n_per_sample > 0, "rvlm_apgd_l2_step: bad args");
    return apgd_step_pooled(2, x, x_adv, x_adv_old, grad, step, a, eps, n_per_sample, B, nullptr, (hipStream_t)stream);
}

extern "C" int rvlm_apgd_linf_step(const float* x, float* x_adv, float* x_adv_old, const float* grad, const float* step, float a,
                                   float eps, size_t n_per_sample, int B, rvlm_stream_t stream) {
    RVLM_REQUIRE(x && x_adv && x_adv_old && grad && step && B > 0 && n_per_sample > 0, "rvlm_apgd_linf_step: bad args");
    return apgd_step_pooled(0, x, x_adv, x_adv_old, grad, step, a, eps, n_per_sample, B, nullptr, (hipStream_t)stream);
}

// apgd.py:321-351 against rvlm_apgd_controller_rho / rvlm_apgd_select (apgd_train.py:301-355), line by line: `y1 > loss_best`
// (strict) selects x_best / grad_best / loss_best; check_oscillation counts `loss_steps[j - c] > loss_steps[j - c - 1]` over k
// steps with negative rows wrapping and compares `t <= k * k3`, k3 = 0.75; fl_reduce_no_impr = (1 - reduced_last_check) *
// (loss_best_last_check >= loss_best); step /= 2 and x_adv, grad <- x_best, grad_best where either holds.  The semantics are the
// same, so NO kernel is added: the one difference is that this apgd has no classifier - it sets x_best_adv = x_adv in every
// iteration (:310) where apgd_train does so only for misclassified samples (:304-305).  That is the controller with pred == 0
// for every sample: the select then copies x_adv into x_best_adv before the restart overwrites it, the order of :310 and :347.
extern "C" int rvlm_apgd_masked_bookkeeping(int i, int B, int n_iter, int k, int do_check, const float* loss_i, float* loss_steps,
                                            float* loss_best, float* loss_best_last_check, float* reduced_last_check, float* step,
                                            float* x_adv, float* grad, float* x_best, float* grad_best, float* x_best_adv,
                                            uint8_t* scratch, size_t n_per_sample, rvlm_stream_t stream) {
    RVLM_REQUIRE(scratch && B > 0 && n_per_sample > 0, "rvlm_apgd_masked_bookkeeping: bad arguments");
    uint8_t* pred = scratch;                 // [B] zeros, kept by the caller: "never classified correctly"
    uint8_t* acc = scratch + B;              // min(acc, pred): unused here
    uint8_t* f_notpred = scratch + 2 * (size_t)B;
    uint8_t* f_improved = scratch + 3 * (size_t)B;
    uint8_t* f_reduced = scratch + 4 * (size_t)B;
    const int rc = rvlm_apgd_controller_rho(i, B, n_iter, k, do_check, 0.75, loss_i, pred, loss_steps, loss_best,
                                            loss_best_last_check, reduced_last_check, step, acc, f_notpred, f_improved, f_reduced,
                                            stream);
    if (rc != RVLM_OK) return rc;
    return rvlm_apgd_select(x_adv, grad, x_best, grad_best, x_best_adv, f_notpred, f_improved, f_reduced, n_per_sample, B, stream);
}
