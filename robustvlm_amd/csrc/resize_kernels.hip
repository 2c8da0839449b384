// Bicubic resize as part of the model (CLIP_eval/clip_robustbench.py:60-68: logits = head(encode_image(Normalize(resizer(x))))
// with resizer = Resize(224, BICUBIC, antialias=False)): forward, adjoint, and the two forms fused into the patch embedding.
//
// The operator is F.interpolate(x, (H, W), mode='bicubic', align_corners=False, antialias=False) on float tensors: separable and
// linear, Y = R_h X R_w^T.  Per output index o: src = (in / out) (o + 0.5) - 0.5, i = floor(src), t = src - i, taps i-1 .. i+2 with
// the index clamped to [0, in-1], cubic-convolution weights with A = -0.75.  The result is NOT clamped (overshoot goes on to
// Normalize).  Tap tables are computed once per (in, out) on the host in double and rounded to fp32 (as the taps of preprocess.hip).
//
// The adjoint gx = R_h^T gy R_w is a GATHER: the tables carry, per INPUT index, the list of (output index, weight) pairs whose taps
// name it, in (output index, tap) order; a clamped tap is an entry of the border pixel like any other.  One thread per low-resolution
// pixel sums its rows x columns in that fixed order: no atomics, the same bits every run.  Cost of either direction: 16 loads per
// HIGH-resolution pixel, whatever the ratio.
#include <cmath>
#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "kernels.h"

namespace rvlm {

static double cubic_near(double x, double A) { return ((A + 2.0) * x - (A + 3.0)) * x * x + 1.0; }          // |x| <= 1
static double cubic_far(double x, double A) { return ((A * x - 5.0 * A) * x + 8.0 * A) * x - 4.0 * A; }     // 1 < |x| < 2

void resize_taps_host(int in, int out, int32_t* idx, float* w) {
    const double scale = (double)in / (double)out, A = -0.75;
    for (int o = 0; o < out; ++o) {
        const double src = scale * ((double)o + 0.5) - 0.5;
        const double fl = std::floor(src), t = src - fl;
        const int i0 = (int)fl;
        const double c[4] = {cubic_far(t + 1.0, A), cubic_near(t, A), cubic_near(1.0 - t, A), cubic_far(2.0 - t, A)};
        for (int k = 0; k < 4; ++k) {
            const int i = i0 - 1 + k;
            idx[o * 4 + k] = i < 0 ? 0 : (i > in - 1 ? in - 1 : i);
            w[o * 4 + k] = (float)c[k];
        }
    }
}

// Device tables of one (device, in, out): one allocation of 16 out + in + 1 words, kept for the life of the process (a few KB per
// pair of sizes; the handful of resolutions an evaluation uses).
int resize_axis_device(int in, int out, ResizeAxis* ax) {
    static std::mutex mu;
    static std::map<std::tuple<int, int, int>, ResizeAxis> cache;
    if (in < 1 || out < 1 || in > (1 << 15) || out > (1 << 15)) return fail(RVLM_ERR_ARG, "resize: sizes must be in 1..32768");
    int dev = 0;
    RVLM_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    const auto key = std::make_tuple(dev, in, out);
    const auto it = cache.find(key);
    if (it != cache.end()) { *ax = it->second; return RVLM_OK; }
    const size_t n4 = (size_t)out * 4;
    std::vector<int32_t> words(4 * n4 + in + 1);
    int32_t* idx = words.data();
    float* w = reinterpret_cast<float*>(words.data() + n4);
    int32_t* adj_o = words.data() + 2 * n4;
    float* adj_w = reinterpret_cast<float*>(words.data() + 3 * n4);
    int32_t* adj_start = words.data() + 4 * n4;
    resize_taps_host(in, out, idx, w);
    // counting sort of the 4 out taps by the input index they name; (o, k) order within one input index
    for (int i = 0; i <= in; ++i) adj_start[i] = 0;
    for (size_t e = 0; e < n4; ++e) adj_start[idx[e] + 1] += 1;
    for (int i = 0; i < in; ++i) adj_start[i + 1] += adj_start[i];
    std::vector<int32_t> fill(adj_start, adj_start + in);
    for (size_t e = 0; e < n4; ++e) {
        const int32_t at = fill[idx[e]]++;
        adj_o[at] = (int32_t)(e / 4);
        adj_w[at] = w[e];
    }
    int32_t* d = nullptr;
    RVLM_HIP(hipMalloc(&d, words.size() * 4));
    const hipError_t e = hipMemcpy(d, words.data(), words.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d); return fail(RVLM_ERR_HIP, std::string("resize tables: ") + hipGetErrorString(e)); }
    ResizeAxis a;
    a.in = in; a.out = out;
    a.idx = d; a.w = reinterpret_cast<const float*>(d + n4);
    a.adj_o = d + 2 * n4; a.adj_w = reinterpret_cast<const float*>(d + 3 * n4); a.adj_start = d + 4 * n4;
    cache[key] = a;
    *ax = a;
    return RVLM_OK;
}

// One output pixel from a low-resolution plane: four rows, each the horizontal cubic of its four (x (+ delta)) values, then the
// vertical cubic of the four row results - the order F.interpolate's CPU kernel sums in.
template <typename I>
__device__ __forceinline__ float resize_pixel(const float* __restrict__ xp, const float* __restrict__ dp, int w_in, const int4 iy,
                                              const float4 wy, const int4 ix, const float4 wx) {
    const int ry[4] = {iy.x, iy.y, iy.z, iy.w};
    const float cy[4] = {wy.x, wy.y, wy.z, wy.w};
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const I r = (I)ry[i] * w_in;
        float v0 = xp[r + ix.x], v1 = xp[r + ix.y], v2 = xp[r + ix.z], v3 = xp[r + ix.w];
        if (dp) { v0 = v0 + dp[r + ix.x]; v1 = v1 + dp[r + ix.y]; v2 = v2 + dp[r + ix.z]; v3 = v3 + dp[r + ix.w]; }
        const float row = ((wx.x * v0 + wx.y * v1) + wx.z * v2) + wx.w * v3;
        acc = acc + cy[i] * row;
    }
    return acc;
}

template <typename I>
__global__ void __launch_bounds__(256)
resize_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, I planes, ResizeAxis ah, ResizeAxis aw) {
    const int H = ah.out, W = aw.out, h = ah.in, w = aw.in;
    const I total = planes * H * W;
    for (I idx = (I)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (I)gridDim.x * blockDim.x) {
        const int ox = (int)(idx % W);
        const I t = idx / W;
        const int oy = (int)(t % H);
        const I p = t / H;
        y[idx] = resize_pixel<I>(x + p * h * w, nullptr, w, reinterpret_cast<const int4*>(ah.idx)[oy],
                                 reinterpret_cast<const float4*>(ah.w)[oy], reinterpret_cast<const int4*>(aw.idx)[ox],
                                 reinterpret_cast<const float4*>(aw.w)[ox]);
    }
}

// The resizing twin of im2col_kernel (vit_kernels.hip): A0[row, col] = (resize(x (+ delta)) - mean_c) / std_c; x and delta are
// [B, 3, h, w] (the perturbation lives in the small space and is added BEFORE the resize).
template <typename T, typename I>
__global__ void __launch_bounds__(256)
resize_im2col_kernel(const float* __restrict__ x, const float* __restrict__ delta, int B, ResizeAxis ah, ResizeAxis aw, int P,
                     float m0, float m1, float m2, float s0, float s1, float s2, T* __restrict__ A0, long lda, int Kpad) {
    const int g = ah.out / P, PP = P * P, K = 3 * PP, h = ah.in, w = aw.in;
    const I total = (I)B * g * g * Kpad;
    for (I idx = (I)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (I)gridDim.x * blockDim.x) {
        const int col = (int)(idx % Kpad);
        const I row = idx / Kpad;
        float v = 0.0f;
        if (col < K) {
            const int c = col / PP, r = col - c * PP, i = r / P, j = r - i * P;
            const int px = (int)(row % g);
            const I t = row / g;
            const int py = (int)(t % g);
            const I b = t / g;
            const int oy = py * P + i, ox = px * P + j;
            const I po = (b * 3 + c) * h * w;
            const float pix = resize_pixel<I>(x + po, delta ? delta + po : nullptr, w, reinterpret_cast<const int4*>(ah.idx)[oy],
                                              reinterpret_cast<const float4*>(ah.w)[oy], reinterpret_cast<const int4*>(aw.idx)[ox],
                                              reinterpret_cast<const float4*>(aw.w)[ox]);
            const float mu = c == 0 ? m0 : (c == 1 ? m1 : m2);
            const float sd = c == 0 ? s0 : (c == 1 ? s1 : s2);
            v = (pix - mu) / sd;
        }
        A0[row * lda + col] = from_f32<T>(v);
    }
}

// gx[p, iy, ix] = sum over the (oy, wy) of iy, over the (ox, wx) of ix: wy wx src(p, oy, ox)   [ / std_c ].
// src is addressed as base(p) + offh[oy] + offw[ox] with the two offset tables in LDS, which covers both layouts:
//   P == 0: gy [planes, H, W]:                 base = p H W,                        offh = oy W,                       offw = ox
//   P  > 0: dA0 [B g g, lda] (col2im layout):  base = (p / 3) g g lda + (p % 3) PP,  offh = (oy / P) g lda + (oy % P) P,  offw = (ox / P) lda + ox % P
// so the tail of the engine needs no full-resolution gradient image.
template <typename T, typename I>
__global__ void __launch_bounds__(256)
resize_adjoint_kernel(const T* __restrict__ src, long lda, int P, float s0, float s1, float s2, I planes, ResizeAxis ah,
                      ResizeAxis aw, float* __restrict__ gx) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    I* offh = reinterpret_cast<I*>(smem_raw);
    I* offw = offh + ah.out;
    const int H = ah.out, W = aw.out, h = ah.in, w = aw.in;
    const int g = P > 0 ? H / P : 0;
    for (int o = threadIdx.x; o < H; o += blockDim.x) offh[o] = P > 0 ? ((I)(o / P) * g * lda + (I)(o % P) * P) : (I)o * W;
    for (int o = threadIdx.x; o < W; o += blockDim.x) offw[o] = P > 0 ? ((I)(o / P) * lda + (o % P)) : (I)o;
    __syncthreads();
    const I total = planes * h * w;
    for (I idx = (I)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (I)gridDim.x * blockDim.x) {
        const int ix = (int)(idx % w);
        const I t = idx / w;
        const int iy = (int)(t % h);
        const I p = t / h;
        const int c = (int)(p % 3);
        const I base = P > 0 ? ((p / 3) * g * g * lda + (I)c * P * P) : p * H * W;
        const int hs = ah.adj_start[iy], he = ah.adj_start[iy + 1], ws = aw.adj_start[ix], we = aw.adj_start[ix + 1];
        float acc = 0.0f;
        for (int a = hs; a < he; ++a) {
            const I ro = base + offh[ah.adj_o[a]];
            float row = 0.0f;
            for (int e = ws; e < we; ++e) row = row + aw.adj_w[e] * to_f32(src[ro + offw[aw.adj_o[e]]]);
            acc = acc + ah.adj_w[a] * row;
        }
        if (P > 0) acc = acc / (c == 0 ? s0 : (c == 1 ? s1 : s2));      // Normalize's 1 / std, once per pixel (the operator is linear)
        gx[idx] = acc;
    }
}

static int ew_grid(long total) {
    long grid = (total + 255) / 256;
    return (int)(grid > 256 * 16 ? 256 * 16 : (grid < 1 ? 1 : grid));
}

int resize_bicubic_fwd(const float* x, long planes, const ResizeAxis& ah, const ResizeAxis& aw, float* y, hipStream_t s) {
    const long total = planes * ah.out * aw.out;
    if (total < (1L << 30) && planes * ah.in * aw.in < (1L << 30))
        hipLaunchKernelGGL((resize_fwd_kernel<int>), dim3(ew_grid(total)), dim3(256), 0, s, x, y, (int)planes, ah, aw);
    else
        hipLaunchKernelGGL((resize_fwd_kernel<long>), dim3(ew_grid(total)), dim3(256), 0, s, x, y, planes, ah, aw);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

template <typename T>
static int launch_adjoint(const T* src, long lda, int P, const float* std3, long planes, long src_elems, const ResizeAxis& ah,
                          const ResizeAxis& aw, float* gx, hipStream_t s) {
    const long total = planes * ah.in * aw.in;
    const bool small = total < (1L << 30) && src_elems < (1L << 30);
    const size_t lds = (size_t)(ah.out + aw.out) * (small ? sizeof(int) : sizeof(long));
    if (lds > 48 * 1024) return fail(RVLM_ERR_UNSUPPORTED, "resize adjoint: output sizes beyond the offset tables' 48 KiB of LDS");
    const float s0 = std3 ? std3[0] : 1.0f, s1 = std3 ? std3[1] : 1.0f, s2 = std3 ? std3[2] : 1.0f;
    if (small)
        hipLaunchKernelGGL((resize_adjoint_kernel<T, int>), dim3(ew_grid(total)), dim3(256), lds, s, src, lda, P, s0, s1, s2,
                           (int)planes, ah, aw, gx);
    else
        hipLaunchKernelGGL((resize_adjoint_kernel<T, long>), dim3(ew_grid(total)), dim3(256), lds, s, src, lda, P, s0, s1, s2,
                           planes, ah, aw, gx);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}

int resize_bicubic_adjoint(const float* gy, long planes, const ResizeAxis& ah, const ResizeAxis& aw, float* gx, hipStream_t s) {
    return launch_adjoint<float>(gy, 0, 0, nullptr, planes, planes * ah.out * aw.out, ah, aw, gx, s);
}

template <typename T>
int resize_im2col_normalize(const float* x, const float* delta, int B, const ResizeAxis& ah, const ResizeAxis& aw, int P,
                            const float* mean3, const float* std3, T* A0, long lda, int Kpad, hipStream_t s) {
    const long rows = (long)B * (ah.out / P) * (aw.out / P), total = rows * Kpad;
    const bool small = total < (1L << 30) && (long)B * 3 * ah.in * aw.in < (1L << 30) && rows * lda < (1L << 30);
    if (small)
        hipLaunchKernelGGL((resize_im2col_kernel<T, int>), dim3(ew_grid(total)), dim3(256), 0, s, x, delta, B, ah, aw, P, mean3[0],
                           mean3[1], mean3[2], std3[0], std3[1], std3[2], A0, lda, Kpad);
    else
        hipLaunchKernelGGL((resize_im2col_kernel<T, long>), dim3(ew_grid(total)), dim3(256), 0, s, x, delta, B, ah, aw, P, mean3[0],
                           mean3[1], mean3[2], std3[0], std3[1], std3[2], A0, lda, Kpad);
    RVLM_CHECK_LAUNCH();
    return RVLM_OK;
}
template int resize_im2col_normalize<float>(const float*, const float*, int, const ResizeAxis&, const ResizeAxis&, int, const float*,
                                            const float*, float*, long, int, hipStream_t);
template int resize_im2col_normalize<bf16_t>(const float*, const float*, int, const ResizeAxis&, const ResizeAxis&, int, const float*,
                                             const float*, bf16_t*, long, int, hipStream_t);

template <typename T>
int col2im_resize_grad(const T* dA0, long lda, int B, const ResizeAxis& ah, const ResizeAxis& aw, int P, const float* std3,
                       float* grad_x, hipStream_t s) {
    return launch_adjoint<T>(dA0, lda, P, std3, (long)B * 3, (long)B * (ah.out / P) * (aw.out / P) * lda, ah, aw, grad_x, s);
}
template int col2im_resize_grad<float>(const float*, long, int, const ResizeAxis&, const ResizeAxis&, int, const float*, float*,
                                       hipStream_t);
template int col2im_resize_grad<bf16_t>(const bf16_t*, long, int, const ResizeAxis&, const ResizeAxis&, int, const float*, float*,
                                        hipStream_t);

}  // namespace rvlm

using namespace rvlm;

extern "C" int rvlm_resize_taps(int in, int out, int32_t* idx, float* w) {
    RVLM_REQUIRE(idx && w, "rvlm_resize_taps: null argument");
    RVLM_REQUIRE(in >= 1 && out >= 1 && in <= (1 << 15) && out <= (1 << 15), "rvlm_resize_taps: sizes must be in 1..32768");
    resize_taps_host(in, out, idx, w);
    return RVLM_OK;
}

static int resize_args(const char* who, const void* a, const void* b, long planes, int in_h, int in_w, int out_h, int out_w,
                       ResizeAxis* ah, ResizeAxis* aw) {
    if (!a || !b || planes < 1) return fail(RVLM_ERR_ARG, std::string(who) + ": null argument or no planes");
    int rc;
    if ((rc = resize_axis_device(in_h, out_h, ah))) return rc;
    return resize_axis_device(in_w, out_w, aw);
}

extern "C" int rvlm_resize_bicubic(const float* x, long planes, int in_h, int in_w, int out_h, int out_w, float* y,
                                   rvlm_stream_t stream) {
    ResizeAxis ah, aw;
    int rc;
    if ((rc = resize_args("rvlm_resize_bicubic", x, y, planes, in_h, in_w, out_h, out_w, &ah, &aw))) return rc;
    return resize_bicubic_fwd(x, planes, ah, aw, y, (hipStream_t)stream);
}

extern "C" int rvlm_resize_bicubic_adjoint(const float* gy, long planes, int in_h, int in_w, int out_h, int out_w, float* gx,
                                           rvlm_stream_t stream) {
    ResizeAxis ah, aw;
    int rc;
    if ((rc = resize_args("rvlm_resize_bicubic_adjoint", gy, gx, planes, in_h, in_w, out_h, out_w, &ah, &aw))) return rc;
    return resize_bicubic_adjoint(gy, planes, ah, aw, gx, (hipStream_t)stream);
}
