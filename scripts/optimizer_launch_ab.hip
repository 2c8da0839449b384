// A/B of launch shapes for the optimizer streams (not part of the library): the SGD-with-momentum update as
// 16-byte and scalar grid-stride kernels under block caps from 1024 up to one item per thread, with two groups per iteration, with
// non-temporal accesses and with one contiguous slab per block, next to a copy of the AdamW kernel and a float4 copy.
// n = FlatParams(ViT-L/14).numel fp32 elements, zero-filled buffers, HIP events, all variants interleaved, median of 15 after 3.
//     hipcc -O3 -std=c++17 -ffp-contract=off --offload-arch=gfx950 scripts/optimizer_launch_ab.hip -o optimizer_launch_ab
//     ./optimizer_launch_ab > profiles/optimizer_launch_ab.log
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <functional>
#include <string>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); exit(2); } } while (0)

__device__ __forceinline__ void sgd_elem(float& p, float g, float& buf, float lr_neg, float mom, float wd, float gs) {
    float d = fmaf(wd, p, g * gs);
    d = mom * buf + d;
    buf = d;
    p = fmaf(lr_neg, d, p);
}
template <bool NT> __device__ __forceinline__ float4 ld4(const float4* a) {
    if (NT) { float4 r; r.x = __builtin_nontemporal_load(&a->x); r.y = __builtin_nontemporal_load(&a->y); r.z = __builtin_nontemporal_load(&a->z); r.w = __builtin_nontemporal_load(&a->w); return r; }
    return *a;
}
template <bool NT> __device__ __forceinline__ void st4(float4* a, float4 v) {
    if (NT) { __builtin_nontemporal_store(v.x, &a->x); __builtin_nontemporal_store(v.y, &a->y); __builtin_nontemporal_store(v.z, &a->z); __builtin_nontemporal_store(v.w, &a->w); }
    else *a = v;
}
template <bool NT, int U>
__global__ void __launch_bounds__(256)
sgd_v(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, size_t nvec, float lr_neg, float mom, float wd, float gs) {
    const size_t tid = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
    float4* p4 = (float4*)p; const float4* g4 = (const float4*)g; float4* b4 = (float4*)buf;
    for (size_t i = tid; i < nvec; i += stride * U) {
        float4 pv[U], gv[U], bv[U];
#pragma unroll
        for (int u = 0; u < U; ++u) { size_t j = i + u * stride; if (j < nvec) { pv[u] = ld4<NT>(p4 + j); gv[u] = ld4<NT>(g4 + j); bv[u] = ld4<NT>(b4 + j); } }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            size_t j = i + u * stride;
            if (j < nvec) {
                sgd_elem(pv[u].x, gv[u].x, bv[u].x, lr_neg, mom, wd, gs); sgd_elem(pv[u].y, gv[u].y, bv[u].y, lr_neg, mom, wd, gs);
                sgd_elem(pv[u].z, gv[u].z, bv[u].z, lr_neg, mom, wd, gs); sgd_elem(pv[u].w, gv[u].w, bv[u].w, lr_neg, mom, wd, gs);
                st4<NT>(p4 + j, pv[u]); st4<NT>(b4 + j, bv[u]);
            }
        }
    }
}
// block-contiguous: each block walks its own contiguous slab
__global__ void __launch_bounds__(256)
sgd_slab(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, size_t nvec, float lr_neg, float mom, float wd, float gs) {
    const size_t per = (nvec + gridDim.x - 1) / gridDim.x, lo = per * blockIdx.x, hi = lo + per < nvec ? lo + per : nvec;
    float4* p4 = (float4*)p; const float4* g4 = (const float4*)g; float4* b4 = (float4*)buf;
    for (size_t i = lo + threadIdx.x; i < hi; i += 256) {
        float4 pv = p4[i], gv = g4[i], bv = b4[i];
        sgd_elem(pv.x, gv.x, bv.x, lr_neg, mom, wd, gs); sgd_elem(pv.y, gv.y, bv.y, lr_neg, mom, wd, gs);
        sgd_elem(pv.z, gv.z, bv.z, lr_neg, mom, wd, gs); sgd_elem(pv.w, gv.w, bv.w, lr_neg, mom, wd, gs);
        p4[i] = pv; b4[i] = bv;
    }
}
__global__ void __launch_bounds__(256)
sgd_s(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf, size_t n, float lr_neg, float mom, float wd, float gs) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float pi = p[i], bi = buf[i];
        sgd_elem(pi, g[i], bi, lr_neg, mom, wd, gs);
        p[i] = pi; buf[i] = bi;
    }
}
__global__ void __launch_bounds__(256)
adamw_s(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n, float decay, float w1,
        float b2, float w2, float eps, float step_size, float bc2_sqrt, float gs) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float gi = g[i] * gs;
        float pi = p[i] * decay;
        const float mi = m[i] + (gi - m[i]) * w1;
        const float vi = b2 * v[i] + w2 * gi * gi;
        pi = pi - step_size * (mi / (sqrtf(vi) / bc2_sqrt + eps));
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
}
__global__ void __launch_bounds__(256) copy_v(float4* __restrict__ d, const float4* __restrict__ s, size_t nvec) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (size_t)gridDim.x * blockDim.x) d[i] = s[i];
}

int main() {
    const size_t n = 303966208, nvec = n / 4;
    float *p, *g, *b, *m, *v;
    CK(hipMalloc(&p, n * 4)); CK(hipMalloc(&g, n * 4)); CK(hipMalloc(&b, n * 4)); CK(hipMalloc(&m, n * 4)); CK(hipMalloc(&v, n * 4));
    CK(hipMemset(p, 0, n * 4)); CK(hipMemset(g, 0, n * 4)); CK(hipMemset(b, 0, n * 4)); CK(hipMemset(m, 0, n * 4)); CK(hipMemset(v, 0, n * 4));
    const float lr = -1e-5f, mom = 0.9f, wd = 1e-4f;
    struct V { std::string name; double bytes; std::function<void()> fn; std::vector<float> ms; };
    std::vector<V> vs;
    auto add = [&](std::string nm, double by, std::function<void()> f) { vs.push_back({nm, by, f, {}}); };
    for (int grid : {1024, 2048, 4096, 8192, 16384, 32768, 65536, 131072, 262144, 296842})
        add("sgd_v U1 grid " + std::to_string(grid), 20.0 * n, [=] { hipLaunchKernelGGL((sgd_v<false, 1>), dim3(grid), dim3(256), 0, 0, p, g, b, nvec, lr, mom, wd, 1.f); });
    for (int grid : {2048, 4096, 148421})
        add("sgd_v U2 grid " + std::to_string(grid), 20.0 * n, [=] { hipLaunchKernelGGL((sgd_v<false, 2>), dim3(grid), dim3(256), 0, 0, p, g, b, nvec, lr, mom, wd, 1.f); });
    add("sgd_v NT U1 grid 4096", 20.0 * n, [=] { hipLaunchKernelGGL((sgd_v<true, 1>), dim3(4096), dim3(256), 0, 0, p, g, b, nvec, lr, mom, wd, 1.f); });
    add("sgd_slab grid 2048", 20.0 * n, [=] { hipLaunchKernelGGL(sgd_slab, dim3(2048), dim3(256), 0, 0, p, g, b, nvec, lr, mom, wd, 1.f); });
    add("sgd_slab grid 16384", 20.0 * n, [=] { hipLaunchKernelGGL(sgd_slab, dim3(16384), dim3(256), 0, 0, p, g, b, nvec, lr, mom, wd, 1.f); });
    add("sgd_s grid 4096", 20.0 * n, [=] { hipLaunchKernelGGL(sgd_s, dim3(4096), dim3(256), 0, 0, p, g, b, n, lr, mom, wd, 1.f); });
    add("sgd_s grid full", 20.0 * n, [=] { hipLaunchKernelGGL(sgd_s, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, p, g, b, n, lr, mom, wd, 1.f); });
    add("sgd_s grid 65536", 20.0 * n, [=] { hipLaunchKernelGGL(sgd_s, dim3(65536), dim3(256), 0, 0, p, g, b, n, lr, mom, wd, 1.f); });
    add("adamw_s grid 4096", 28.0 * n, [=] { hipLaunchKernelGGL(adamw_s, dim3(4096), dim3(256), 0, 0, p, g, m, v, n, 0.999f, 0.1f, 0.999f, 0.001f, 1e-8f, 1e-5f, 0.5f, 1.f); });
    add("adamw_s grid full", 28.0 * n, [=] { hipLaunchKernelGGL(adamw_s, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, p, g, m, v, n, 0.999f, 0.1f, 0.999f, 0.001f, 1e-8f, 1e-5f, 0.5f, 1.f); });
    add("copy_v grid 4096", 8.0 * n, [=] { hipLaunchKernelGGL(copy_v, dim3(4096), dim3(256), 0, 0, (float4*)m, (const float4*)g, nvec); });
    add("copy_v grid full", 8.0 * n, [=] { hipLaunchKernelGGL(copy_v, dim3(296842), dim3(256), 0, 0, (float4*)m, (const float4*)g, nvec); });
    hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int it = 0; it < 3 + 15; ++it)
        for (auto& x : vs) {
            CK(hipEventRecord(e0, 0)); x.fn(); CK(hipEventRecord(e1, 0)); CK(hipEventSynchronize(e1)); CK(hipGetLastError());
            float ms; CK(hipEventElapsedTime(&ms, e0, e1));
            if (it >= 3) x.ms.push_back(ms);
        }
    for (auto& x : vs) {
        std::sort(x.ms.begin(), x.ms.end());
        const float med = x.ms[x.ms.size() / 2];
        printf("%-26s median %.4f ms  min %.4f  max %.4f  %.3f TB/s\n", x.name.c_str(), med, x.ms.front(), x.ms.back(), x.bytes / (med * 1e-3) / 1e12);
    }
    return 0;
}
