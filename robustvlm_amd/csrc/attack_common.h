// What attack_kernels.hip and vlm_attack_kernels.hip both use (internal; both are built with -ffp-contract=off).
#pragma once
#include "common.h"

namespace rvlm {

__device__ __forceinline__ float sgnf(float a) {  // torch.sign: sign(+-0) = 0, sign(NaN) = 0
    return (a > 0.0f) ? 1.0f : ((a < 0.0f) ? -1.0f : 0.0f);
}
// sum over a workgroup of 1024 threads: wave shuffles, then the 16 wave partials in LDS added in wave order (a fixed order)
__device__ __forceinline__ float block_sum_1024(float v, float* red) {
    v = wave_sum(v);
    __syncthreads();                                   // red may still be read from the previous reduction
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) t += red[i];
    return t;
}
// flat grid of an elementwise kernel: 256 threads x per_thread elements per workgroup
static inline int ew_grid(size_t n, int per_thread = 4) {
    size_t blocks = (n / per_thread + 255) / 256;
    if (blocks < 1) blocks = 1;
    if (blocks > 256 * 8) blocks = 256 * 8;  // 256 CUs x 8 blocks, grid-stride the rest
    return (int)blocks;
}

}  // namespace rvlm
