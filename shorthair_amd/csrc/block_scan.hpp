// Workgroup-wide inclusive scan for the single-workgroup scan kernels (unframe.hip, rx_list.hip).
#pragma once

#include <hip/hip_runtime.h>

namespace sh {

// Inclusive scan over the workgroup's THREADS values (whole waves); `total` is their sum. wsum:
// THREADS / 64 entries of LDS, free to rewrite after the next __syncthreads().
template <int THREADS, class T>
__device__ __forceinline__ T block_scan(T v, T *wsum, T &total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    if (lane == 63) wsum[wave] = x;
    __syncthreads();
    T pre = 0;
    total = 0;
    for (int w = 0; w < THREADS / 64; ++w) {
        if (w < wave) pre += wsum[w];
        total += wsum[w];
    }
    return pre + x;
}

}  // namespace sh
