// Workgroup-wide scan, and the pass loop of the single-workgroup scan kernels, for the packet calls:
// block_scan alone in unframe_lengths, txd_lengths, rxg_classify, rxg_down, rxg_scatter and rxw_scan;
// scan_passes in unframe_scan, txd_scan, rx_scan, rxg_scan_tiles and rxg_scan_slots.
#pragma once

#include <hip/hip_runtime.h>

namespace sh {

struct ScanAdd {
    template <class T>
    __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};

template <class T>
struct Scanned {
    T incl, excl, total;  // this lane's inclusive and exclusive prefix, and the workgroup's aggregate
};

// x of the lane d below, dword by dword (the lowest d lanes of a wave get their own x back).
template <class T>
__device__ __forceinline__ T scan_shfl_up(T x, int d) {
    static_assert(sizeof(T) % 4 == 0, "whole dwords");
    int w[sizeof(T) / 4];
    __builtin_memcpy(w, &x, sizeof(T));
#pragma unroll
    for (unsigned i = 0; i < sizeof(T) / 4; ++i) w[i] = __shfl_up(w[i], d);
    __builtin_memcpy(&x, w, sizeof(T));
    return x;
}

// Scan of the workgroup's THREADS values (whole waves) in lane order under the associative `op` --
// op(lower lanes, higher lanes); it need not commute -- with `identity` in front of lane 0. lds:
// THREADS / 64 entries, free to rewrite after the next __syncthreads().
template <int THREADS, class T, class Op = ScanAdd>
__device__ __forceinline__ Scanned<T> block_scan(T v, T *lds, T identity = T{}, Op op = Op{}) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    T x = v;
    for (int d = 1; d < 64; d <<= 1) {
        const T y = scan_shfl_up(x, d);
        if (lane >= d) x = op(y, x);
    }
    T prev = scan_shfl_up(x, 1);
    if (lane == 0) prev = identity;
    if (lane == 63) lds[wave] = x;
    __syncthreads();
    T pre = identity, total = identity;
    for (int w = 0; w < THREADS / 64; ++w) {
        if (w < wave) pre = op(pre, lds[w]);
        total = op(total, lds[w]);
    }
    return Scanned<T>{op(pre, x), op(pre, prev), total};
}

// Exclusive scan of n items by one workgroup, THREADS * PER of them per pass: a lane takes PER
// consecutive items, the workgroup scans the lanes' aggregates, and a carry runs from pass to pass.
// load(i) gives item i; store(i, prefix, item) receives the aggregate of items [0, i) and item i again.
// Both are called for 0 <= i < n only, with a 64-bit i (n may lie near INT_MAX); a lane's places past
// the end hold the identity. Returns the aggregate of all n items. lds: THREADS / 64 entries.
template <int THREADS, int PER, class T, class Load, class Store, class Op = ScanAdd>
__device__ __forceinline__ T scan_passes(long long n, T *lds, Load load, Store store, T identity = T{}, Op op = Op{}) {
    T carry = identity;
    for (long long base = 0; base < n; base += static_cast<long long>(THREADS) * PER) {
        const long long i0 = base + static_cast<long long>(threadIdx.x) * PER;
        T item[PER], mine = identity;
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            item[j] = i0 + j < n ? load(i0 + j) : identity;
            mine = op(mine, item[j]);
        }
        const Scanned<T> s = block_scan<THREADS>(mine, lds, identity, op);
        T at = op(carry, s.excl);
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            if (i0 + j < n) store(i0 + j, at, item[j]);
            at = op(at, item[j]);
        }
        carry = op(carry, s.total);
        __syncthreads();  // lds is rewritten by the next pass
    }
    return carry;
}

}  // namespace sh
