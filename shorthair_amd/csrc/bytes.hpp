// Byte-level helpers shared by the packet kernels (frame, unframe, wire, rx_list, rx_group, rx_window,
// tx_datagram). Plain C++ behind SH_TXD_FN, so that tools/tx_copy_check.cpp and
// tools/rx_window_copy_check.cpp compile the same source for the CPU under a sanitizer.
#pragma once

#include <stdint.h>

#ifndef SH_TXD_FN
#define SH_TXD_FN __host__ __device__ __forceinline__
#endif

namespace sh {

typedef uint64_t u64x2 __attribute__((ext_vector_type(2)));

SH_TXD_FN uint64_t ld64(const uint8_t *p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);  // unaligned global_load_dwordx2
    return v;
}

// n (0..8) low bytes of v to dst, at any alignment: one 8-byte store, or 4 + 2 + 1.
SH_TXD_FN void store_bytes(uint8_t *dst, uint64_t v, int n) {
    if (n >= 8) {
        __builtin_memcpy(dst, &v, 8);  // unaligned global_store_dwordx2
        return;
    }
    if (n & 4) {
        const uint32_t t = static_cast<uint32_t>(v);
        __builtin_memcpy(dst, &t, 4);
        dst += 4;
        v >>= 32;
    }
    if (n & 2) {
        const uint16_t t = static_cast<uint16_t>(v);
        __builtin_memcpy(dst, &t, 2);
        dst += 2;
        v >>= 16;
    }
    if (n & 1) *dst = static_cast<uint8_t>(v);
}

// The ballot bits of the lanes below `lane` of a wave.
SH_TXD_FN uint64_t lanes_below(int lane) { return (1ull << lane) - 1; }

// Flat lane t of a grid that gives each item a sub-group of step = 1 << lshift lanes: lane `sub` of
// item `item`. 64-bit: items near INT_MAX times 32 lanes.
struct LaneSplit {
    long long item;
    int sub, step;
};
SH_TXD_FN LaneSplit lane_split(long long t, int lshift) {
    const int step = 1 << lshift;
    return LaneSplit{t >> lshift, static_cast<int>(t) & (step - 1), step};
}

// The lshift of items of `bytes` bytes: the power of two, 32 at most, of 16-byte pieces that covers them.
SH_TXD_FN int lshift_for(int bytes) {
    int lshift = 0;
    while (lshift < 5 && (16 << lshift) < bytes) ++lshift;
    return lshift;
}

}  // namespace sh
