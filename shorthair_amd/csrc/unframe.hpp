// Device-side delivery of recovered blocks (csrc/unframe.hip, include/shorthair_unframe.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

// Bytes of scratch launch_unframe needs for `slots` slots: one 64-bit sum per tile of
// SHORTHAIR_UNFRAME_TILE_SLOTS slots and one more for the total, then one 32-bit in-tile offset per slot.
long long unframe_scratch_bytes(long long slots);

struct UnframeArgs {
    const uint8_t *out;
    const int *count;  // may be null
    uint8_t *payload;
    long long capacity;
    long long *off;
    int *len;
    int *errors;
    long long stride_blocks;
    int groups, emax, B;
    // set by launch_unframe
    long long *sums;  // scratch [tiles + 1]
    int *local;       // scratch [slots]
    int slots, tiles;
    int lshift;  // unframe_copy: 1 << lshift lanes per slot
};

// Slot s = g * emax + i reads the block at out + (g * stride_blocks + i) * B: len[s] = its u16 prefix
// p (p <= B - 2), -2 (p > B - 2) or -1 (i >= count[g]; count == nullptr: emax); off[s] = the exclusive
// 64-bit prefix sum of max(len, 0), off[groups * emax] the total; block bytes [2, 2 + p) go to payload
// + off[s] unless the span leaves [0, capacity) (counted in *errors, as a count outside -1..emax is,
// once per group). Three kernels on `stream`. groups > 0.
hipError_t launch_unframe(UnframeArgs a, void *scratch, hipStream_t stream);

}  // namespace sh
