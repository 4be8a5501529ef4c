// Device-side wire records of recovery blocks (csrc/wire.hip, include/shorthair_wire.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

struct WireArgs {
    const uint8_t *rec;
    uint8_t *wire;
    const int *first;  // null: every group has k originals
    int B, m, k, groups, total;
    // set by launch_wire_emit
    long long run;  // groups * m * S: bytes written
    long long src;  // groups * m * B: bytes of rec
    int S;          // 3 + B
    int head;       // wire & 15: the run starts `head` bytes into workgroup 0's first piece
    uint32_t mul_s;  // floor(2^32 / S) + 1 for S <= WIRE_MUL_S (x / S = umulhi(x, mul_s), exact for
                     // x < S + WIRE_BYTES as (S + WIRE_BYTES) * S < 2^32), else 0
    uint32_t mul_m;  // floor(2^32 / m) + 1 for m >= 2 (exact for x < 2^32 / m; x < m + 375 here)
};

// Record p = g * m + y of wire[groups * m][3 + B] = "[k_g + y][k_g - 1][m - 1][rec[g][y][0..B)]";
// k_g = k, or first[g + 1] - first[g] when first != nullptr (k is then kmax, `total` the blocks first[]
// spans, and a group malformed by geometry.hpp's var_group rule gets m all-zero records). rec is 8-byte
// aligned, wire takes any address, B % 8 == 0, groups * m <= INT_MAX. hipErrorInvalidValue (nothing
// launched) when the batch needs more workgroups than a grid holds.
hipError_t launch_wire_emit(WireArgs a, hipStream_t stream);

}  // namespace sh
