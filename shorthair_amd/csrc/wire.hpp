// Device-side wire records of recovery blocks (csrc/wire.hip, include/shorthair_wire.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

// Record p = g * m + y of wire[groups * m][3 + B] = "[k_g + y][k_g - 1][m - 1][recovery[g][y][0..B)]";
// k_g = k, or first[g + 1] - first[g] when first != nullptr (k is then kmax, and a group malformed by
// geometry.hpp's var_group rule gets m all-zero records). recovery is 8-byte aligned, wire takes any
// address, B % 8 == 0, groups * m <= INT_MAX. hipErrorInvalidValue (nothing launched) when the batch
// needs more workgroups than a grid holds.
hipError_t launch_wire_emit(int k, int m, int B, int groups, const int *first, int total_blocks,
                            const uint8_t *recovery, uint8_t *wire, hipStream_t stream);

}  // namespace sh
