// Device-side payload framing (csrc/frame.hip, include/shorthair_frame.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

// Block j of blocks[total_blocks][B] = "[len_j u16 LE][payload[off_j .. off_j + len_j)][zeros]", or
// the B bytes at off_j verbatim when raw && raw[j]; malformed blocks are zeros and counted in *errors.
// blocks is 8-byte aligned, B % 8 == 0. hipErrorInvalidValue (nothing launched) when the batch needs
// more workgroups than a grid holds.
hipError_t launch_frame(int B, int total_blocks, const uint8_t *payload, long long payload_bytes,
                        const long long *off, const int *len, const uint8_t *raw, uint8_t *blocks, int *errors,
                        hipStream_t stream);

}  // namespace sh
