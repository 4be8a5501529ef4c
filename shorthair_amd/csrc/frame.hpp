// Device-side payload framing (csrc/frame.hip, include/shorthair_frame.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

struct FrameArgs {
    const uint8_t *payload;
    long long payload_bytes;
    const long long *off;
    const int *len;
    const uint8_t *raw;  // may be null
    uint8_t *blocks;
    int *errors;
    int B, total_blocks;
    // set by launch_frame
    long long total_words;  // total_blocks * nw
    int nw;                 // B / 8
    int head;               // 1: blocks is 8- but not 16-aligned, pairs start at word -1
    uint32_t mul;           // floor(2^32 / nw) + 1 for 2 <= nw <= FRAME_MUL_NW (x / nw = umulhi(x, mul),
                            // exact for x < 2^13), else 0
};

// Block j of blocks[total_blocks][B] = "[len_j u16 LE][payload[off_j .. off_j + len_j)][zeros]", or
// the B bytes at off_j verbatim when raw && raw[j]; malformed blocks are zeros and counted in *errors.
// blocks is 8-byte aligned, B % 8 == 0. hipErrorInvalidValue (nothing launched) when the batch needs
// more workgroups than a grid holds.
hipError_t launch_frame(FrameArgs a, hipStream_t stream);

}  // namespace sh
