// Device-side listing of received packets (csrc/rx_list.hip, include/shorthair_rx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

// Bytes of scratch launch_rx_list needs: a status/k code and a list base per group, then two bytes
// (id, class) per record. > 0, non-decreasing in both arguments.
long long rx_list_scratch_bytes(long long groups, long long packets);

struct RxListArgs {
    const int *pkt_first;      // [groups + 1]
    const long long *pkt_off;  // [packets]
    const int *pkt_len;        // [packets]
    const uint8_t *ring;
    long long ring_bytes;
    int *info;        // [groups][SHORTHAIR_RX_INFO_INTS]
    int *first;       // [groups + 1]
    int *slot_group;  // [groups]
    long long *off;   // the four lists: [capacity]
    int *len;
    uint8_t *raw, *rows;
    int *summary;  // [8]
    int *errors;
    int *code;      // scratch [groups]: (k << 8) | (status + 1)
    int *base;      // scratch [groups]: d_first of a listed group's slot, else -1
    uint16_t *rec;  // scratch [packets]: id | (recovery << 8)
    int kmin, kmax, m, B, groups, packets, capacity;
};

// The rule of shorthair_rx.h for `groups` > 0 groups: three kernels on `stream`. The scratch pointers
// of `a` are set here from `scratch`.
hipError_t launch_rx_list(RxListArgs a, void *scratch, hipStream_t stream);

}  // namespace sh
