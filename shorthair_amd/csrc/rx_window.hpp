// Device-side carry of open code groups between receive batches (csrc/rx_window.hip, include/shorthair_rx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

constexpr int RXW_MAX_INFO = 4;  // SHORTHAIR_RX_WINDOW_MAX_INFO

// Bytes of scratch launch_rx_window needs: a header, seven ints per slot and 40 bytes per workgroup of the
// per-slot pass; nothing per record. > 0, non-decreasing in both arguments.
long long rx_window_scratch_bytes(long long groups, long long capacity);

struct RxWindowArgs {
    // the previous window (has_prev) and the listings' d_info over it
    const int *p_base;            // [1]
    const int *p_first;           // [groups + 1]
    const long long *p_off;       // [p_cap]
    const int *p_len;             // [p_cap]
    const unsigned char *p_done;  // [groups]
    const int *info[RXW_MAX_INFO];
    // the group call's outputs
    const int *g_first;      // [groups + 1]
    const long long *g_off;  // [datagrams]
    const int *g_len;        // [datagrams]
    const int *g_dg;         // [datagrams]
    const int *g_slot_group; // [groups]
    uint8_t *ring;
    long long ring_bytes, hold_off, hold_bytes;
    // the next window
    int *n_base;
    int *n_first;
    long long *n_off;
    int *n_len;
    int *n_dg;
    unsigned char *n_done;
    long long *summary;  // [8]
    int *errors;
    // scratch
    int *cnt_c;          // [groups]: carried records of the slot
    int *cnt_n;          // [groups]: new records of the slot
    int *src_c;          // [groups]: the carried records' first index in the previous window
    int *src_n;          // [groups]: the new records' first index in the group call's lists
    int *flag;           // [groups]: the done code before the overflow cut
    long long *bytes;    // [groups]: the slot's carried bytes, each record rounded up; then their exclusive sum
    long long *wg_stat;  // [wgs][RXW_STATS]: newly finished, expired, ignored, below the window, malformed
    int groups, datagrams, p_cap, n_cap, n_info, wgs, lshift;
    bool has_prev, copy;
};

// The rule of shorthair_rx.h for `groups` > 0 slots: four kernels on `stream`. The scratch pointers of
// `a`, a.wgs and a.lshift are set here from `scratch`.
hipError_t launch_rx_window(RxWindowArgs a, void *scratch, hipStream_t stream);

}  // namespace sh
