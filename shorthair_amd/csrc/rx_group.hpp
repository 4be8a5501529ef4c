// Device-side grouping of received datagrams (csrc/rx_group.hip, include/shorthair_rx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sh {

// Bytes of scratch launch_rx_group needs: eight ints of header, a counter per slot, two ints per
// datagram and eight ints per tile of SHORTHAIR_RX_GROUP_TILE datagrams. > 0, non-decreasing in both
// arguments.
long long rx_group_scratch_bytes(long long datagrams, long long groups);

struct RxGroupArgs {
    const long long *dg_off;  // [datagrams]
    const int *dg_len;        // [datagrams]
    const uint8_t *ring;
    long long ring_bytes;
    const int *state_in;  // [1]
    int *state_out;       // [1], may alias state_in
    int *dg_class;        // [datagrams]
    int *dg_slot;         // [datagrams]
    int *pkt_first;       // [groups + 1]
    long long *pkt_off;   // [datagrams]
    int *pkt_len;         // [datagrams]
    int *pkt_dg;          // [datagrams]
    int *slot_group;      // [groups]
    int *other;           // [datagrams]
    int *summary;         // [8]
    int *errors;
    int *hdr;         // scratch [8]: [0] state_in[0], kept for the kernels after the one that writes state_out
    int *cnt;         // scratch [groups]: records per slot
    int *code;        // scratch [datagrams]: kind | pong << 4 | h << 8 | p << 16
    int *pos;         // scratch [datagrams]: a binned datagram's position in its slot as the counter gave it
    int *tile_fp;     // scratch [tiles]: the tile's step function: its first data partial, or -1 without one,
    int *tile_sum;    // scratch [tiles]: and the sum of the steps between its data datagrams
    int *tile_u;      // scratch [tiles]: the group number in front of the tile
    int *tile_nb;     // scratch [tiles]: datagrams of the tile that are not binned; then their exclusive sum
    int *tile_stat;   // scratch [tiles][4]: malformed, out of window, pong, short
    int datagrams, groups, back, tiles;
};

// The rule of shorthair_rx.h for `groups` > 0 slots: six kernels on `stream`. The scratch pointers of
// `a` and a.tiles are set here from `scratch`.
hipError_t launch_rx_group(RxGroupArgs a, void *scratch, hipStream_t stream);

}  // namespace sh
