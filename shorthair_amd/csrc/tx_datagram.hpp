// Device-side datagrams in send order (csrc/tx_datagram.hip, include/shorthair_tx.h).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shorthair_tx.h"
#include "tx_datagram_copy.hpp"

namespace sh {

// Bytes of scratch launch_tx_datagram needs: a TxDesc per datagram, a 64-bit sum and six class counts per
// tile of SHORTHAIR_TX_TILE datagrams, and one more sum. > 0, non-decreasing.
long long tx_datagram_scratch_bytes(long long datagrams);

struct TxDatagramArgs {
    const int *sched;                   // [datagrams]
    const int *first;                   // [groups + 1]
    const uint8_t *payload;
    long long payload_bytes;
    const long long *off;               // [total]
    const int *len;                     // [total]
    const uint8_t *recovery;
    long long recovery_bytes;
    const ShorthairTxGroupDesc *group;  // [groups] or null
    const int *pong_at;                 // [n_pong]
    const unsigned *pong_val;           // [2 * n_pong]
    const int *state_in;                // [2]
    int *state_out;                     // [2], may alias state_in
    uint8_t *ring;
    long long ring_bytes;
    long long *dg_off;                  // [datagrams + 1]
    int *dg_len;                        // [datagrams]
    int *dg_class;                      // [datagrams]
    int *summary;                       // [8]
    int *errors;
    TxDesc *desc;                       // scratch [datagrams]
    long long *sums;                    // scratch [tiles + 1]: tile sums, then tile bases and the total
    int *tile_stat;                     // scratch [tiles][6]: written, originals, recovery, holes, pong, malformed
    int datagrams, groups, m, B, total, n_pong, advance, align, tiles;
    int lshift;                         // txd_copy: 1 << lshift lanes per datagram
};

// The rule of shorthair_tx.h: three kernels on `stream` (one when datagrams == 0). The scratch pointers,
// a.tiles and a.lshift are set here.
hipError_t launch_tx_datagram(TxDatagramArgs a, void *scratch, hipStream_t stream);

}  // namespace sh
