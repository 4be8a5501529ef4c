// The copy of rxw_place (csrc/rx_window.hip): tx_datagram_copy.hpp's, unchanged, with a header of 0 bytes and
// the ring as the payload buffer. Plain C++, so that tools/rx_window_copy_check.cpp runs the same source on
// the CPU under a sanitizer.
//
// A carried record is `len` bytes at ring + off. A record of 8 bytes or more is read with 8-byte windows
// that stay inside the record; a shorter one with one window that covers it and stays inside
// [0, ring_bytes) -- it reaches up to 7 bytes past or before the record, and what it reaches outside is
// masked away -- or byte by byte when the whole ring is shorter than a window.
#pragma once

#include "tx_datagram_copy.hpp"

namespace sh {

SH_TXD_FN TxCopy rxw_copy_plan(const uint8_t *ring, long long ring_bytes, long long off, int len) {
    TxCopy c;
    c.h0 = 0;
    c.h1 = 0;
    c.buf = ring;
    c.src = off;
    c.end = len >= 8 ? off + len : ring_bytes;
    c.hlen = 0;
    c.blen = len;
    c.L = len;
    c.bytewise = len > 0 && c.end < 8;
    return c;
}

}  // namespace sh
