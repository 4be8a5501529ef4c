// The copy of txd_copy (csrc/tx_datagram.hip), per lane, free of anything but plain C++ so that
// tools/tx_copy_check.cpp can run the same source on the CPU under a sanitizer.
//
// A datagram is `hlen` header bytes, held in the descriptor, and `blen` body bytes at `src` of the payload
// or the recovery buffer. It goes to dst = ring + offset, at any address. The lanes of a sub-group own the
// 16-byte pieces of the destination that are aligned to the *destination*: piece p covers datagram bytes
// [16p - a, 16p - a + 16), a = dst & 15. A piece is two 8-byte words; a word that holds body bytes is one
// unaligned 8-byte load of a window that covers them and stays inside the source -- inside the body itself
// when it has 8 bytes, else inside its buffer, pulled back from the buffer's end -- shifted, masked and
// joined with the header bytes that fall into it. A piece that lies wholly in the datagram is one aligned
// 16-byte store; the ragged piece at either end goes out word by word as 8/4/2/1-byte stores. A lane stores
// only bytes of its own datagram and reads none of the destination.
#pragma once

#include <stdint.h>

#include "bytes.hpp"

namespace sh {

// What the copy needs of one datagram: 32 bytes, read as two 16-byte loads.
struct TxDesc {
    uint64_t h0, h1;  // the header bytes (5, 6, 11 or 14 of them), zero behind the last
    long long src;    // the body's first byte, from the payload buffer or (TXD_REC) the recovery buffer
    int meta;         // body bytes | header bytes << 20 | TXD_REC
    int local;        // the datagram's offset within its tile
};
constexpr int TXD_REC = 1 << 24;
constexpr int TXD_HLEN_SHIFT = 20;
constexpr int TXD_BLEN_MASK = (1 << TXD_HLEN_SHIFT) - 1;

SH_TXD_FN int txd_min(int a, int b) { return a < b ? a : b; }
SH_TXD_FN int txd_max(int a, int b) { return a > b ? a : b; }

// One datagram as the copy sees it.
struct TxCopy {
    uint64_t h0, h1;
    const uint8_t *buf;  // the buffer the body lies in
    long long src;       // the body's first byte in buf
    long long end;       // loads stay below buf + end: the body's end when it has 8 bytes, else the buffer's
    int hlen, blen, L;
    bool bytewise;       // the buffer is shorter than one word: the body is read byte by byte
};

SH_TXD_FN TxCopy txd_plan(const TxDesc &d, const uint8_t *payload, long long payload_bytes,
                          const uint8_t *recovery) {
    TxCopy c;
    c.h0 = d.h0;
    c.h1 = d.h1;
    c.blen = d.meta & TXD_BLEN_MASK;
    c.hlen = (d.meta >> TXD_HLEN_SHIFT) & 15;
    c.L = c.hlen + c.blen;
    const bool rec = (d.meta & TXD_REC) != 0;  // a recovery block has at least 8 bytes
    c.buf = rec ? recovery : payload;
    c.src = d.src;
    c.end = c.blen >= 8 ? d.src + c.blen : payload_bytes;
    c.bytewise = c.blen > 0 && c.end < 8;
    return c;
}

// The body bytes a word takes: those of [b0, b0 + 8) that lie in [0, blen), b0 the body byte under byte 0
// of the word.
struct TxWord {
    long long ws;  // where the 8-byte window starts in buf
    int shr;       // bits to shift the window down
    int n;         // body bytes (0..8)
    int shl;       // bits to shift them up to their place in the word
};

SH_TXD_FN TxWord txd_word_plan(const TxCopy &c, int d0) {
    const int b0 = d0 - c.hlen;
    const int lo = txd_max(b0, 0);
    TxWord w;
    w.n = txd_max(txd_min(b0 + 8, c.blen) - lo, 0);
    w.shl = w.n > 0 ? 8 * (lo - b0) : 0;  // (n > 0: lo - b0 <= 7)
    const long long at = c.src + lo;
    const long long ws = at < c.end - 8 ? at : c.end - 8;
    w.ws = w.n > 0 ? ws : 0;
    w.shr = w.n > 0 ? 8 * static_cast<int>(at - ws) : 0;
    return w;
}

SH_TXD_FN uint64_t txd_load(const TxCopy &c, const TxWord &w, int d0) {
    uint64_t x = 0;
    if (w.n <= 0) return 0;  // (a word of header bytes only, or outside the datagram: nothing is read)
    if (c.bytewise) {
        const int lo = txd_max(d0 - c.hlen, 0);
        for (int i = 0; i < w.n; ++i) x |= static_cast<uint64_t>(c.buf[c.src + lo + i]) << (8 * i);
        return x;
    }
    __builtin_memcpy(&x, c.buf + w.ws, 8);  // unaligned global_load_dwordx2
    return x >> w.shr;
}

// Header bytes [d0, d0 + 8) as a word; the header is zero outside [0, hlen). -16 < d0.
SH_TXD_FN uint64_t txd_header_word(const TxCopy &c, int d0) {
    if (d0 >= 16 || d0 <= -8) return 0;
    if (d0 < 0) return c.h0 << (8 * -d0);
    if (d0 == 0) return c.h0;
    if (d0 < 8) return (c.h0 >> (8 * d0)) | (c.h1 << (64 - 8 * d0));
    return c.h1 >> (8 * (d0 - 8));
}

SH_TXD_FN uint64_t txd_finish(const TxCopy &c, const TxWord &w, uint64_t x, int d0) {
    const uint64_t mask = w.n >= 8 ? ~0ull : (1ull << (8 * w.n)) - 1;
    return ((x & mask) << w.shl) | txd_header_word(c, d0);
}

// The word over datagram bytes [d0, d0 + 8): those inside [0, L) go to dst + their index.
SH_TXD_FN void txd_emit_word(uint8_t *dst, const TxCopy &c, int d0, uint64_t v) {
    const int lo = txd_max(d0, 0);
    const int n = txd_min(d0 + 8, c.L) - lo;
    if (n > 0) store_bytes(dst + lo, v >> (8 * (lo - d0)), n);
}

// Piece p: d0 = 16p - a. Whole: one aligned 16-byte store.
SH_TXD_FN void txd_emit_piece(uint8_t *dst, const TxCopy &c, int d0, uint64_t v0, uint64_t v1) {
    if (d0 >= 0 && d0 + 16 <= c.L) {
        u64x2 o;
        o.x = v0;
        o.y = v1;
        *reinterpret_cast<u64x2 *>(dst + d0) = o;  // global_store_dwordx4
        return;
    }
    txd_emit_word(dst, c, d0, v0);
    txd_emit_word(dst, c, d0 + 8, v1);
}

// Lane `sub` of `step` lanes copies its pieces of the datagram to dst: two pieces in step -- the plans, then
// all four loads, then the splices and the stores -- so that no load waits for another's stores.
SH_TXD_FN void txd_copy_lane(const TxCopy &c, uint8_t *dst, int sub, int step) {
    if (c.L <= 0) return;
    const int a = static_cast<int>(reinterpret_cast<uintptr_t>(dst) & 15);
    const int pieces = (a + c.L + 15) >> 4;
    for (int p = sub; p < pieces; p += 2 * step) {
        const bool two = p + step < pieces;
        int d0[4];
        d0[0] = 16 * p - a;
        d0[1] = d0[0] + 8;
        d0[2] = 16 * (p + step) - a;
        d0[3] = d0[2] + 8;
        TxWord w[4];
        uint64_t x[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            w[i] = txd_word_plan(c, d0[i]);
            if (i >= 2 && !two) w[i].n = 0;
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = txd_load(c, w[i], d0[i]);
#pragma unroll
        for (int i = 0; i < 4; ++i) x[i] = txd_finish(c, w[i], x[i], d0[i]);
        txd_emit_piece(dst, c, d0[0], x[0], x[1]);
        if (two) txd_emit_piece(dst, c, d0[2], x[2], x[3]);
    }
}

}  // namespace sh
