// Host side of the packet calls (include/shorthair_frame.h, shorthair_unframe.h, shorthair_wire.h,
// shorthair_rx.h, shorthair_tx.h): their size queries, which touch no GPU, and the seven batch entry points.
//
// An entry point checks its arguments -- every -1 comes before the GPU is touched -- takes a StreamCall
// (csrc/stream_call.hpp), fills the launcher's argument struct in declaration order and launches. The
// launcher (csrc/<call>.hip) derives the rest of the struct: scratch pointers, tile counts, lane shifts.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <cstdio>

#include "../../include/shorthair_frame.h"
#include "../../include/shorthair_rx.h"
#include "../../include/shorthair_tx.h"
#include "../../include/shorthair_unframe.h"
#include "../../include/shorthair_wire.h"
#include "frame.hpp"
#include "rx_group.hpp"
#include "rx_list.hpp"
#include "rx_window.hpp"
#include "stream_call.hpp"
#include "tx_datagram.hpp"
#include "unframe.hpp"
#include "wire.hpp"

namespace {

// p is not a multiple of `align` (null is aligned).
bool mis(const void *p, unsigned align) { return reinterpret_cast<uintptr_t>(p) % align != 0; }

// What an entry point returns after its launch: 0, or -2 with the error on stderr.
int launched(hipError_t e, const char *what) {
    if (e == hipSuccess) return 0;
    std::fprintf(stderr, "libcauchy256: %s failed: %s\n", what, hipGetErrorString(e));
    return -2;
}

}  // namespace

extern "C" int shorthair_frame_batch(int block_bytes, int total_blocks, const void *d_payload,
                                     long long payload_bytes, const long long *d_off, const int *d_len,
                                     const unsigned char *d_raw, void *d_blocks, void *stream) {
    if (block_bytes < 8 || block_bytes % 8 != 0 || total_blocks < 0 || payload_bytes < 0) return -1;
    if (total_blocks > 0 && (!d_payload || !d_off || !d_len || !d_blocks)) return -1;
    if (mis(d_blocks, 8)) return -1;
    if (total_blocks == 0) return 0;
    sh::StreamCall call(stream);
    if (call.rc) return call.rc;
    const sh::FrameArgs a{.payload = static_cast<const uint8_t *>(d_payload),
                          .payload_bytes = payload_bytes,
                          .off = d_off,
                          .len = d_len,
                          .raw = d_raw,
                          .blocks = static_cast<uint8_t *>(d_blocks),
                          .errors = call.errors,
                          .B = block_bytes,
                          .total_blocks = total_blocks};
    return launched(sh::launch_frame(a, call.stream), "shorthair_frame_batch");
}

extern "C" long long shorthair_unframe_scratch_bytes(int groups, int emax) {
    if (groups < 0 || emax < 1 || emax > 255) return -1;
    const long long slots = static_cast<long long>(groups) * emax;
    if (slots > 0x7fffffffll) return -1;
    return sh::unframe_scratch_bytes(slots);
}

extern "C" int shorthair_unframe_batch(int block_bytes, int groups, int emax, long long group_stride_blocks,
                                       const void *d_out, const int *d_out_count, void *d_payload,
                                       long long payload_capacity, long long *d_off, int *d_len, void *d_scratch,
                                       void *stream) {
    if (block_bytes < 8 || block_bytes % 8 != 0 || groups < 0 || emax < 1 || emax > 255) return -1;
    if (static_cast<long long>(groups) * emax > 0x7fffffffll) return -1;
    if (group_stride_blocks < emax || payload_capacity < 0) return -1;
    if (mis(d_out, 8) || mis(d_off, 8) || mis(d_len, 4) || mis(d_scratch, 8)) return -1;
    if (groups > 0 && (!d_out || !d_off || !d_len || !d_scratch || (payload_capacity > 0 && !d_payload))) return -1;
    if (groups == 0) return 0;
    sh::StreamCall call(stream);
    if (call.rc) return call.rc;
    const sh::UnframeArgs a{.out = static_cast<const uint8_t *>(d_out),
                            .count = d_out_count,
                            .payload = static_cast<uint8_t *>(d_payload),
                            .capacity = payload_capacity,
                            .off = d_off,
                            .len = d_len,
                            .errors = call.errors,
                            .stride_blocks = group_stride_blocks,
                            .groups = groups,
                            .emax = emax,
                            .B = block_bytes};
    return launched(sh::launch_unframe(a, d_scratch, call.stream), "shorthair_unframe_batch");
}

extern "C" int shorthair_wire_emit_batch(int k, int m, int block_bytes, int groups, const int *d_first,
                                         int total_blocks, const void *d_recovery, void *d_wire, void *stream) {
    if (k < 2 || k > 255 || m < 1 || k + m > 256 || block_bytes < 8 || block_bytes % 8 != 0 || groups < 0) return -1;
    if (static_cast<long long>(groups) * m > 0x7fffffffll) return -1;
    if (d_first && (total_blocks < 0 || static_cast<long long>(total_blocks) > static_cast<long long>(groups) * k ||
                    mis(d_first, 4)))
        return -1;
    if (groups > 0 && (!d_recovery || !d_wire)) return -1;
    if (mis(d_recovery, 8)) return -1;
    if (groups == 0) return 0;
    sh::StreamCall call(stream, /*counts=*/false);  // (nothing is counted: no stream state, no lock)
    if (call.rc) return call.rc;
    const sh::WireArgs a{.rec = static_cast<const uint8_t *>(d_recovery),
                         .wire = static_cast<uint8_t *>(d_wire),
                         .first = d_first,
                         .B = block_bytes,
                         .m = m,
                         .k = k,
                         .groups = groups,
                         .total = total_blocks};
    return launched(sh::launch_wire_emit(a, call.stream), "shorthair_wire_emit_batch");
}

extern "C" int shorthair_rx_list_capacity(int groups, int packets, int kmax) {
    if (groups < 0 || packets < 0 || kmax < 2 || kmax > 255) return -1;
    return static_cast<int>(std::min<long long>(packets, static_cast<long long>(groups) * kmax));
}

extern "C" long long shorthair_rx_list_scratch_bytes(int groups, int packets) {
    if (groups < 0 || packets < 0) return -1;
    return sh::rx_list_scratch_bytes(groups, packets);
}

extern "C" int shorthair_rx_list_batch(int kmin, int kmax, int m, int block_bytes, int groups, int packets,
                                       const int *d_pkt_first, const long long *d_pkt_off, const int *d_pkt_len,
                                       const void *d_ring, long long ring_bytes, int *d_info, int *d_first,
                                       int *d_slot_group, long long *d_off, int *d_len, unsigned char *d_raw,
                                       unsigned char *d_rows, int *d_summary, void *d_scratch, void *stream) {
    if (kmin < 2 || kmin > kmax || kmax > 255 || m < 1 || kmax + m > 256) return -1;
    if (block_bytes < 8 || block_bytes % 8 != 0 || groups < 0 || packets < 0 || ring_bytes < 0) return -1;
    if (mis(d_pkt_first, 4) || mis(d_pkt_len, 4) || mis(d_info, 4) || mis(d_first, 4) || mis(d_slot_group, 4) ||
        mis(d_len, 4) || mis(d_summary, 4) || mis(d_pkt_off, 8) || mis(d_off, 8) || mis(d_scratch, 8))
        return -1;
    const int capacity = shorthair_rx_list_capacity(groups, packets, kmax);
    if (groups > 0) {
        if (!d_pkt_first || !d_info || !d_first || !d_slot_group || !d_summary || !d_scratch) return -1;
        if (packets > 0 && (!d_pkt_off || !d_pkt_len || !d_ring)) return -1;
        if (capacity > 0 && (!d_off || !d_len || !d_raw || !d_rows)) return -1;
    }
    if (groups == 0) return 0;
    sh::StreamCall call(stream);
    if (call.rc) return call.rc;
    const sh::RxListArgs a{.pkt_first = d_pkt_first,
                           .pkt_off = d_pkt_off,
                           .pkt_len = d_pkt_len,
                           .ring = static_cast<const uint8_t *>(d_ring),
                           .ring_bytes = ring_bytes,
                           .info = d_info,
                           .first = d_first,
                           .slot_group = d_slot_group,
                           .off = d_off,
                           .len = d_len,
                           .raw = d_raw,
                           .rows = d_rows,
                           .summary = d_summary,
                           .errors = call.errors,
                           .kmin = kmin,
                           .kmax = kmax,
                           .m = m,
                           .B = block_bytes,
                           .groups = groups,
                           .packets = packets,
                           .capacity = capacity};
    return launched(sh::launch_rx_list(a, d_scratch, call.stream), "shorthair_rx_list_batch");
}

extern "C" long long shorthair_rx_group_scratch_bytes(int datagrams, int groups) {
    if (datagrams < 0 || groups < 0) return -1;
    return sh::rx_group_scratch_bytes(datagrams, groups);
}

extern "C" int shorthair_rx_group_batch(int datagrams, int groups, int back, const long long *d_dg_off,
                                        const int *d_dg_len, const void *d_ring, long long ring_bytes,
                                        const int *d_state_in, int *d_state_out, int *d_dg_class, int *d_dg_slot,
                                        int *d_pkt_first, long long *d_pkt_off, int *d_pkt_len, int *d_pkt_dg,
                                        int *d_slot_group, int *d_other, int *d_summary, void *d_scratch,
                                        void *stream) {
    if (datagrams < 0 || groups < 0 || back < 0 || back > groups || ring_bytes < 0) return -1;
    if (mis(d_dg_len, 4) || mis(d_state_in, 4) || mis(d_state_out, 4) || mis(d_dg_class, 4) || mis(d_dg_slot, 4) ||
        mis(d_pkt_first, 4) || mis(d_pkt_len, 4) || mis(d_pkt_dg, 4) || mis(d_slot_group, 4) || mis(d_other, 4) ||
        mis(d_summary, 4) || mis(d_dg_off, 8) || mis(d_pkt_off, 8) || mis(d_scratch, 8))
        return -1;
    if (groups > 0) {
        if (!d_state_in || !d_state_out || !d_pkt_first || !d_slot_group || !d_summary || !d_scratch) return -1;
        if (datagrams > 0 && (!d_dg_off || !d_dg_len || !d_ring || !d_dg_class || !d_dg_slot || !d_pkt_off ||
                              !d_pkt_len || !d_pkt_dg || !d_other))
            return -1;
    }
    if (groups == 0) return 0;
    sh::StreamCall call(stream);
    if (call.rc) return call.rc;
    const sh::RxGroupArgs a{.dg_off = d_dg_off,
                            .dg_len = d_dg_len,
                            .ring = static_cast<const uint8_t *>(d_ring),
                            .ring_bytes = ring_bytes,
                            .state_in = d_state_in,
                            .state_out = d_state_out,
                            .dg_class = d_dg_class,
                            .dg_slot = d_dg_slot,
                            .pkt_first = d_pkt_first,
                            .pkt_off = d_pkt_off,
                            .pkt_len = d_pkt_len,
                            .pkt_dg = d_pkt_dg,
                            .slot_group = d_slot_group,
                            .other = d_other,
                            .summary = d_summary,
                            .errors = call.errors,
                            .datagrams = datagrams,
                            .groups = groups,
                            .back = back};
    return launched(sh::launch_rx_group(a, d_scratch, call.stream), "shorthair_rx_group_batch");
}

extern "C" long long shorthair_rx_window_scratch_bytes(int groups, int capacity) {
    if (groups < 0 || capacity < 0) return -1;
    return sh::rx_window_scratch_bytes(groups, capacity);
}

extern "C" int shorthair_rx_window_batch(int groups, const ShorthairRxWindow *prev, int n_info,
                                         const int *const *d_info, int datagrams, const int *d_pkt_first,
                                         const long long *d_pkt_off, const int *d_pkt_len, const int *d_pkt_dg,
                                         const int *d_slot_group, void *d_ring, long long ring_bytes,
                                         long long hold_off, long long hold_bytes, const ShorthairRxWindow *next,
                                         long long *d_summary, void *d_scratch, void *stream) {
    if (groups < 0 || datagrams < 0 || !next || next->capacity < 0 || (prev && prev->capacity < 0)) return -1;
    if (n_info < 0 || n_info > SHORTHAIR_RX_WINDOW_MAX_INFO || (!prev && n_info != 0) || (n_info > 0 && !d_info)) return -1;
    if (ring_bytes < 0 || hold_off < 0 || hold_bytes < 0 || hold_off > ring_bytes - hold_bytes) return -1;
    for (const ShorthairRxWindow *w : {prev, next}) {
        if (!w) continue;
        if (mis(w->base, 4) || mis(w->first, 4) || mis(w->len, 4) || mis(w->dg, 4) || mis(w->off, 8)) return -1;
        if (groups > 0 && (!w->base || !w->first || !w->done)) return -1;
        if (groups > 0 && w->capacity > 0 && (!w->off || !w->len || !w->dg)) return -1;
    }
    for (int q = 0; q < n_info; ++q)
        if (mis(d_info[q], 4) || (groups > 0 && !d_info[q])) return -1;
    if (mis(d_pkt_first, 4) || mis(d_pkt_len, 4) || mis(d_pkt_dg, 4) || mis(d_slot_group, 4) || mis(d_pkt_off, 8) ||
        mis(d_summary, 8) || mis(d_scratch, 8))
        return -1;
    if (groups > 0) {
        if (!d_pkt_first || !d_slot_group || !d_summary || !d_scratch) return -1;
        if (datagrams > 0 && (!d_pkt_off || !d_pkt_len || !d_pkt_dg)) return -1;
        if (ring_bytes > 0 && !d_ring) return -1;
    }
    if (prev) {  // the two windows share no array
        const void *a[6] = {prev->base, prev->first, prev->off, prev->len, prev->dg, prev->done};
        const void *b[6] = {next->base, next->first, next->off, next->len, next->dg, next->done};
        for (const void *x : a)
            for (const void *y : b)
                if (x && x == y) return -1;
    }
    if (groups == 0) return 0;
    sh::StreamCall call(stream);
    if (call.rc) return call.rc;
    const ShorthairRxWindow none{};  // a fresh receiver: no previous window
    const ShorthairRxWindow &p = prev ? *prev : none;
    sh::RxWindowArgs a{.p_base = p.base,
                       .p_first = p.first,
                       .p_off = p.off,
                       .p_len = p.len,
                       .p_done = p.done,
                       .g_first = d_pkt_first,
                       .g_off = d_pkt_off,
                       .g_len = d_pkt_len,
                       .g_dg = d_pkt_dg,
                       .g_slot_group = d_slot_group,
                       .ring = static_cast<uint8_t *>(d_ring),
                       .ring_bytes = ring_bytes,
                       .hold_off = hold_off,
                       .hold_bytes = hold_bytes,
                       .n_base = next->base,
                       .n_first = next->first,
                       .n_off = next->off,
                       .n_len = next->len,
                       .n_dg = next->dg,
                       .n_done = next->done,
                       .summary = d_summary,
                       .errors = call.errors,
                       .groups = groups,
                       .datagrams = datagrams,
                       .p_cap = p.capacity,
                       .n_cap = next->capacity,
                       .n_info = n_info,
                       .has_prev = prev != nullptr};
    std::copy(d_info, d_info + n_info, a.info);
    return launched(sh::launch_rx_window(a, d_scratch, call.stream), "shorthair_rx_window_batch");
}

extern "C" long long shorthair_tx_datagram_scratch_bytes(int datagrams) {
    if (datagrams < 0) return -1;
    return sh::tx_datagram_scratch_bytes(datagrams);
}

extern "C" long long shorthair_tx_datagram_capacity(int datagrams, int max_datagram_bytes, int align) {
    if (datagrams < 0 || max_datagram_bytes < 0 || align < 1 || align > 4096 || (align & (align - 1))) return -1;
    const long long each = (static_cast<long long>(max_datagram_bytes) + align - 1) & ~static_cast<long long>(align - 1);
    return datagrams * each;
}

extern "C" int shorthair_tx_datagram_batch(int datagrams, int groups, int m, int block_bytes, const int *d_sched,
                                           const int *d_first, int total_blocks, const void *d_payload,
                                           long long payload_bytes, const long long *d_off, const int *d_len,
                                           const void *d_recovery, long long recovery_bytes,
                                           const ShorthairTxGroupDesc *d_group, int n_pong, const int *d_pong_at,
                                           const unsigned *d_pong_val, int advance, const int *d_state_in,
                                           int *d_state_out, int align, void *d_ring, long long ring_bytes,
                                           long long *d_dg_off, int *d_dg_len, int *d_dg_class, int *d_summary,
                                           void *d_scratch, void *stream) {
    if (datagrams < 0 || groups < 0 || groups > (1 << 22) || m < 0 || block_bytes < 0 || total_blocks < 0) return -1;
    if (payload_bytes < 0 || recovery_bytes < 0 || ring_bytes < 0 || n_pong < 0 || advance < 0) return -1;
    if (align < 1 || align > 4096 || (align & (align - 1))) return -1;
    if (mis(d_sched, 4) || mis(d_first, 4) || mis(d_len, 4) || mis(d_pong_at, 4) || mis(d_pong_val, 4) ||
        mis(d_state_in, 4) || mis(d_state_out, 4) || mis(d_dg_len, 4) || mis(d_dg_class, 4) || mis(d_summary, 4) ||
        mis(d_off, 8) || mis(d_group, 8) || mis(d_recovery, 8) || mis(d_dg_off, 8) || mis(d_scratch, 8))
        return -1;
    if (!d_state_in || !d_state_out || !d_dg_off || !d_summary || !d_scratch) return -1;
    if (datagrams > 0 && (!d_sched || !d_dg_len || !d_dg_class)) return -1;
    if (groups > 0 && !d_first) return -1;
    if (total_blocks > 0 && (!d_off || !d_len)) return -1;
    if ((payload_bytes > 0 && !d_payload) || (recovery_bytes > 0 && !d_recovery) || (ring_bytes > 0 && !d_ring)) return -1;
    if (n_pong > 0 && (!d_pong_at || !d_pong_val)) return -1;
    sh::StreamCall call(stream);
    if (call.rc) return call.rc;
    const sh::TxDatagramArgs a{.sched = d_sched,
                               .first = d_first,
                               .payload = static_cast<const uint8_t *>(d_payload),
                               .payload_bytes = payload_bytes,
                               .off = d_off,
                               .len = d_len,
                               .recovery = static_cast<const uint8_t *>(d_recovery),
                               .recovery_bytes = recovery_bytes,
                               .group = d_group,
                               .pong_at = d_pong_at,
                               .pong_val = d_pong_val,
                               .state_in = d_state_in,
                               .state_out = d_state_out,
                               .ring = static_cast<uint8_t *>(d_ring),
                               .ring_bytes = ring_bytes,
                               .dg_off = d_dg_off,
                               .dg_len = d_dg_len,
                               .dg_class = d_dg_class,
                               .summary = d_summary,
                               .errors = call.errors,
                               .datagrams = datagrams,
                               .groups = groups,
                               .m = m,
                               .B = block_bytes,
                               .total = total_blocks,
                               .n_pong = n_pong,
                               .advance = advance,
                               .align = align};
    return launched(sh::launch_tx_datagram(a, d_scratch, call.stream), "shorthair_tx_datagram_batch");
}
