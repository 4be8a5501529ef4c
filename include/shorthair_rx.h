/*
 * shorthair_rx.h -- device-resident listing of received packets (new; no counterpart in the reference).
 * The stage in front of shorthair_frame.h on the receive side.
 *
 * The reference decides on the CPU, packet by packet, whether a code group can be decoded and which of
 * its packets become the decoder's blocks (Decoder::OnData, Shorthair.cpp:796-898; CanRecover,
 * ShorthairDetails.hpp:328-336; RecoverGroup, Shorthair.cpp:704-761). This call applies the same rule to
 * a whole batch of groups whose datagrams sit in GPU memory, reading only their header bytes, and writes
 * exactly the arrays that shorthair_frame_batch (d_off, d_len, d_raw) and
 * cauchy_256_decode_batch_out_var (d_first, d_rows) read. The caller supplies where each datagram lies
 * and which group it belongs to -- what a completion queue reports -- and nothing else.
 *
 * Records. A received datagram, after the caller has stripped the 7-bit code-group byte and assigned the
 * datagram to its group, is a record "[id][c][body]" of d_pkt_len[p] bytes at d_ring + d_pkt_off[p]:
 *
 *   original   (Shorthair.cpp:1001-1015)   c == id, the body is the payload
 *   recovery   (:614-616)                  id = k + y, c = k - 1, the body is "[m-1][block]"
 *   a record is an original iff id <= c    (OnData :814)
 *
 * Reconstructing the truncated group counter (:774-780) is sequential state; it stays with the caller.
 * Group g holds the records p in [d_pkt_first[g], d_pkt_first[g + 1]), in arrival order.
 *
 * Per-group rule, in this order (the result is rx_info's of shorthair_recover_groups on the same
 * packets split into its two lists):
 *
 *   0  malformed, and nothing of the group is read: pkt_first[g] < 0, pkt_first[g + 1] < pkt_first[g],
 *      pkt_first[g + 1] > packets, or more than SHORTHAIR_RX_MAX_PACKETS records
 *   1  a record with len < 2, or whose span [off, off + len) leaves [0, ring_bytes], is malformed and
 *      makes its group malformed. Otherwise id and c are its bytes 0 and 1. n_orig and n_rec count the
 *      two classes; first_rec is the absolute index p of the group's first recovery record, or -1
 *   2  n_rec == 0: status 0, with k = m = block_bytes = 0
 *   3  k = c + 1 of the first recovery record; any recovery record with another c: malformed
 *   4  k == 1: status 2 if n_orig == 0, else status 0. Status 2 is the :858-866 form: the payload is
 *      bytes [2, len) of record first_rec; this call copies nothing for it
 *   5  n_orig >= k or n_orig + n_rec < k: status 0
 *   6  the last recovery record must have len >= 3, else malformed. m = its byte 2 + 1, B = its len - 3;
 *      B < 8, B % 8 != 0 or k + m > 256: malformed
 *   7  an original with c >= k, a repeated id, or len - 2 > B - 2: malformed. use = k - n_orig; each of
 *      the first `use` recovery records must have id in [k, k + m), an id not seen before and len ==
 *      B + 3, else malformed. Later recovery records are not checked beyond steps 1 and 3
 *   8  kmin <= k <= kmax, m == the argument m and B == the argument block_bytes: status 1 (listed),
 *      else status 3 (decodable, but another bucket). Either way d_info reports the group's k, m and B,
 *      so the caller can issue a second call for that bucket; the headers are then parsed again
 *   9  listed groups take their blocks in ascending g; one whose blocks would end past the capacity --
 *      possible only when the spans of d_pkt_first overlap, which is not rejected as such -- is
 *      malformed, and so is every listed group after it
 *
 * d_info[g] is SHORTHAIR_RX_INFO_INTS ints:
 *   [0] status   1 listed, 0 skipped, 2 k == 1 form, 3 decodable but another bucket, -1 malformed
 *   [1] k  [2] m  [3] block_bytes   as far as the rule got: 0 0 0 at step 2; k 0 0 at steps 4 and 5
 *   [4] n_orig  [5] n_rec  [6] slot (-1 unless listed)  [7] first_rec (-1 if none)
 * A malformed group reports -1 0 0 0 0 0 -1 -1, and adds one to the stream's error counter, which
 * cauchy_256_batch_errors(stream) reads and resets.
 *
 * d_summary[8]: [0] groups listed [1] blocks listed [2] skipped [3] k == 1 [4] other bucket
 *               [5] malformed [6..7] 0
 *
 * Lists. capacity = shorthair_rx_list_capacity(groups, packets, kmax) = min(packets, groups * kmax).
 * Listed groups take slots 0, 1, ... in ascending g: d_info[g][6] is the slot and d_slot_group[slot] = g;
 * d_slot_group is -1 for every slot at or past n_listed. d_first[0] = 0, d_first[s + 1] - d_first[s] = k
 * of slot s, and d_first[s] = total_listed for every s > n_listed. For slot s with f = d_first[s]
 * (RecoverGroup :713-737):
 *
 *   blocks f + i, i < n_orig        the originals in arrival order:
 *                                   off = pkt_off + 2, len = pkt_len - 2, raw = 0, row = id
 *   blocks f + n_orig + j, j < use  the recovery records in arrival order:
 *                                   off = pkt_off + 3, len = B, raw = 1, row = id
 *
 * Entries [total_listed, capacity) of d_off, d_len, d_raw and d_rows are written as 0, so a
 * shorthair_frame_batch over `capacity` blocks frames zero-length blocks there and counts nothing. Every
 * output element named above is written on every call: nothing depends on earlier contents. The ring
 * and the three input arrays are only read.
 *
 * Two ways to continue. (a) Read back d_summary (32 bytes) and pass groups = d_summary[0],
 * total_blocks = d_summary[1] to shorthair_frame_batch and cauchy_256_decode_batch_out_var. (b) Without
 * any synchronisation, pass `groups` and `capacity` as upper bounds: the decode marks each of the
 * groups - n_listed empty tail slots with count -1 and counts it once in the error counter; d_summary[0]
 * lets the caller subtract those later.
 *
 * Scratch: shorthair_rx_list_scratch_bytes(groups, packets) bytes of device memory at d_scratch (8-byte
 * aligned), which the call overwrites; the caller owns it so that the call allocates nothing. The size
 * is > 0 for valid arguments and non-decreasing in both. It holds two ints per group and two bytes per
 * record. One workgroup scans the groups for slots and d_first: each of its lanes sums
 * SHORTHAIR_RX_SCAN_TILE consecutive groups, SHORTHAIR_RX_SCAN_PASS groups per pass with a running
 * carry.
 *
 * Host-checked (-1, nothing enqueued, the GPU is not initialised): 2 <= kmin <= kmax <= 255; m >= 1 and
 * kmax + m <= 256; block_bytes >= 8 and block_bytes % 8 == 0; groups, packets and ring_bytes >= 0;
 * d_pkt_first, d_pkt_len, d_info, d_first, d_slot_group, d_len and d_summary 4-byte aligned; d_pkt_off,
 * d_off and d_scratch 8-byte aligned; when groups > 0, non-null d_pkt_first, d_info, d_first,
 * d_slot_group, d_summary and d_scratch, non-null d_pkt_off, d_pkt_len and d_ring unless packets == 0,
 * and non-null d_off, d_len, d_raw and d_rows unless the capacity is 0. groups == 0 returns 0 and
 * touches nothing.
 *
 * Asynchronous on `stream` (a hipStream_t passed through verbatim: NULL = the null stream): three
 * kernels, none of which waits on another workgroup; no host synchronisation, no device array is read
 * on the host, and nothing is allocated after the stream's first call into the library, so the call can
 * be captured into a graph.
 *
 * Return codes: 0 ok, -1 invalid arguments, -2 GPU/runtime error.
 */
#ifndef SH_AMD_SHORTHAIR_RX_H
#define SH_AMD_SHORTHAIR_RX_H

#ifdef __cplusplus
extern "C" {
#endif

#define SHORTHAIR_RX_MAX_PACKETS 512 /* records per group; more: the group is malformed */
#define SHORTHAIR_RX_INFO_INTS 8     /* ints per group in d_info */
#define SHORTHAIR_RX_SCAN_TILE 16    /* consecutive groups one lane of the scan workgroup sums */
#define SHORTHAIR_RX_SCAN_PASS 4096  /* groups the scan workgroup takes per pass */

/* min(packets, groups * kmax): entries of each list array. Host only: never initialises the GPU. -1 on
 * invalid arguments (groups < 0, packets < 0, kmax outside 2..255). */
int shorthair_rx_list_capacity(int groups, int packets, int kmax);

/* Bytes of device scratch the call below needs. Host only. -1 on invalid arguments (groups < 0,
 * packets < 0). */
long long shorthair_rx_list_scratch_bytes(int groups, int packets);

int shorthair_rx_list_batch(int kmin, int kmax, int m, int block_bytes, int groups, int packets,
                            const int *d_pkt_first /* [groups + 1] */, const long long *d_pkt_off /* [packets] */,
                            const int *d_pkt_len /* [packets] */, const void *d_ring, long long ring_bytes,
                            int *d_info /* [groups][8] */, int *d_first /* [groups + 1] */,
                            int *d_slot_group /* [groups] */, long long *d_off, int *d_len,
                            unsigned char *d_raw, unsigned char *d_rows /* each [capacity] */,
                            int *d_summary /* [8] */, void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SH_AMD_SHORTHAIR_RX_H */
