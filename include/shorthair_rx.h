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
 * Reconstructing the truncated group counter (:774-780) and sorting the datagrams by group is what
 * shorthair_rx_group_batch (below) does, on the GPU, for datagrams as they arrive.
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

/*
 * shorthair_rx_group_batch -- the stage in front of the listing: datagrams as they arrive, in arrival
 * order, become the records and the CSR by group that shorthair_rx_list_batch reads (its d_pkt_first,
 * d_pkt_off and d_pkt_len, with packets = datagrams). The host supplies the (offset, length) pairs its
 * completion queue reports and one int of state, and reads no header byte.
 *
 * Datagram i is the d_dg_len[i] bytes at d_ring + d_dg_off[i], at any alignment, exactly as
 * ShorthairCodec::Recv (Shorthair.cpp:1192-1211) gets it: "[seq u16]", then one of
 *
 *   [g & 0x7f][id][c][body]                  a data datagram (Send :984-1015)
 *   [0x80 | ...][oob bytes]                  an out-of-band datagram (SendOOB :1036-1055)
 *   [f with bits 0x80 and 1][seen u32][count u32]
 *                                            a pong prefix (Tick :1079-1089, OnOOB :664-699), followed by
 *                                            nothing, by "[0x80 | ...][oob]" or by "[g][id][c][body]"
 *
 * d_state_in[0] is the unwrapped group number U of the last data datagram before this batch; U & 255 is
 * the reference's _last_group. A fresh receiver passes 0. With s7(x) = ((x & 127) ^ 64) - 64:
 *
 * Per-datagram rule, in this order:
 *
 *   1  malformed (class -1), and nothing of the datagram is read: len < 3, off < 0 or off + len >
 *      ring_bytes
 *   2  f = byte 2. If f & 0x80 and f & 1, the datagram carries a pong and 8 is added to its class:
 *      len < 11 is class -1 after all (OnOOB drops a truncated pong; no 8 is added, and it is not counted
 *      as carrying a pong); len == 11 is kind 2, pong only; otherwise h = 11, and byte 11 decides: kind 1
 *      (out of band) when it has bit 0x80, else a data candidate. If f & 0x80 without bit 0: kind 1,
 *      h = 2. Otherwise a data candidate with h = 2. The out-of-band payload and the record
 *      "[id][c][body]" both start at off + h + 1
 *   3  a data candidate's record has len - h - 1 bytes. At most 2: kind 3, short (OnData returns at
 *      len <= PROTOCOL_OVERHEAD before it touches _last_group, so a short datagram does not move the group
 *      state). Otherwise it is a data datagram with p = byte h & 127
 *   4  the data datagrams of step 3, in arrival order: u_i = u_prev + s7(p_i - prev_p), where for the
 *      first one u_prev = d_state_in[0] and prev_p = d_state_in[0] & 127, and after that u_prev and prev_p
 *      are the previous data datagram's u and p. u_i & 255 is the code_group of :774-780
 *      (Counter<u8,8>::ExpandFromTruncated, Counter.h:297-316). u is kept modulo 2^32.
 *      d_state_out[0] is the last u, or d_state_in[0] if the batch has no data datagram
 *   5  slot = u_i - d_state_in[0] + back. Outside [0, groups): kind 4, out of window; it has still moved
 *      the group state in step 4, as it would in the reference. Otherwise kind 0, binned
 *
 * Outputs; every element named here is written on every call, and nothing depends on earlier contents:
 *
 *   d_dg_class[i]   kind (+ 8 with a pong), or -1
 *   d_dg_slot[i]    the slot for kind 0, else -1
 *   d_pkt_first     [groups + 1]: slot s holds the records [d_pkt_first[s], d_pkt_first[s + 1]), the
 *                   kind-0 datagrams of the slot in arrival order
 *   d_pkt_off, d_pkt_len, d_pkt_dg
 *                   per record: dg_off + h + 1, dg_len - h - 1 and the datagram's index i. Entries at or
 *                   past the record total are 0, 0 and -1
 *   d_slot_group[s] d_state_in[0] - back + s: the unwrapped group of every slot, so that a caller matches
 *                   slots across batches without reading the state back
 *   d_other         the indices of all datagrams that were not binned, ascending; -1 past their count
 *   d_summary[8]    [0] records binned [1] entries of d_other [2] lowest used slot (groups if none)
 *                   [3] highest used slot + 1 (0 if none) [4] malformed [5] out of window
 *                   [6] datagrams carrying a pong (class >= 8) [7] short
 *
 * Malformed datagrams add to the stream's error counter (cauchy_256_batch_errors), as the listing's
 * malformed groups do.
 *
 * Arrival order within a slot is exact for every slot with at most SHORTHAIR_RX_MAX_PACKETS records. A
 * slot with more holds each of its records exactly once, in an unspecified order; the listing rejects
 * such a group anyway.
 *
 * What the call does not do. The loss statistics from the sequence numbers (LossStatistics::Update,
 * which has a reset branch) stay with the caller. Group time-outs and "ignore the rest of a finished
 * group" (:783-791) are time and history: the batch looks at all records of a slot, as the listing does.
 * The listing's limit of SHORTHAIR_RX_MAX_PACKETS records is unchanged. Two slots more than 256 apart
 * share an 8-bit group number in the reference; here they stay distinct.
 *
 * Scratch: shorthair_rx_group_scratch_bytes(datagrams, groups) bytes of device memory at d_scratch
 * (8-byte aligned), which the call overwrites; > 0 for valid arguments and non-decreasing in both. It
 * holds a counter per slot, two ints per datagram and eight per tile. The datagrams are scanned in tiles
 * of SHORTHAIR_RX_GROUP_TILE; one workgroup scans the tile aggregates, SHORTHAIR_RX_GROUP_TILE_PASS tiles
 * per pass with a running carry, and another the slot counters: each of its lanes sums
 * SHORTHAIR_RX_GROUP_SLOT_TILE consecutive slots, SHORTHAIR_RX_GROUP_SLOT_PASS slots per pass.
 *
 * Host-checked (-1, nothing enqueued, the GPU is not initialised): datagrams, groups and ring_bytes >= 0;
 * 0 <= back <= groups; d_dg_len, d_state_in, d_state_out, d_dg_class, d_dg_slot, d_pkt_first, d_pkt_len,
 * d_pkt_dg, d_slot_group, d_other and d_summary 4-byte aligned; d_dg_off, d_pkt_off and d_scratch 8-byte
 * aligned; when groups > 0, non-null d_state_in, d_state_out, d_pkt_first, d_slot_group, d_summary and
 * d_scratch, and non-null d_dg_off, d_dg_len, d_ring, d_dg_class, d_dg_slot, d_pkt_off, d_pkt_len,
 * d_pkt_dg and d_other unless datagrams == 0. groups == 0 returns 0 and touches nothing; datagrams == 0
 * with groups > 0 writes the empty outputs. There is no limit on groups other than memory.
 *
 * Asynchronous on `stream`, like the listing: six kernels, none of which waits on another workgroup; no
 * host synchronisation, nothing is allocated after the stream's first call into the library, so the call
 * can be captured into a graph. Return codes: 0 ok, -1 invalid arguments, -2 GPU/runtime error.
 */
#define SHORTHAIR_RX_GROUP_TILE 256       /* datagrams per tile of the datagram scans */
#define SHORTHAIR_RX_GROUP_TILE_PASS 1024 /* tile aggregates the scan workgroup takes per pass */
#define SHORTHAIR_RX_GROUP_SLOT_TILE 16   /* consecutive slots one lane of the slot scan sums */
#define SHORTHAIR_RX_GROUP_SLOT_PASS 4096 /* slots the slot scan takes per pass */

/* Bytes of device scratch the call below needs. Host only. -1 on invalid arguments (datagrams < 0,
 * groups < 0). */
long long shorthair_rx_group_scratch_bytes(int datagrams, int groups);

int shorthair_rx_group_batch(int datagrams, int groups, int back,
                             const long long *d_dg_off /* [datagrams] */, const int *d_dg_len /* [datagrams] */,
                             const void *d_ring, long long ring_bytes,
                             const int *d_state_in /* [1] */, int *d_state_out /* [1], may alias d_state_in */,
                             int *d_dg_class /* [datagrams] */, int *d_dg_slot /* [datagrams] */,
                             int *d_pkt_first /* [groups + 1] */,
                             long long *d_pkt_off, int *d_pkt_len, int *d_pkt_dg /* each [datagrams] */,
                             int *d_slot_group /* [groups] */, int *d_other /* [datagrams] */,
                             int *d_summary /* [8] */, void *d_scratch, void *stream);

/*
 * shorthair_rx_window_batch -- what a receiver keeps between two batches: the records of the groups that
 * are still open, and which groups are done (Decoder::OnData ignores the rest of a finished group,
 * Shorthair.cpp:783-791, IsDone). It runs between the group call and the listing:
 *
 *   group(new datagrams) -> window(prev window, prev d_info, new records) -> list -> frame -> decode -> unframe
 *
 * A window is `groups` slots of consecutive unwrapped group numbers: slot s is group *base + s. Per slot it
 * holds the records of its open group in arrival order, as a CSR like the group call's, and a done code.
 * The caller owns two windows and alternates them as prev and next. The next window's first, off and len
 * are exactly shorthair_rx_list_batch's d_pkt_first, d_pkt_off and d_pkt_len, with packets = capacity.
 * ShorthairRxWindow is a host struct of device pointers, read on the host at the call.
 *
 * All group arithmetic is on 32-bit wrapped values compared by signed difference. Rule, in this order:
 *
 *   1  Base. Gb = d_slot_group[0]; P = *prev->base. N = Gb for a fresh receiver (prev == NULL), else
 *      N = P + max(0, Gb - P): the window never moves back, so a done code is never lost. *next->base = N
 *   2  Old slots (prev != NULL). Old slot so has the records [prev->first[so], prev->first[so + 1]). Its
 *      finished flag f is 2 if any of the n_info arrays has status -1 for so; else 1 if any has status 1 or
 *      2, or status 0 with k >= 1 and n_orig >= k (all originals seen, :851-857); else 0. d =
 *      prev->done[so] if that is non-zero, else f. The arrays are the d_info outputs of the listing calls
 *      that ran over prev's arrays; n_info == 0 finishes nothing. The new slot is s = so - (N - P). Inside
 *      [0, groups): next->done[s] = d, and if d == 0 the slot's records are carried, with dg = -1. Outside:
 *      the slot expires, and counts in d_summary[4] if d == 0 and prev->first[so + 1] > prev->first[so]
 *      (nothing else of an expiring slot is read). This takes the place of the reference's GROUP_TIMEOUT: a
 *      group leaves when the window's base passes it, not after a time. New slots that no old slot maps to
 *      are open and empty. d_summary[3] counts the old slots, expiring or not, with prev->done[so] == 0 and
 *      f == 1
 *   3  New records. Slot t of the group call, with the records [d_pkt_first[t], d_pkt_first[t + 1]), maps
 *      to s = t - (N - Gb). s < 0: below the window, dropped and counted in [6]. next->done[s] != 0 (from
 *      step 2, or made malformed by step 4 on the carried side): ignored, as :787-791 does, and counted in
 *      [5]. Else they are appended behind the slot's carried records in their own order, with dg from
 *      d_pkt_dg
 *   4  Malformed input. A span is malformed if its start is below 0, its end before its start, or its end
 *      past prev->capacity (of prev) or past `datagrams` (of the group call). A carried record is malformed
 *      if len < 0, off < 0 or off + len > ring_bytes. A slot that would carry such a span or record, or an
 *      open slot whose new span is malformed, is malformed: it gets no records and done = 2, and adds one
 *      to the stream's error counter (cauchy_256_batch_errors) and to [7]. A malformed new span of a slot
 *      that is below the window or not open counts nothing. Nothing out of bounds is ever read
 *   5  Placement. Slots take their records in ascending s: next->first[0] = 0, next->first[groups] the
 *      total. With hold_bytes > 0, carried record r is copied to d_ring + hold_off + (the exclusive sum of
 *      len rounded up to SHORTHAIR_RX_HOLD_ALIGN over the carried records before it), and its off is that
 *      place. New records keep their offsets. With hold_bytes == 0 nothing is copied and carried records
 *      keep their offsets; the caller then keeps the bytes alive
 *   6  Overflow. The first slot whose records would end past next->capacity, or whose carried bytes -- the
 *      rounded sum including its own records -- would end past hold_bytes (when hold_bytes > 0), and every
 *      later slot that has a record, is emptied and gets done = 3; each adds one to the error counter and
 *      to [7]
 *   7  Tail. Entries of off, len and dg at or past the total are 0, 0 and -1
 *   8  Writes. Every named output element is written on every call. prev, the info arrays and the group
 *      call's outputs are only read. Of d_ring, exactly the carried records' bytes inside [hold_off,
 *      hold_off + hold_bytes) are written; pad bytes and everything else are left alone, and no byte is
 *      written twice
 *
 * d_summary[8] (64-bit): [0] records in the next window [1] carried records [2] hold bytes used (the
 * rounded sum) [3] slots newly finished [4] open slots that expired [5] new records ignored [6] new
 * records below the window [7] slots made malformed or emptied.
 *
 * Source lifetime. prev's records are the sources: they lie in the previous hold region and the previous
 * batch's ring region. Both must stay intact until the call has run, and must not overlap the hold region
 * that is written. Reach of a load: a load may reach up to 7 bytes past (or, at the ring's end, before) a
 * record shorter than 8 bytes; it never leaves [0, ring_bytes), and what it reaches outside the record is
 * masked away.
 *
 * Delivering originals. The caller delivers the records of the next window that have dg >= 0 and id <= c:
 * what OnData delivers on arrival. Carried records (dg == -1) were delivered in their own batch.
 *
 * Scratch: shorthair_rx_window_scratch_bytes(groups, capacity) bytes of device memory at d_scratch (8-byte
 * aligned), which the call overwrites, for `capacity` the larger of the two windows' capacities; > 0 for
 * valid arguments and non-decreasing in both. It holds seven ints per slot and forty bytes per 256 slots;
 * nothing is kept per record today. One workgroup scans the slots' (records, bytes) pairs: each of its lanes sums
 * SHORTHAIR_RX_WINDOW_SCAN_TILE consecutive slots, SHORTHAIR_RX_WINDOW_SCAN_PASS slots per pass with a
 * running carry.
 *
 * Host-checked (-1, nothing enqueued, the GPU is not initialised): groups, datagrams and both capacities
 * >= 0; next non-null; 0 <= n_info <= SHORTHAIR_RX_WINDOW_MAX_INFO, n_info == 0 when prev is NULL, d_info
 * non-null when n_info > 0; ring_bytes, hold_off and hold_bytes >= 0 and hold_off + hold_bytes <=
 * ring_bytes; base, first, len, dg of both windows, every d_info[j], d_pkt_first, d_pkt_len, d_pkt_dg and
 * d_slot_group 4-byte aligned; off of both windows, d_pkt_off, d_summary and d_scratch 8-byte aligned; when
 * groups > 0, non-null base, first and done of both windows, every d_info[j], d_pkt_first, d_slot_group,
 * d_summary and d_scratch, non-null off, len and dg of a window unless its capacity is 0, non-null
 * d_pkt_off, d_pkt_len and d_pkt_dg unless datagrams == 0, and non-null d_ring unless ring_bytes == 0; prev
 * and next share no array. groups == 0 returns 0 and touches nothing.
 *
 * Asynchronous on `stream`, like the listing: four kernels, none of which waits on another workgroup; no
 * host synchronisation, nothing is allocated after the stream's first call into the library, so the call
 * can be captured into a graph (the pointers of prev, next and d_info are captured with it). Return codes:
 * 0 ok, -1 invalid arguments, -2 GPU/runtime error.
 */
#define SHORTHAIR_RX_WINDOW_MAX_INFO 4       /* d_info arrays of the previous window's listing calls */
#define SHORTHAIR_RX_HOLD_ALIGN 16           /* carried records start at multiples of this from hold_off */
#define SHORTHAIR_RX_WINDOW_SCAN_TILE 16     /* consecutive slots one lane of the window scan sums */
#define SHORTHAIR_RX_WINDOW_SCAN_PASS 4096   /* slots the window scan takes per pass */

typedef struct {
    int *base;           /* [1] unwrapped group of slot 0 */
    int *first;          /* [groups + 1] */
    long long *off;      /* [capacity] bytes from d_ring */
    int *len;            /* [capacity] */
    int *dg;             /* [capacity] datagram index within this batch; -1: carried from an earlier one */
    unsigned char *done; /* [groups] 0 open, 1 finished, 2 malformed, 3 emptied by overflow */
    int capacity;
} ShorthairRxWindow;

/* Bytes of device scratch the call below needs. Host only. -1 on invalid arguments (groups < 0,
 * capacity < 0). */
long long shorthair_rx_window_scratch_bytes(int groups, int capacity);

int shorthair_rx_window_batch(int groups, const ShorthairRxWindow *prev /* NULL: a fresh receiver */,
                              int n_info, const int *const *d_info /* host array of n_info device pointers, each [groups][8] */,
                              int datagrams, const int *d_pkt_first, const long long *d_pkt_off,
                              const int *d_pkt_len, const int *d_pkt_dg, const int *d_slot_group,
                              void *d_ring, long long ring_bytes, long long hold_off, long long hold_bytes,
                              const ShorthairRxWindow *next, long long *d_summary /* [8] */, void *d_scratch,
                              void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SH_AMD_SHORTHAIR_RX_H */
