/*
 * shorthair_tx.h -- device-resident datagrams in send order (new; no counterpart in the reference).
 * The mirror of shorthair_rx_group_batch (shorthair_rx.h): its outputs (d_ring, d_dg_off, d_dg_len) are that
 * call's inputs.
 *
 * The reference builds what leaves a sender on the CPU, datagram by datagram, from one running sequence
 * counter: an original in Send (Shorthair.cpp:966-1022), a recovery datagram in SendCheckSymbol (:631-649)
 * on GenerateRecoveryBlock (:589-625), a pong-only datagram in Tick (:1079-1089). This call writes a whole
 * batch of them from payloads and recovery blocks that sit in GPU memory, in the order a schedule names.
 *
 * Inputs. d_first [groups + 1] is the CSR of originals by slot, as the var-k calls take it: slot g holds
 * the payloads j in [d_first[g], d_first[g + 1]), k_g = d_first[g + 1] - d_first[g]; payload j is the
 * d_len[j] bytes at d_payload + d_off[j], as shorthair_frame_batch reads them (no raw blocks). Slot g's
 * recovery blocks are m_g blocks of B_g bytes at d_recovery + rec_off_g, as an encode wrote them: (rec_off_g,
 * m_g, B_g) = d_group[g], or (g * m * block_bytes, m, block_bytes) when d_group is NULL. m = 0, or a
 * descriptor with m = 0, means "no recovery yet": a streaming sender emits originals before their group is
 * encoded, and d_recovery may then be NULL.
 *
 * State. d_state_in[0] is the next sequence number (its low 16 bits go on the wire, as _out_seq's do);
 * d_state_in[1] is the unwrapped group number U0 of slot 0. Originals and recovery datagrams of slot g both
 * carry g7 = (U0 + g) & 0x7f: the reference sends the originals under _code_group + 1 and the recovery
 * after the swap under _code_group, which is the same number. d_state_out = { in[0] + datagrams, in[1] +
 * advance }, so a captured graph carries both counters from batch to batch with no host write.
 *
 * Schedule. Datagram i has seq_i = (d_state_in[0] + i) & 0xffff; every entry consumes a sequence number,
 * whatever becomes of it. With e = d_sched[i], and q the index with d_pong_at[q] == i if there is one
 * (d_pong_at is strictly ascending; if it is not, which entry wins is unspecified, but nothing is accessed
 * out of bounds), seen = d_pong_val[2q], total = d_pong_val[2q + 1] and
 * PONG = [0x81][seen u32 LE][total u32 LE] (9 bytes, :984-997):
 *
 * Per-datagram rule, in this order:
 *
 *   1  e == -1: a hole; the host sends a datagram of its own (out of band, say) under seq_i. With a pong:
 *      [seq u16 LE][PONG], 11 bytes, the pong-only datagram of Tick, class 3 + 8. Otherwise length 0, class 3
 *   2  e < -1: malformed. Otherwise g = e >> 9, x = e & 511; g >= groups: malformed
 *   3  f0 = d_first[g], f1 = d_first[g + 1]: f0 < 0, f1 > total_blocks or k_g = f1 - f0 outside 1..255:
 *      malformed
 *   4  x < 256, an original: x >= k_g is malformed; j = f0 + x; d_len[j] outside 0..65535, d_off[j] < 0 or
 *      d_off[j] + d_len[j] > payload_bytes: malformed. [seq][PONG if any][g7][x][x][payload j]: 5 + len bytes,
 *      14 + len with a pong; class 0, + 8 with a pong. m_g, B_g and rec_off_g are not looked at
 *   5  x >= 256, recovery y = x - 256. With a pong: malformed (the reference never does it). y >= m_g,
 *      m_g < 1 or k_g + m_g > 256: malformed
 *   6  k_g == 1: payload j = f0 is checked as in step 4; [seq][g7][1][0][payload f0], 5 + len bytes, class 2.
 *      B_g and rec_off_g are not looked at and d_recovery is not read
 *   7  k_g >= 2: B_g < 8, B_g % 8 != 0, B_g > SHORTHAIR_TX_MAX_BLOCK_BYTES, rec_off_g < 0, rec_off_g % 8 != 0
 *      or rec_off_g + m_g * B_g > recovery_bytes: malformed. [seq][g7][k_g + y][k_g - 1][m_g - 1][block y],
 *      6 + B_g bytes, block y at d_recovery + rec_off_g + y * B_g; class 1
 *
 * A malformed entry has length 0 and class -1, ignores a pong, and adds one to the stream's error counter,
 * which cauchy_256_batch_errors(stream) reads and resets.
 *
 * Placement. L_i being the lengths above, d_dg_off[i] is the exclusive sum of roundup(L_i, align) and
 * d_dg_off[datagrams] the total: the ring bytes the batch needs, reported even when the ring is smaller.
 * A datagram with L_i > 0 and d_dg_off[i] + L_i > ring_bytes does not fit: it is not written, d_dg_len[i]
 * = 0, class -2, and it is counted in the error counter and in d_summary[6]. The offsets ascend and keep
 * the rule's lengths, so the datagrams that do not fit are all those of non-zero length from the first one on;
 * a hole behind them stays class 3. shorthair_tx_datagram_capacity(datagrams, max_datagram_bytes, align) =
 * datagrams * roundup(max_datagram_bytes, align) always suffices when no L_i exceeds max_datagram_bytes
 * (SHORTHAIR_TX_MAX_DATAGRAM_BYTES never is exceeded).
 *
 * Outputs; every element named here is written on every call, and nothing depends on earlier contents:
 *
 *   d_ring          exactly the bytes [d_dg_off[i], d_dg_off[i] + d_dg_len[i]) of the written datagrams. No
 *                   byte is written twice, none is read, and gap bytes are left alone
 *   d_dg_off        [datagrams + 1], 64-bit
 *   d_dg_len[i]     L_i, or 0 where the datagram does not fit
 *   d_dg_class[i]   0 original, 1 recovery, 2 the k = 1 form, 3 hole; + 8 when the datagram carries a pong;
 *                   -1 malformed, -2 does not fit
 *   d_state_out     [2], see State; may alias d_state_in
 *   d_summary[8]    [0] written (d_dg_len > 0) [1] originals [2] recovery, the k = 1 form included [3] holes
 *                   [4] with a pong [5] malformed [6] not fitting [7] 0; [1]..[4] count final classes, so a
 *                   datagram that does not fit is in [6] only
 *
 * Read: d_sched, d_first[g], d_first[g + 1] and d_group[g] of the slots the schedule names, d_off[j] and
 * d_len[j] of the payloads it names, bytes [d_off[j], d_off[j] + d_len[j]) of d_payload -- a load may reach up
 * to 7 bytes further down or up, but never outside [0, payload_bytes) -- and the named blocks of d_recovery,
 * never a byte outside the block. d_ring and d_payload take any address; d_recovery is 8-byte aligned.
 *
 * Scratch: shorthair_tx_datagram_scratch_bytes(datagrams) bytes of device memory at d_scratch (8-byte
 * aligned), which the call overwrites: 32 bytes per datagram (its header bytes, source and lengths) and 32
 * per tile of SHORTHAIR_TX_TILE datagrams, + 8. > 0 for valid arguments and non-decreasing. One workgroup
 * scans the tile sums, SHORTHAIR_TX_TILE_PASS tiles per pass with a running carry.
 *
 * block_bytes also sizes the copy's sub-groups (the lanes that share a datagram: 16 bytes each per step,
 * at most 32 lanes); with d_group it is only that hint and may be 0, which means 32 lanes.
 *
 * Host-checked (-1, nothing enqueued, the GPU is not initialised): datagrams, groups, m, block_bytes,
 * total_blocks, payload_bytes, recovery_bytes, ring_bytes, n_pong and advance >= 0; groups <= 2^22 (an entry
 * holds the slot above 9 bits); align a power of two in 1..4096; d_sched, d_first, d_len, d_pong_at,
 * d_pong_val, d_state_in, d_state_out, d_dg_len, d_dg_class and d_summary 4-byte aligned; d_off, d_group,
 * d_recovery, d_dg_off and d_scratch 8-byte aligned; non-null d_state_in, d_state_out, d_dg_off, d_summary
 * and d_scratch; non-null d_sched, d_dg_len and d_dg_class unless datagrams == 0; non-null d_first unless
 * groups == 0; non-null d_off and d_len unless total_blocks == 0; non-null d_payload unless payload_bytes
 * == 0, d_recovery unless recovery_bytes == 0, d_ring unless ring_bytes == 0, d_pong_at and d_pong_val
 * unless n_pong == 0. datagrams == 0 still writes d_state_out, d_dg_off[0] = 0 and the summary.
 *
 * Asynchronous on `stream` (a hipStream_t passed through verbatim: NULL = the null stream): three kernels
 * (one when datagrams == 0), none of which waits on another workgroup; no host synchronisation, no device
 * array is read on the host, and nothing is allocated after the stream's first call into the library, so
 * the call can be captured into a graph.
 *
 * What the call does not do: out-of-band datagrams (holes are theirs), choosing the schedule or the
 * amount of recovery, and the encode itself.
 *
 * Return codes: 0 ok, -1 invalid arguments, -2 GPU/runtime error.
 */
#ifndef SH_AMD_SHORTHAIR_TX_H
#define SH_AMD_SHORTHAIR_TX_H

#ifdef __cplusplus
extern "C" {
#endif

#define SHORTHAIR_TX_TILE 256                 /* datagrams per tile of the length scan */
#define SHORTHAIR_TX_TILE_PASS 1024           /* tile sums the scan workgroup takes per pass */
#define SHORTHAIR_TX_MAX_BLOCK_BYTES 65544    /* roundup8(2 + 65535): the largest recovery block */
#define SHORTHAIR_TX_MAX_DATAGRAM_BYTES 65550 /* 6 + SHORTHAIR_TX_MAX_BLOCK_BYTES >= 14 + 65535 */
#define SHORTHAIR_TX_ORIGINAL(g, x) (((g) << 9) | (x))         /* schedule entry: original x of slot g */
#define SHORTHAIR_TX_RECOVERY(g, y) (((g) << 9) | 256 | (y))   /* schedule entry: recovery block y of slot g */
#define SHORTHAIR_TX_HOLE (-1)                                 /* schedule entry: the host's own datagram */

typedef struct {
    long long rec_off; /* bytes from d_recovery to the slot's first recovery block */
    int m;             /* recovery blocks of the slot; 0: none yet */
    int block_bytes;
} ShorthairTxGroupDesc; /* 16 bytes */

/* Bytes of device scratch the call below needs. Host only: never initialises the GPU. -1 if datagrams < 0. */
long long shorthair_tx_datagram_scratch_bytes(int datagrams);

/* datagrams * roundup(max_datagram_bytes, align): ring bytes that always suffice for datagrams of at most
 * max_datagram_bytes. Host only. -1 on invalid arguments (datagrams < 0, max_datagram_bytes < 0, align not
 * a power of two in 1..4096). */
long long shorthair_tx_datagram_capacity(int datagrams, int max_datagram_bytes, int align);

int shorthair_tx_datagram_batch(int datagrams, int groups, int m, int block_bytes,
                                const int *d_sched /* [datagrams] */,
                                const int *d_first /* [groups + 1] */, int total_blocks,
                                const void *d_payload, long long payload_bytes,
                                const long long *d_off, const int *d_len /* each [total_blocks] */,
                                const void *d_recovery, long long recovery_bytes,
                                const ShorthairTxGroupDesc *d_group /* [groups] or NULL */,
                                int n_pong, const int *d_pong_at /* [n_pong] */,
                                const unsigned *d_pong_val /* [2 * n_pong] */,
                                int advance, const int *d_state_in /* [2] */,
                                int *d_state_out /* [2], may alias d_state_in */,
                                int align, void *d_ring, long long ring_bytes,
                                long long *d_dg_off /* [datagrams + 1] */, int *d_dg_len /* [datagrams] */,
                                int *d_dg_class /* [datagrams] */, int *d_summary /* [8] */,
                                void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SH_AMD_SHORTHAIR_TX_H */
