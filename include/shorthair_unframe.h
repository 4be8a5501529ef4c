/*
 * shorthair_unframe.h -- device-resident delivery of recovered blocks (new; no counterpart in the
 * reference). The inverse of shorthair_frame.h.
 *
 * The reference hands every recovered block to the application on the CPU: it reads the block's
 * "[len u16 LE]" prefix and delivers "data + 2, len" when len <= block_bytes - 2, and drops the block
 * otherwise (RecoverGroup, Shorthair.cpp:741-756). This call applies the same rule to a whole batch of
 * recovered blocks that sit in GPU memory -- d_out / d_out_count as cauchy_256_decode_batch_out and
 * cauchy_256_decode_batch_out_var (cauchy_256_batch.h) leave them -- and packs the delivered payloads
 * back to back into d_payload, with their lengths and offsets alongside.
 *
 *   slot s = g * emax + i           (g in 0..groups-1, i in 0..emax-1; slots = groups * emax)
 *   its block                       the block_bytes bytes at d_out + (g * group_stride_blocks + i) * block_bytes
 *   c_g                             d_out_count ? d_out_count[g] : emax
 *
 * group_stride_blocks = emax is the d_out[groups][emax][block_bytes] layout of the two decode_batch_out
 * calls. For the in-place m = 1 decode (cauchy_256_decode_batch, the erasure lands in block k - 1 of
 * d_blocks[groups][k][block_bytes]): d_out = d_blocks + (k - 1) * block_bytes, group_stride_blocks = k,
 * emax = 1, d_out_count = NULL.
 *
 * Per group: c_g == -1 is the decode's malformed flag: the group yields nothing (every d_len = -1) and is
 * not counted again. c_g < -1 or c_g > emax yields nothing as well and is counted once per group in the
 * stream's error counter, which cauchy_256_batch_errors(stream) reads and resets.
 *
 * Per slot:
 *   i >= c_g (or a group that yields nothing)   d_len[s] = -1; the block is not read
 *   else p = u16 LE at the block's byte 0
 *        p > block_bytes - 2                    d_len[s] = -2: dropped as the reference drops it; no error
 *        else                                   d_len[s] = p, and block bytes [2, 2 + p) are copied to
 *                                               d_payload + d_off[s]
 *
 * Offsets: d_off[s] = sum over t < s of max(d_len[t], 0), in 64 bits, for every slot, delivered or
 * not; d_off[slots] is the total. Payloads are packed with no alignment and no gap, so (d_payload,
 * d_off, d_len) restricted to the delivered slots is valid input for shorthair_frame_batch.
 *
 * Capacity: a payload of p > 0 bytes whose span [d_off[s], d_off[s] + p) leaves [0, payload_capacity)
 * is not written at all and is counted in the error counter (an empty payload has an empty span and
 * is never counted). d_off and d_len do not depend on payload_capacity, so d_off[slots] tells the
 * caller the capacity it needed. No byte outside [0, min(total, payload_capacity)) of d_payload is
 * written, no byte is written twice, and d_out is only read.
 *
 * Stale input: the result does not depend on the bytes of slots i >= c_g nor on block bytes past
 * 2 + p (the decode leaves zeros there; anything may be there).
 *
 * Scratch: the call needs shorthair_unframe_scratch_bytes(groups, emax) bytes of device memory at
 * d_scratch (8-byte aligned), which it overwrites; the caller owns it so that the call allocates
 * nothing. The size is > 0 for valid arguments and non-decreasing in groups and in emax. It holds one
 * 64-bit sum per tile of SHORTHAIR_UNFRAME_TILE_SLOTS slots, scanned by one workgroup in passes of
 * SHORTHAIR_UNFRAME_SCAN_PASS sums, and one 32-bit in-tile offset per slot.
 *
 * Host-checked (-1, nothing enqueued, the GPU is not initialised): block_bytes >= 8 and
 * block_bytes % 8 == 0; groups >= 0; emax in 1..255; groups * emax <= INT_MAX; group_stride_blocks >=
 * emax; payload_capacity >= 0; d_out 8-byte aligned, d_off 8-byte aligned, d_len 4-byte aligned,
 * d_scratch 8-byte aligned; when groups > 0, non-null d_out, d_off, d_len and d_scratch, and non-null
 * d_payload when payload_capacity > 0 as well. groups == 0 returns 0 and touches nothing.
 *
 * Asynchronous on `stream` (a hipStream_t passed through verbatim: NULL = the null stream): three
 * kernels, none of which waits on another workgroup; no host synchronisation, no device array is read
 * on the host, and nothing is allocated after the stream's first call into the library.
 *
 * Return codes: 0 ok, -1 invalid arguments, -2 GPU/runtime error.
 */
#ifndef SH_AMD_SHORTHAIR_UNFRAME_H
#define SH_AMD_SHORTHAIR_UNFRAME_H

#ifdef __cplusplus
extern "C" {
#endif

#define SHORTHAIR_UNFRAME_TILE_SLOTS 256 /* slots whose lengths one workgroup sums */
#define SHORTHAIR_UNFRAME_SCAN_PASS 256  /* tile sums the scan workgroup takes per pass */

/* Bytes of device scratch the call below needs for (groups, emax). Host only: never initialises the
 * GPU. -1 on invalid arguments (groups < 0, emax outside 1..255, groups * emax > INT_MAX). */
long long shorthair_unframe_scratch_bytes(int groups, int emax);

int shorthair_unframe_batch(int block_bytes, int groups, int emax, long long group_stride_blocks,
                            const void *d_out, const int *d_out_count /* may be NULL */,
                            void *d_payload, long long payload_capacity,
                            long long *d_off /* [groups*emax + 1] */, int *d_len /* [groups*emax] */,
                            void *d_scratch, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SH_AMD_SHORTHAIR_UNFRAME_H */
