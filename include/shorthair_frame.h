/*
 * shorthair_frame.h -- device-resident payload framing (new; no counterpart in the reference).
 *
 * The reference turns each queued payload into a code block on the CPU: "[len u16 LE][payload]
 * [zeros up to block_bytes]" (Encoder::EncodeQueued, Shorthair.cpp:540-557; RecoverGroup :710-725),
 * and takes a received recovery packet's body as a block verbatim (:727-735). This call does the
 * same for a whole batch whose payload bytes already sit in GPU memory, and writes exactly the
 * packed block array the batch calls of cauchy_256_batch.h read: the var-k calls (first[] indexes
 * it) and the uniform calls (total_blocks = groups * k).
 *
 *   block j of d_blocks[total_blocks][block_bytes]
 *       = [len_j u16 LE][d_payload[off_j .. off_j + len_j)][zeros]          d_raw == NULL or d_raw[j] == 0
 *       = d_payload[off_j .. off_j + block_bytes) verbatim                  d_raw[j] != 0
 *
 * d_off / d_len are separate arrays (not CSR): payloads may sit anywhere in [0, payload_bytes) of
 * d_payload, at any byte alignment, with headers and gaps between them (a receive ring). Nothing
 * outside [0, payload_bytes) is read.
 *
 * Host-checked (-1, nothing enqueued, the GPU is not initialised): block_bytes >= 8 and
 * block_bytes % 8 == 0; total_blocks >= 0; payload_bytes >= 0; d_payload, d_off, d_len and d_blocks
 * non-null when total_blocks > 0; d_blocks 8-byte aligned.
 *
 * Malformed blocks are seen only by the device: len_j < 0 or len_j > min(block_bytes - 2, 65535);
 * for a raw block len_j != block_bytes; a span [off_j, off_j + len_j) that leaves [0, payload_bytes].
 * Nothing of such a block is read, it is written as all zeros, and it is counted in the stream's
 * error counter, which cauchy_256_batch_errors(stream) reads and resets. The other blocks are
 * unaffected.
 *
 * Asynchronous on `stream` (a hipStream_t passed through verbatim: NULL = the null stream): no host
 * synchronisation, no device array is read on the host, and nothing is allocated after the
 * stream's first call into the library.
 *
 * Return codes: 0 ok, -1 invalid arguments, -2 GPU/runtime error.
 */
#ifndef SH_AMD_SHORTHAIR_FRAME_H
#define SH_AMD_SHORTHAIR_FRAME_H

#ifdef __cplusplus
extern "C" {
#endif

int shorthair_frame_batch(int block_bytes, int total_blocks, const void *d_payload, long long payload_bytes,
                          const long long *d_off, const int *d_len, const unsigned char *d_raw /* may be NULL */,
                          void *d_blocks, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SH_AMD_SHORTHAIR_FRAME_H */
