/*
 * shorthair_wire.h -- device-resident wire framing of recovery blocks (new; no counterpart in the
 * reference).
 *
 * The reference frames recovery block y of a group on the CPU as "[k+y][k-1][m-1][block]"
 * (Encoder::GenerateRecoveryBlock, Shorthair.cpp:598-608). This call does the same for a whole batch
 * whose recovery blocks already sit in GPU memory -- the output of cauchy_256_encode_batch or
 * cauchy_256_encode_batch_var (cauchy_256_batch.h) -- and leaves the packets in GPU memory.
 *
 * Write B = block_bytes, S = 3 + B. d_recovery is [groups][m][B]. d_wire receives groups * m records
 * of S bytes, dense: record p = g * m + y lies at byte p * S and holds
 *
 *       [k_g + y][k_g - 1][m - 1][d_recovery[g][y][0..B)]
 *
 * which is the layout of ShorthairTxGroup.out with out_stride = 3 + B (shorthair_groups.h), and what
 * shorthair_frame_batch (shorthair_frame.h) reads as a raw block at off = p * S + 3.
 *
 * d_first == NULL: k_g = k for every group and total_blocks is ignored. Otherwise k is kmax and
 * d_first[groups + 1] is the var-k calls' array: k_g = d_first[g + 1] - d_first[g]. A malformed group, by
 * the rule of those calls (k_g outside 2..kmax, or a span that leaves [0, total_blocks]), gets all m
 * records written as S zero bytes, header included. It is not counted: the encode call before this one
 * counted it, and this call never touches the stream's error counter.
 *
 * Every byte of [0, groups * m * S) of d_wire is written and nothing outside it. Nothing outside
 * [0, groups * m * B) of d_recovery is read, and nothing outside d_first[0..groups]. The two buffers
 * must not overlap. d_wire takes any address; d_recovery must be 8-byte aligned and d_first 4-byte
 * aligned. All byte offsets are 64-bit.
 *
 * Host-checked (-1, nothing enqueued, the GPU is not initialised): k in 2..255; m >= 1; k + m <= 256;
 * block_bytes >= 8 and block_bytes % 8 == 0; groups >= 0; groups * m <= INT_MAX; with d_first,
 * 0 <= total_blocks <= groups * k and d_first 4-byte aligned; d_recovery and d_wire non-null when
 * groups > 0; d_recovery 8-byte aligned. groups == 0 returns 0 and does no GPU work.
 *
 * Asynchronous on `stream` (a hipStream_t passed through verbatim: NULL = the null stream): no host
 * synchronisation, no device array is read on the host, and nothing is allocated. Runs on the
 * library's device and restores the caller's.
 *
 * Return codes: 0 ok, -1 invalid arguments, -2 GPU/runtime error.
 */
#ifndef SH_AMD_SHORTHAIR_WIRE_H
#define SH_AMD_SHORTHAIR_WIRE_H

#ifdef __cplusplus
extern "C" {
#endif

int shorthair_wire_emit_batch(int k, int m, int block_bytes, int groups,
                              const int *d_first /* NULL: every group has k originals */, int total_blocks,
                              const void *d_recovery, void *d_wire, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* SH_AMD_SHORTHAIR_WIRE_H */
