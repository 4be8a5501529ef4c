/*
 * cauchy_256_batch.h -- batched, device-resident C ABI (new; no counterpart in the reference).
 *
 * The reference codes one group per call on one CPU thread (cauchy_256.cpp:1479, :1233). Here a
 * call codes `groups` independent code groups that already sit in GPU memory (HBM), with the same
 * per-group semantics and bytes as cauchy_256_encode / cauchy_256_decode. All calls are
 * asynchronous on `stream` (a hipStream_t passed through verbatim: NULL = the null stream) and
 * enqueue no host
 * synchronisation, except where noted for invalid parameters.
 *
 * Layouts (byte offsets inside one device allocation, no alignment required):
 *   data      [groups][k][block_bytes]      encode input
 *   recovery  [groups][m][block_bytes]      encode output
 *   blocks    [groups][k][block_bytes]      decode blocks (received, in array order)
 *   rows      [groups][k]                   decode rows (the Block.row fields)
 *
 * Return codes: 0 ok, -1 invalid parameters (as the reference), -2 GPU/runtime error.
 *
 * Large blocks. Any block_bytes % 8 == 0 is coded, as by the reference. The compile-time and tile
 * kernels address a workgroup's groups through 32-bit offsets below 2 GiB, which holds while
 *   n * max(k, m) * block_bytes <= 0x7FFFFFFF,  n = 511 / nq + 2,
 *   nq = block_bytes / 8 bytes in 4-byte columns, rounded up to a multiple of 4
 * (from block_bytes = 16,264 on: 2 * max(k, m) * block_bytes <= 0x7FFFFFFF; smaller blocks always
 * fit). Shapes past this bound run the generic kernels (64-bit addresses) in every call of this
 * header and in the single-group cauchy_256_encode / cauchy_256_decode, and cauchy_256_batch_path
 * reports 0 for them. The bound looks at (k, m, block_bytes) alone, never at `groups`.
 */
#ifndef SH_AMD_CAUCHY_256_BATCH_H
#define SH_AMD_CAUCHY_256_BATCH_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Select the device for this process (default 0) and initialise; 0 ok, -2 no GPU. */
int cauchy_256_batch_init(int device);

/* Encode every group: recovery[g] = cauchy_256_encode(k, m, data[g]). */
int cauchy_256_encode_batch(int k, int m, int block_bytes, int groups, const void *d_data,
                            void *d_recovery, void *stream);

/* Decode every group in place, exactly like cauchy_256_decode on (blocks[g], rows[g]). */
int cauchy_256_decode_batch(int k, int m, int block_bytes, int groups, void *d_blocks,
                            unsigned char *d_rows, void *stream);

/*
 * Out-of-place decode: blocks and rows are read only. Group g's recovered originals go to
 * d_out[g][0 .. e_g-1][block_bytes] (dense, emax = min(k, m) slots per group) in the order the
 * in-place call would write them (i-th recovery block in array order <- i-th smallest erasure);
 * d_out_rows[g][i] receives that erasure index and d_out_count[g] = e_g. m >= 2 only.
 * The unused slots are left untouched: no byte of d_out[g][e_g .. emax) or d_out_rows[g][e_g .. emax)
 * is written, for a group with e_g = 0 and for one flagged d_out_count[g] = -1 (below) the whole of
 * its emax slots, and nothing outside [groups][emax][block_bytes], [groups][emax] and [groups] is.
 * d_blocks, d_rows, d_out and d_out_rows take any address; d_out_count is an int array and must be
 * 4-byte aligned.
 */
int cauchy_256_decode_batch_out(int k, int m, int block_bytes, int groups, const void *d_blocks,
                                const unsigned char *d_rows, void *d_out, unsigned char *d_out_rows,
                                int *d_out_count, void *stream);

/*
 * Var-k batches: one launch for groups whose k differ (the caller closes a group with however
 * many packets were queued; m and block_bytes move slowly). Groups are described CSR-style by one
 * device array d_first[groups + 1]: group g owns blocks first[g] .. first[g+1]-1 of the packed
 * arrays, so k_g = first[g+1] - first[g]; its blocks start at byte first[g] * block_bytes of d_data
 * / d_blocks and its rows at byte first[g] of d_rows. Nothing is padded or aligned. total_blocks is
 * the host's copy of first[groups]: it bounds every access, so no call reads d_first on the host
 * and nothing synchronises.
 *   recovery  [groups][m][block_bytes]; a recovery block of group g carries row k_g + y
 *   out       [groups][emax][block_bytes], out_rows [groups][emax], emax = min(kmax, m)
 * Per-group semantics and bytes are those of cauchy_256_encode(k_g, m, ..) / cauchy_256_decode(k_g,
 * m, ..). The kernels are those cauchy_256_batch_path(kmax, m, block_bytes) reports, coding every
 * k_g <= kmax (the generator's column x is the same for every k).
 * As in the uniform call, out[g][e_g .. emax) and out_rows[g][e_g .. emax) are left untouched (all
 * emax slots of a group with e_g = 0 or d_out_count[g] = -1). d_first and d_out_count are int arrays
 * and must be 4-byte aligned; every other pointer takes any address.
 * Host-checked (-1, nothing enqueued): kmax in 2..255, kmax + m <= 256, block_bytes % 8 == 0,
 * groups >= 0, 0 <= total_blocks <= groups * kmax, m >= 1 (encode) / m >= 2 (decode).
 * Malformed groups -- k_g outside 2..kmax, or a span that leaves [0, total_blocks] -- are seen only
 * by the device: nothing of them is read, encode writes all-zero recovery blocks, decode sets
 * d_out_count[g] = -1, each is counted by cauchy_256_batch_errors(stream), and the other groups
 * are coded as usual. (In a batch above 2 GiB whose malformed groups make first[] jump by more
 * than 2 GiB inside one 128-column tile, the well-formed groups beyond the jump read as zeros.)
 */
int cauchy_256_encode_batch_var(int kmax, int m, int block_bytes, int groups, const int *d_first,
                                int total_blocks, const void *d_data, void *d_recovery, void *stream);
int cauchy_256_decode_batch_out_var(int kmax, int m, int block_bytes, int groups, const int *d_first,
                                    int total_blocks, const void *d_blocks, const unsigned char *d_rows,
                                    void *d_out, unsigned char *d_out_rows, int *d_out_count,
                                    void *stream);

/* Pre-allocate the internal decode workspace so later calls allocate nothing (graph capture).
 * A reserve for (kmax, m, block_bytes, groups) is sufficient for a later
 * cauchy_256_decode_batch_out_var with those parameters: it allocates nothing either.
 * Workspaces are per stream (decodes in flight on different streams never share scratch):
 * cauchy_256_batch_reserve sizes the null stream's workspace and the minimum size of every
 * workspace created later; cauchy_256_batch_reserve_stream does the same for `stream`. */
int cauchy_256_batch_reserve(int k, int m, int block_bytes, int groups);
int cauchy_256_batch_reserve_stream(int k, int m, int block_bytes, int groups, void *stream);

/* Malformed decode groups (more recovery blocks than erased originals: duplicate rows, outside
 * the reference's contract) are left untouched, counted, and flagged with d_out_count[g] = -1 by
 * cauchy_256_decode_batch_out. The var-k calls count their malformed groups (k_g outside 2..kmax,
 * a span outside [0, total_blocks]) in the same counter, encode and decode alike, on top of the
 * decode's malformed rows. Counts are kept per stream: this waits for `stream` and returns the
 * number of such groups among the decodes enqueued on `stream` since the previous call for that
 * stream (read and reset in stream order), or -2 on a GPU error. The single-group
 * cauchy_256_decode returns -1 for such a group and counts it nowhere (it decodes on a private
 * staging stream).
 * Every entry point runs on the library's device and restores the calling thread's current HIP
 * device before it returns. */
int cauchy_256_batch_errors(void *stream);

/* Synthetic workload: block x of group g0+g = PCG32 Seed((g0+g)*256 + x, cfg) words (the same
 * stream as the test oracle), written to d_out[groups][n][block_bytes]. */
int cauchy_256_fill_synthetic(void *d_out, int n, int block_bytes, int groups,
                              unsigned long long g0, unsigned long long cfg, void *stream);

/* Synthetic erasure pattern of group g (host only, no GPU): rows_out[0..k-1] = the decoder's
 * input rows (survivors ascending, then e chosen recovery rows k+y ascending), same stream as the
 * test oracle; e = e_fixed (clamped to min(k, m)) or PCG-random in [1, min(k, m)] when 0.
 * Returns e, or -1 on bad arguments. */
int cauchy_256_erasure_pattern(unsigned long long g, int k, int m, unsigned long long cfg, int e_fixed,
                               unsigned char *rows_out);

/* Which kernels code (k, m, block_bytes): 1 = compile-time-scheduled (generated for this (k, m), or
 * for a larger K of the same m with k >= 0.6 K, whose steps past k then read zeros),
 * 2 = the runtime-coefficient tile kernels (any other (k, m) with block_bytes/8 >= 16),
 * 0 = the generic per-column kernels (shorter blocks, and blocks past the 2 GiB span bound at the
 * top of this header), -1 = invalid parameters. Host-only: never
 * initialises the GPU. Before the library is initialised, 2 assumes the snippet table loaded
 * inside one 4 GB page (checked at launch, generic kernels otherwise); afterwards it includes it. */
int cauchy_256_batch_path(int k, int m, int block_bytes);

/* The library's stream (the batched calls' stream when they are passed a null stream) and a
 * synchronize helper for callers without HIP. The single-group calls use their own staging
 * streams (up to 8, one per concurrent call), so calls from different threads overlap. */
void *cauchy_256_default_stream(void);
int cauchy_256_sync(void *stream);

/* Measurement hooks (bench.py's roofline): after cauchy_256_profile(n), each batched decode on
 * the compile-time path records HIP events on its stream around its three kernels (the last n
 * decodes are kept; nothing synchronises while recording; n = 0 turns it off).
 * profile_read waits for them and returns ms[0..2] = mean setup, stage A and stage B times and
 * the number of decodes averaged (-1: none recorded). cauchy_256_profile(-n) records only the two
 * events around stage A (the headline's dominant kernel) of the last n decodes: ms[1] is then its
 * mean time and ms[0], ms[2] are -1. */
int cauchy_256_profile(int capacity);
int cauchy_256_profile_read(float *ms);

#ifdef __cplusplus
}
#endif

#endif /* SH_AMD_CAUCHY_256_BATCH_H */
