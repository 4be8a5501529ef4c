// Device-resident delivery of recovered blocks (include/shorthair_unframe.h): the block-to-packet step
// of RecoverGroup (Shorthair.cpp:741-756) for a whole batch, as a variable-length compaction.
//
// Three launches, none of which waits on another workgroup:
//   unframe_lengths  a lane per slot: count, 2-byte prefix, len[]; the workgroup's in-tile exclusive
//                    scan of max(len, 0) goes to scratch (local[]), its sum to sums[tile]
//   unframe_scan     one workgroup turns sums[] into exclusive tile bases, UNFRAME_SCAN_PASS per pass
//                    with a running carry, and writes the total
//   unframe_copy     source-driven: a sub-group of L lanes per slot (L = the power of two that covers
//                    the block's 16-byte chunks, at most 32) reads the slot's descriptor once, off[s] =
//                    sums[tile] + local[s], and walks the chunks that hold payload, two per lane in step:
//                    a 16-byte load of chunk c (8-byte aligned, as blocks are), stored at off[s] + 16c - 2
//                    with one unaligned 16-byte store; the two ragged chunks (chunk 0 behind the prefix,
//                    the chunk that straddles 2 + p) go out as 8-byte words, the ragged word of each as
//                    4/2/1-byte stores. A lane stores only bytes of its own payload and reads none of the
//                    destination; a slot that delivers nothing costs its descriptor loads and no more.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shorthair_unframe.h"
#include "block_scan.hpp"
#include "bytes.hpp"
#include "unframe.hpp"

namespace sh {
namespace {

constexpr int UNFRAME_THREADS = 256;
constexpr int UNFRAME_TILE = SHORTHAIR_UNFRAME_TILE_SLOTS;  // slots per workgroup of unframe_lengths
constexpr int UNFRAME_SCAN_PASS = SHORTHAIR_UNFRAME_SCAN_PASS;
static_assert(UNFRAME_TILE == UNFRAME_THREADS && UNFRAME_SCAN_PASS == UNFRAME_THREADS, "a lane per slot / per sum");

// The block of slot s, in blocks from `out`.
__device__ __forceinline__ long long slot_block(const UnframeArgs &a, uint32_t s) {
    if (a.stride_blocks == a.emax) return s;
    const uint32_t g = s / static_cast<uint32_t>(a.emax);
    return g * a.stride_blocks + (s - g * a.emax);
}

__global__ __launch_bounds__(UNFRAME_THREADS) void unframe_lengths(UnframeArgs a) {
    __shared__ int wsum[UNFRAME_THREADS / 64];
    const uint32_t s = blockIdx.x * static_cast<uint32_t>(UNFRAME_TILE) + threadIdx.x;
    const bool in = s < static_cast<uint32_t>(a.slots);
    int len = -1;
    bool report = false;
    if (in) {
        const uint32_t g = s / static_cast<uint32_t>(a.emax), i = s - g * a.emax;
        const int c = a.count ? a.count[g] : a.emax;
        const bool bad = c < -1 || c > a.emax;  // -1: the decode's malformed flag, counted there
        report = bad && i == 0;
        if (!bad && static_cast<int>(i) < c) {
            const uint8_t *blk = a.out + (g * a.stride_blocks + i) * a.B;
            const uint32_t p = *reinterpret_cast<const uint16_t *>(blk);  // u16 LE
            len = p > static_cast<uint32_t>(a.B - 2) ? -2 : static_cast<int>(p);
        }
        a.len[s] = len;
    }
    const int v = max(len, 0);  // <= 65535: a tile sums to < 2^24
    const Scanned<int> sc = block_scan<UNFRAME_THREADS>(v, wsum);
    if (in) a.local[s] = sc.excl;
    if (threadIdx.x == 0) a.sums[blockIdx.x] = sc.total;
    // as var_check (kernels.hip): a ballot, then one atomicAdd per wave
    const int n = __popcll(__ballot(report));
    if (n && (threadIdx.x & 63) == 0) atomicAdd(a.errors, n);
}

__global__ __launch_bounds__(UNFRAME_THREADS) void unframe_scan(UnframeArgs a) {
    __shared__ long long wsum[UNFRAME_THREADS / 64];
    const long long total = scan_passes<UNFRAME_THREADS, UNFRAME_SCAN_PASS / UNFRAME_THREADS>(
        a.tiles, wsum, [&](long long t) { return a.sums[t]; },
        [&](long long t, long long base, long long) { a.sums[t] = base; });
    if (threadIdx.x == 0) {
        a.sums[a.tiles] = total;
        a.off[a.slots] = total;
    }
}

// Word w of a slot's block: its payload bytes -- block bytes [8w, 8w + 8) cut to [2, 2 + p) -- go to
// dst + 8w - 2, dst the slot's place in the packed buffer.
__device__ __forceinline__ void emit_word(uint8_t *dst, int w, int p, uint64_t x) {
    const int lo = max(8 * w, 2);
    store_bytes(dst + (lo - 2), x >> (8 * (lo - 8 * w)), min(8 * w + 8, 2 + p) - lo);
}

// Chunk c of a block: 16 bytes, or the block's last 8 when B % 16 == 8 (nothing is read past the block).
__device__ __forceinline__ u64x2 load_chunk(const uint8_t *src, int c, int B) {
    u64x2 x;
    if (16 * c + 16 <= B) {
        __builtin_memcpy(&x, src + 16 * c, 16);  // global_load_dwordx4 at an 8-byte aligned address
    } else {
        x.x = *reinterpret_cast<const uint64_t *>(src + 16 * c);
        x.y = 0;
    }
    return x;
}

// Chunk c holds payload (16c < 2 + p): whole, one 16-byte store; ragged, its one or two words.
__device__ __forceinline__ void emit_chunk(uint8_t *dst, int c, int p, u64x2 x) {
    if (c > 0 && 16 * c + 16 <= 2 + p) {
        __builtin_memcpy(dst + (16 * c - 2), &x, 16);  // unaligned global_store_dwordx4
        return;
    }
    emit_word(dst, 2 * c, p, x.x);
    if (16 * c + 8 < 2 + p) emit_word(dst, 2 * c + 1, p, x.y);
}

__global__ __launch_bounds__(UNFRAME_THREADS) void unframe_copy(UnframeArgs a) {
    const LaneSplit ls = lane_split(static_cast<long long>(blockIdx.x) * UNFRAME_THREADS + threadIdx.x, a.lshift);
    const bool ok = ls.item < a.slots;
    const uint32_t s = ok ? static_cast<uint32_t>(ls.item) : 0;  // (a lane past the last slot reads slot 0's descriptor and drops it)
    const int step = ls.step, sub = ls.sub;
    const int p = a.len[s];
    const long long off = a.sums[s / UNFRAME_TILE] + a.local[s];
    if (ok && sub == 0) a.off[s] = off;
    const bool over = p > 0 && off + p > a.capacity;  // not written at all
    const int chunks = (ok && p > 0 && !over) ? (2 + p + 15) >> 4 : 0;
    const uint8_t *__restrict__ src = a.out + slot_block(a, s) * a.B;
    uint8_t *__restrict__ dst = a.payload + off;
    for (int c = sub; c < chunks; c += 2 * step) {
        // two chunks in step, so that the load of one does not wait for the other's stores
        const int c1 = c + step;
        const bool two = c1 < chunks;
        const u64x2 x0 = load_chunk(src, c, a.B);
        u64x2 x1 = {0, 0};
        if (two) x1 = load_chunk(src, c1, a.B);
        emit_chunk(dst, c, p, x0);
        if (two) emit_chunk(dst, c1, p, x1);
    }
    // payloads that do not fit: the slot's first lane reports it
    const int e = __popcll(__ballot(ok && sub == 0 && over));
    if (e && (threadIdx.x & 63) == 0) atomicAdd(a.errors, e);
}

}  // namespace

long long unframe_scratch_bytes(long long slots) {
    const long long tiles = (slots + UNFRAME_TILE - 1) / UNFRAME_TILE;
    return 8 * (tiles + 1) + 4 * slots;
}

hipError_t launch_unframe(UnframeArgs a, void *scratch, hipStream_t stream) {
    if (a.groups <= 0) return hipSuccess;
    a.slots = a.groups * a.emax;
    a.tiles = (a.slots - 1) / UNFRAME_TILE + 1;
    a.lshift = lshift_for(a.B);
    a.sums = static_cast<long long *>(scratch);
    a.local = reinterpret_cast<int *>(a.sums + a.tiles + 1);
    // slots <= INT_MAX, 32 lanes each at most: always within a grid
    const long long wgs = ((static_cast<long long>(a.slots) << a.lshift) + UNFRAME_THREADS - 1) / UNFRAME_THREADS;
    hipLaunchKernelGGL(unframe_lengths, dim3(static_cast<unsigned>(a.tiles)), dim3(UNFRAME_THREADS), 0, stream, a);
    hipLaunchKernelGGL(unframe_scan, dim3(1), dim3(UNFRAME_THREADS), 0, stream, a);
    hipLaunchKernelGGL(unframe_copy, dim3(static_cast<unsigned>(wgs)), dim3(UNFRAME_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sh
