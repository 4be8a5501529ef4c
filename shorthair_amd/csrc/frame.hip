// Device-resident payload framing (include/shorthair_frame.h): the packet-to-block step of
// Encoder::EncodeQueued (Shorthair.cpp:540-557) and RecoverGroup (:710-735) as one streaming kernel.
//
// The output blocks[total_blocks][B] is one flat run of 8-byte words (B % 8 == 0, base 8-aligned).
// A lane owns two consecutive words of that run, placed so that the pair starts on a 16-byte
// boundary (`head` = 1 shifts the pairing by one word when the base is only 8-aligned): every store
// is one aligned 16-byte piece -- or one aligned 8-byte piece at the two ends of the run -- consecutive
// lanes write consecutive memory and no byte is written twice. The source side is byte-aligned only:
// a word is one unaligned 8-byte load, shifted and masked where the word is ragged (word 0 behind the
// 2-byte prefix, the word that straddles len).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes.hpp"
#include "frame.hpp"

namespace sh {
namespace {

constexpr int FRAME_THREADS = 256;
constexpr int FRAME_WORDS = 2 * FRAME_THREADS;  // output words per workgroup
constexpr int FRAME_MUL_NW = 4096;              // largest words-per-block divided by multiplication

// What one output word takes from the payload buffer: n bytes (0..8) starting at byte `at`, placed
// at byte `shl / 8` of the word, over the length prefix in word 0 of a framed block. A malformed block
// (shorthair_frame.h) takes nothing and has no prefix: all zeros.
struct WordPlan {
    long long at;
    int n, shl;
    uint32_t prefix;
    bool bad;
};

__device__ __forceinline__ WordPlan plan_word(const FrameArgs &a, long long off, int len, bool raw, int w) {
    WordPlan p;
    p.bad = (raw ? len != a.B : (len < 0 || len > min(a.B - 2, 65535))) || off < 0 || off > a.payload_bytes - len;
    const int a0 = raw ? 8 * w : 8 * w - 2;  // payload byte under byte 0 of this word
    const int lo = max(a0, 0);
    p.n = p.bad ? 0 : max(min(a0 + 8, len) - lo, 0);  // a raw block has len = B: always 8
    p.at = p.bad ? 0 : off + lo;
    p.shl = 8 * (lo - a0);  // 16 in word 0 of a framed block
    p.prefix = (!p.bad && !raw && w == 0) ? static_cast<uint32_t>(len) : 0;  // len <= 65535
    return p;
}

// The n bytes as the low bytes of a word: one unaligned 8-byte load of a window that covers them and
// stays inside the payload buffer -- pulled back from the buffer's end when the payload stops there,
// which only a ragged word (n < 8: word 0, or the word that straddles len) can need -- shifted down.
// Unconditional, so that a lane's two loads go out together: a word that takes nothing (zero padding,
// a malformed block) loads the buffer's first 8 bytes and masks them away. payload_bytes >= 8.
__device__ __forceinline__ uint64_t load_window(const FrameArgs &a, const WordPlan &p) {
    const long long ws = p.n > 0 ? min(p.at, a.payload_bytes - 8) : 0;
    const int shr = p.n > 0 ? 8 * static_cast<int>(p.at - ws) : 0;
    return ld64(a.payload + ws) >> shr;
}

// A payload buffer shorter than one word: byte by byte.
__device__ __forceinline__ uint64_t load_bytes(const FrameArgs &a, const WordPlan &p) {
    uint64_t x = 0;
    for (int i = 0; i < p.n; ++i) x |= static_cast<uint64_t>(a.payload[p.at + i]) << (8 * i);
    return x;
}

__device__ __forceinline__ uint64_t finish_word(const WordPlan &p, uint64_t x) {
    const uint64_t mask = p.n >= 8 ? ~0ull : (1ull << (8 * p.n)) - 1;
    return ((x & mask) << p.shl) | p.prefix;
}

__global__ __launch_bounds__(FRAME_THREADS) void frame_blocks(FrameArgs a) {
    // the workgroup's first word as (block, word): one wave-uniform 64-bit division
    const long long base = static_cast<long long>(blockIdx.x) * FRAME_WORDS - a.head;
    const long long wb = max(base, 0ll);
    const long long j0 = wb / a.nw;
    const int w0 = static_cast<int>(wb - j0 * a.nw);
    const long long f0 = base + 2 * static_cast<int>(threadIdx.x);  // this lane's words: f0, f0 + 1
    // both words in step -- descriptors, then plans, then the payload loads -- so that the loads of
    // one word do not wait for the other's
    bool ok[2];
    int j[2], w[2];
    for (int i = 0; i < 2; ++i) {
        const long long f = f0 + i;
        ok[i] = f >= 0 && f < a.total_words;
        const uint32_t l = ok[i] ? static_cast<uint32_t>(w0 + static_cast<int>(f - wb)) : 0;  // < nw + FRAME_WORDS
        const uint32_t q = a.mul ? __umulhi(l, a.mul) : l / static_cast<uint32_t>(a.nw);
        w[i] = static_cast<int>(l - q * a.nw);
        j[i] = ok[i] ? static_cast<int>(j0 + q) : 0;
    }
    // (a lane past either end of the run reads block 0's descriptor -- total_blocks > 0 -- and drops it)
    long long off[2];
    int len[2];
    bool raw[2] = {false, false};
    for (int i = 0; i < 2; ++i) {
        off[i] = a.off[j[i]];
        len[i] = a.len[j[i]];
    }
    if (a.raw)
        for (int i = 0; i < 2; ++i) raw[i] = a.raw[j[i]] != 0;
    WordPlan p[2];
    uint64_t x[2], v[2];
    for (int i = 0; i < 2; ++i) {
        p[i] = plan_word(a, off[i], len[i], raw[i], w[i]);
        if (!ok[i]) {
            p[i].n = 0;
            p[i].prefix = 0;
        }
    }
    if (a.payload_bytes >= 8)
        for (int i = 0; i < 2; ++i) x[i] = load_window(a, p[i]);
    else
        for (int i = 0; i < 2; ++i) x[i] = load_bytes(a, p[i]);
    for (int i = 0; i < 2; ++i) v[i] = finish_word(p[i], x[i]);
    uint8_t *dst = a.blocks + 8 * f0;
    if (ok[0] && ok[1]) {
        u64x2 o;
        o.x = v[0];
        o.y = v[1];
        *reinterpret_cast<u64x2 *>(dst) = o;
    } else if (ok[0]) {
        *reinterpret_cast<uint64_t *>(dst) = v[0];
    } else if (ok[1]) {
        *reinterpret_cast<uint64_t *>(dst + 8) = v[1];
    }
    // malformed blocks: the lane that owns a block's word 0 reports it; a ballot, then one atomicAdd
    // per wave (as var_check, kernels.hip)
    const int n = __popcll(__ballot(ok[0] && p[0].bad && w[0] == 0)) + __popcll(__ballot(ok[1] && p[1].bad && w[1] == 0));
    if (n && (threadIdx.x & 63) == 0) atomicAdd(a.errors, n);
}

}  // namespace

hipError_t launch_frame(FrameArgs a, hipStream_t stream) {
    if (a.total_blocks <= 0) return hipSuccess;
    a.nw = a.B / 8;
    a.total_words = static_cast<long long>(a.total_blocks) * a.nw;
    a.head = (reinterpret_cast<uintptr_t>(a.blocks) & 8) ? 1 : 0;
    a.mul = (a.nw >= 2 && a.nw <= FRAME_MUL_NW) ? static_cast<uint32_t>((1ull << 32) / a.nw) + 1 : 0;
    const long long wgs = (a.total_words + a.head + FRAME_WORDS - 1) / FRAME_WORDS;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(frame_blocks, dim3(static_cast<unsigned>(wgs)), dim3(FRAME_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sh
