// Common scaffolding for the compile-time-scheduled kernels generated into csrc/gen/.
//
// A generated file (fixed_<name>.inc) defines `run_<name>_p<p>(src, sink)` -- straight-line
// window-table XORs with the generator coefficients baked in, one step per input block -- and
// fixed_<name>_{enc,dec}.hip instantiate one kernel each through FIXED_KERNEL below.
//
// Work decomposition. Lanes are flattened over (group g, word column q): a lane owns bytes
// 4q..4q+3 of all 8 sub-blocks of a group ("bitsliced": each bit position is an independent
// column of the bitmatrix product). A workgroup covers COLS = CW*64 consecutive columns with
// CW column-waves x P part-waves; part p produces output rows [p*rows, (p+1)*rows). The CW waves
// of one part execute the same straight-line code in lockstep, sharing instruction fetch.
//
// Input staging (LDS ring, filled by LDS-DMA). Input block x of all the workgroup's columns is
// one ring slot laid out [sub-block a][column c] (words), so a lane's 8 words of step x are 8
// conflict-free ds_read_b32 at compile-time offsets. The slot is filled by `buffer_load_dwordx4
// ... lds`: per-lane global source addresses gather each sub-block's (at B=1400: 175-byte) span
// into the aligned LDS image, so misalignment costs nothing in the compute loop. Measured on
// gfx950 (tools/dma_probe.hip): misaligned LDS-DMA sources are exact; a dword straddling the
// buffer's num_records reads as 0.
//
// Pipeline (R slots, a workgroup barrier every S blocks). Iteration x issues the ds_reads of
// block x+1 into the second register set and computes block x from the registers read one
// iteration earlier (LDS latency under the compute). Before reading the first block of each
// group of S, a wave waits (counted vmcnt) for its DMAs of the whole group and joins the barrier
// -- every wave's share of those slots has landed, and every wave is past block x-1, so the
// slots of blocks <= x-1 are free and their DMAs (blocks up to x+R-1) are issued right there.
// R >= 2S+1 keeps R-2S-1 blocks of DMA in flight beyond the group being waited for. Fewer
// barriers matter: measured per-wave stamps (round 1) showed 41 % of a wave's life at the barrier
// with S = 1; S = 4 is 6-8 % faster. All P part-waves read the same slots:
// HBM sees each input byte once.
//
// Sub-block tails. When sub = B/8 is not a multiple of 4 (175 at B = 1400) the last 4-column
// chunk of every sub-block is shifted back by shift = 4*nq - sub bytes, on input (DMA source)
// and output (store offset) alike: its 4 lanes compute bytes [sub-16, sub) instead of
// [4nq-16, 4nq). Every word a lane computes is then a real column, every store is a plain dword
// store, nothing reads or writes past a sub-block, and the first shift bytes of the chunk are
// written twice with identical values (also by the column before it).
//
// Addressing. Buffer descriptors are built per workgroup with the base at the workgroup's first
// group, so 32-bit offsets cover any batch (no 2 GiB launch split); num_records stops at the end
// of the batch.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "geometry.hpp"

namespace sh {
namespace fixed {

#define X3(a, b, c) __builtin_amdgcn_bitop3_b32((a), (b), (c), 0x96)
// Zero-instruction pin of 8 accumulators to the current program point (see the generator).
#define PIN8(r)                                                                                    \
    asm volatile("" : "+v"(r[0]), "+v"(r[1]), "+v"(r[2]), "+v"(r[3]), "+v"(r[4]), "+v"(r[5]),      \
                 "+v"(r[6]), "+v"(r[7]))
#define ZERO(r) asm volatile("v_mov_b32 %0, 0" : "=v"(r))
// 2-input XOR as a bitop3 (third operand ignored): opaque to LLVM's reassociation.
#define X2(a, b) __builtin_amdgcn_bitop3_b32((a), (b), (a), 0x3C)
// acc ^= t as a 4-byte VOP2 v_xor_b32 (half the bytes of a bitop3: the straight-line schedules
// are instruction-fetch heavy); a non-volatile asm is opaque to reassociation yet schedulable.
#define XV(acc, t) asm("v_xor_b32 %0, %1, %2" : "=v"(acc) : "v"(t), "v"(acc))

// Cache policy of the output stores and of the input DMA (aux operand of the buffer op).
#ifndef SH_STORE_AUX
#define SH_STORE_AUX 0
#endif
#ifndef SH_LOAD_AUX
#define SH_LOAD_AUX 0
#endif

typedef __attribute__((address_space(3))) void lds_void;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32_ua __attribute__((aligned(1)));  // byte-aligned dword (LDS reads it unaligned)
constexpr uint32_t OOR = 0x80000000u;  // buffer offset past every descriptor's range (< 2 GiB)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const uint8_t *p, uint32_t bytes) {
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<uint8_t *>(p), static_cast<short>(0),
                                             static_cast<int>(bytes), 0x00020000);
}

__device__ __forceinline__ uint32_t bload(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
    return __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, 0);
}

// Descriptor over [base + first*gstride, base + total) capped below 2 GiB.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t wg_rsrc(const uint8_t *base, long long total,
                                                          long long gstride, int first) {
    const long long start = static_cast<long long>(first) * gstride;
    long long n = total - start;
    n = n < 0 ? 0 : (n > 0x7FFFFFFFll ? 0x7FFFFFFFll : n);
    return make_rsrc(base + start, static_cast<uint32_t>(n));
}

// XCD-aware tile order. Workgroups are dealt round-robin over the 8 XCDs (block b -> XCD b % 8;
// a speed assumption, never a correctness one). Adjacent column tiles usually split a group, so
// both read the same 128-byte lines at their shared edge; giving them blocks b and b + 8 puts
// them on one XCD at about the same time, and the second read hits that XCD's L2 instead of
// going to HBM again (measured: 29% over-fetch on the staging microbenchmark without it; a
// persistent variant that walked each workgroup's own group range tile by tile re-read those
// lines from memory: +30% FETCH_SIZE, 0.94 vs 0.75 ms, round 2). Bijective map of block b in
// [0, n) to a tile: XCD i gets the contiguous tile range [start_i, start_i + count_i),
// count_i = n/8 (+1 for the first n%8 XCDs).
__device__ __forceinline__ int xcd_tile(int b, int n) {
    const int q = n >> 3, r = n & 7;
    const int x = b & 7, i = b >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// Compile-time shape of one kernel instance.
// DMA_ = false only in measurement builds (tools/gen_fixed_kernels.py SH_GEN_ABLATE=nodma).
template <int K_, int M_, int P_, int CW_, int R_, bool DMA_ = true>
struct Shape {
    static constexpr int K = K_, M = M_, P = P_, CW = CW_, R = R_, W = 16;
    static constexpr bool DMA = DMA_;
    static constexpr int NW = CW * P, NT = 64 * NW, COLS = CW * 64;
    static constexpr int ROWB = COLS * 4;               // bytes of one sub-block row of a slot
    static constexpr int IMG = 8 * ROWB;                // bytes of one ring slot (one input block)
                                                        // and of one epilogue row image
    static constexpr int NDMA = IMG / (64 * W);         // DMA wave-instructions per step
    static constexpr int DPW = (NDMA + NW - 1) / NW;    // ... issued by each wave (at most)
    static constexpr int KP = (K + 3) & ~3, MP = (M + 3) & ~3;
    // <= 64 KB: two workgroups per CU, and ds_read's 16-bit offsets reach every slot; the 16-wave
    // shapes (one workgroup per CU) take 128 KB (slot offsets past 64 KB cost an address add)
    static_assert(R >= 3 && R * IMG <= 131072, "ring size");
};

// Per-lane geometry shared by the source and the sink.
struct WGInfo {
    long long col0;  // first column of the tile (may precede lo: the first tile of odd workgroups)
    long long lo, hi;  // this workgroup's columns [lo, hi): whole groups
    int g_first;     // group of max(col0, lo) (descriptor base)
    int wave, lane, c;
    int gl, q;       // this lane's group (relative to g_first) and word column
    bool valid;      // g < groups
};

// Input side. DMA instruction i = wave*DPW + j covers slot bytes [i*1024, (i+1)*1024): lane byte
// `off` -> sub-block a = off / ROWB, first column cc = (off % ROWB) / 4, a 4-column chunk that
// lies in one group because nq % 4 == 0 (has_fixed).
// Byte offset of word column q inside a sub-block (the last chunk shifted back, see above).
__device__ __forceinline__ uint32_t col_off(int q, const Geometry &geo) {
    return 4u * q - (q >= geo.nq - 4 ? static_cast<uint32_t>(4 * geo.nq - geo.sub) : 0u);
}

// Per-lane geometry of the tile starting at column col0.
template <class S>
__device__ __forceinline__ WGInfo tile_info(int nq, long long col0, long long lo, long long hi) {
    WGInfo w;
    w.wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    w.lane = threadIdx.x & 63;
    const int cw = w.wave / S::P;
    w.c = cw * 64 + w.lane;
    w.col0 = col0;
    w.lo = lo;
    w.hi = hi;
    w.g_first = static_cast<int>((col0 > lo ? col0 : lo) / nq);
    const long long col = w.col0 + w.c;
    w.valid = col >= lo && col < hi;
    const int g = w.valid ? static_cast<int>(col / nq) : w.g_first;
    w.q = static_cast<int>(col - static_cast<long long>(g) * nq);
    w.gl = g - w.g_first;
    return w;
}

// Var-k batches (FixedArgs::first): the window of a tile's input. The tile's groups are packed
// blocks first[g] .. first[g + 1] - 1, so its buffer descriptor starts at the lowest first block
// among the tile's well-formed groups (the same value in every lane of the workgroup) and the chunk
// offsets are relative to it. INT_MAX: the tile has no well-formed group.
__device__ __forceinline__ int var_window(const FixedArgs &a, int g_first, int kmax) {
    int lo = 0x7FFFFFFF;
    for (int i = threadIdx.x & 63; i < a.groups_per_wg; i += 64) {
        int f, k;
        if (g_first + i < a.groups && var_group(a.first, g_first + i, kmax, a.total_blocks, f, k)) lo = min(lo, f);
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) lo = min(lo, __shfl_xor(lo, d));
    return __builtin_amdgcn_readfirstlane(lo);
}

// Var-k batches: offset of group gx's first block from the window f0 (OOR: malformed, outside the
// workgroup's columns (`in` false), or ending past the descriptor's 2 GiB) and its k (0 then).
// The host routes every shape with groups_per_wg * kmax * B > 0x7FFFFFFF to the generic kernels
// (stagea_span_fits, stagea_route.hpp), and a tile's well-formed groups are consecutive blocks, so
// the 2 GiB test below is reachable only where malformed groups make first[] jump inside a tile
// (include/cauchy_256_batch.h says what the groups beyond the jump then read).
__device__ __forceinline__ uint32_t var_base(const FixedArgs &a, int gx, bool in, int kmax, int f0, int &kg) {
    int f = 0;
    kg = 0;
    if (!in || !var_group(a.first, gx, kmax, a.total_blocks, f, kg)) return OOR;
    const long long rel = (static_cast<long long>(f) - f0) * a.geo.B;
    if (rel < 0 || rel + static_cast<long long>(kg) * a.geo.B > 0x7FFFFFFFll) {
        kg = 0;
        return OOR;
    }
    return static_cast<uint32_t>(rel);
}

// VAR: the var-k source form (FixedArgs::first). A chunk's group base is (first[g] - window) * B
// instead of gl * in_gstride, and encode's zero-step test is per chunk (the k of its group);
// malformed groups read nothing. Everything else, and the whole VAR = false form, is unchanged.
template <class S, bool DEC, bool VAR = false>
struct Src {
    __amdgpu_buffer_rsrc_t rsrc;
    uint32_t dbase[S::DPW];   // chunk source offset, block 0 / array slot 0 (OOR past the batch)
    int dgl[S::DPW];          // decode: the chunk's group (position-table index)
    int kc[S::DPW];           // VAR encode: k of the chunk's group (its steps x >= kc read zeros)
    uint32_t B;
    int wave;
    uint32_t rd;              // this lane's read offset in a slot (c * 4)
    const uint8_t *lds;       // ring base
    const uint8_t *pos;       // decode: [groups_per_wg][KP + MP] position tables (LDS)
    int krt = S::K;           // encode: steps x >= krt (FixedArgs::k_rt) read zeros

    __device__ __forceinline__ static void chunk_src(const Geometry &geo, long long in_gstride_, const WGInfo &w,
                                                     uint32_t (&db)[S::DPW], int (&gl)[S::DPW]) {
        const uint32_t gstride = static_cast<uint32_t>(in_gstride_);
#pragma unroll
        for (int j = 0; j < S::DPW; ++j) {
            const int off = (w.wave * S::DPW + j) * 64 * S::W + w.lane * S::W;
            const int aa = off / S::ROWB;
            const int cc = (off - aa * S::ROWB) / 4;
            const long long colx = w.col0 + cc;
            const int gx = colx >= 0 ? static_cast<int>(colx / geo.nq) : -1;
            const int qx = static_cast<int>(colx - static_cast<long long>(gx) * geo.nq);
            gl[j] = gx - w.g_first;
            db[j] = (colx >= w.lo && colx < w.hi)
                        ? static_cast<uint32_t>(gx - w.g_first) * gstride + col_off(qx, geo) + aa * geo.sub
                        : OOR;
        }
    }

    __device__ __forceinline__ void init_var(const FixedArgs &a, const WGInfo &w) {
        const Geometry &geo = a.geo;
        const int kmax = a.k_rt > 0 ? a.k_rt : S::K;
        int f0 = var_window(a, w.g_first, kmax);
        if (f0 == 0x7FFFFFFF) f0 = 0;  // no well-formed group: every chunk below is OOR
        const long long start = static_cast<long long>(f0) * geo.B;
        long long n = a.in_bytes - start;
        n = n < 0 ? 0 : (n > 0x7FFFFFFFll ? 0x7FFFFFFFll : n);
        rsrc = make_rsrc(a.in + start, static_cast<uint32_t>(n));
#pragma unroll
        for (int j = 0; j < S::DPW; ++j) {
            const int off = (w.wave * S::DPW + j) * 64 * S::W + w.lane * S::W;
            const int aa = off / S::ROWB;
            const int cc = (off - aa * S::ROWB) / 4;
            const long long colx = w.col0 + cc;
            const int gx = colx >= 0 ? static_cast<int>(colx / geo.nq) : -1;
            const int qx = static_cast<int>(colx - static_cast<long long>(gx) * geo.nq);
            dgl[j] = gx - w.g_first;
            const uint32_t gb = var_base(a, gx, colx >= w.lo && colx < w.hi, kmax, f0, kc[j]);
            dbase[j] = gb == OOR ? OOR : gb + col_off(qx, geo) + aa * geo.sub;
        }
    }

    __device__ __forceinline__ void init(const FixedArgs &a, const WGInfo &w, const uint8_t *lds_ring,
                                         const uint8_t *lds_pos) {
        if constexpr (!VAR) rsrc = wg_rsrc(a.in, a.in_bytes, a.in_gstride, w.g_first);
        B = a.geo.B;
        lds = lds_ring;
        pos = lds_pos;
        wave = w.wave;
        rd = static_cast<uint32_t>(w.c) * 4u;
        if constexpr (!VAR) chunk_src(a.geo, a.in_gstride, w, dbase, dgl);
        krt = a.k_rt > 0 ? a.k_rt : S::K;
        if constexpr (VAR) init_var(a, w);
    }

    // Wait until this wave's DMAs of steps <= T are done (I = steps issued so far), then join the
    // workgroup barrier. One asm statement: nothing is scheduled between the two. Waves that
    // issue no DMA (NDMA < NW) only join the barrier: their vmcnt holds nothing but output
    // stores, which nothing here needs to wait for.
    template <int T, int I>
    __device__ __forceinline__ void wait() const {
        constexpr int N = (I - T - 1) * S::DPW;
        static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
        if (S::NDMA % S::NW != 0 && wave * S::DPW >= S::NDMA)
            asm volatile("s_barrier" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(N) : "memory");
    }

    // After the last step: every wave's reads of the ring are done before any wave writes its
    // store scratch (which aliases the ring).
    __device__ __forceinline__ static void release() {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }

    // Decode: the DMA source of a step depends on the group's position table (LDS): entry t < KP
    // is the array index of original column t, entry KP + y that of recovery row y (0xFF =
    // absent). pre(t) reads it one iteration before issue(x, .) needs it, so the DMA issue never
    // waits on LDS latency.
    struct Pre {
        int p[S::DPW];
    };
    __device__ __forceinline__ Pre pre(int t) const {
        Pre r;
#pragma unroll
        for (int j = 0; j < S::DPW; ++j) r.p[j] = DEC ? pos[dgl[j] * (S::KP + S::MP) + t] : 0;
        return r;
    }

    // The position entries of up to 4 consecutive steps t..t+3 in one (byte-unaligned) LDS read,
    // taken one burst of DMA issues ahead: the issues of a burst then never wait on LDS (one
    // ds_read_u8 per step, each consumed by the next issue, put an LDS latency between every two
    // DMAs of a burst). The table has 4 bytes of padding past its last group.
    struct Pre4 {
        uint32_t w[S::DPW];
    };
    __device__ __forceinline__ Pre4 pre4(int t) const {
        Pre4 r;
#pragma unroll
        for (int j = 0; j < S::DPW; ++j) {
            r.w[j] = 0;
            if (DEC) r.w[j] = *reinterpret_cast<const u32_ua *>(pos + dgl[j] * (S::KP + S::MP) + t);
        }
        return r;
    }
    __device__ __forceinline__ void issue4(int x, const Pre4 &p4, int i) const {
        Pre r;
#pragma unroll
        for (int j = 0; j < S::DPW; ++j) r.p[j] = static_cast<int>((p4.w[j] >> (8 * i)) & 0xFFu);
        issue(x, r);
    }

    // DMA of step x into its ring slot (encode: input block x).
    __device__ __forceinline__ void issue(int x, const Pre &pr) const {
        uint8_t *slot = const_cast<uint8_t *>(lds) + (x % S::R) * S::IMG;
#pragma unroll
        for (int j = 0; j < S::DPW; ++j) {
            if (S::NDMA % S::NW != 0 && wave * S::DPW + j >= S::NDMA) break;  // uniform
            lds_void *dst = (lds_void *)(slot + (wave * S::DPW + j) * 64 * S::W);
            if (DEC) {
                const int p = pr.p[j];
                const uint32_t o = (p == 0xFF || dbase[j] == OOR) ? OOR : dbase[j] + static_cast<uint32_t>(p) * B;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, S::W, o, 0, 0, SH_LOAD_AUX);
            } else {
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, dst, S::W, x < (VAR ? kc[j] : krt) ? dbase[j] : OOR,
                                                         static_cast<uint32_t>(x) * B, 0, SH_LOAD_AUX);
            }
        }
    }

    __device__ __forceinline__ void read(int slot, uint32_t &d0, uint32_t &d1, uint32_t &d2,
                                         uint32_t &d3, uint32_t &d4, uint32_t &d5, uint32_t &d6,
                                         uint32_t &d7) const {
        const uint8_t *p = lds + slot * S::IMG + rd;
        d0 = *reinterpret_cast<const uint32_t *>(p + 0 * S::ROWB);
        d1 = *reinterpret_cast<const uint32_t *>(p + 1 * S::ROWB);
        d2 = *reinterpret_cast<const uint32_t *>(p + 2 * S::ROWB);
        d3 = *reinterpret_cast<const uint32_t *>(p + 3 * S::ROWB);
        d4 = *reinterpret_cast<const uint32_t *>(p + 4 * S::ROWB);
        d5 = *reinterpret_cast<const uint32_t *>(p + 5 * S::ROWB);
        d6 = *reinterpret_cast<const uint32_t *>(p + 6 * S::ROWB);
        d7 = *reinterpret_cast<const uint32_t *>(p + 7 * S::ROWB);
    }

};

// Output assembled per row across the part's CW column-waves, so every store instruction writes
// 64 consecutive 16-byte pieces of the output in MEMORY order (about 1 KB contiguous): the
// CW waves of a part write their words of row y into a shared LDS row image laid out like a ring
// slot ([sub-block][tile column]), meet at a workgroup barrier, and each then stores 128 pieces
// taken from the image in memory order -- group by group over the tile, sub-block by sub-block,
// 4-column chunk by chunk. A group whose columns all lie in the tile is written as one
// contiguous m*B span by one workgroup within a few microseconds; only the groups split between
// two tiles are written as per-sub-block runs. (A per-wave transposition, round 2's store path,
// stored 8 runs of <= 176 bytes per instruction: the encode kernel was 3 % slower with it.) Row images are double-buffered by row parity: a wave
// reads row y's image before it joins row y+1's barrier, so row y+2 may overwrite it.
// Every wave of the workgroup joins one barrier per row of the largest part (pad() for the
// shorter parts). The images ([2][P][IMG] bytes) alias the ring (after Src::release()).
template <class S>
struct RowSink {
    __amdgpu_buffer_rsrc_t rsrc;
    mutable uint32_t gdst[2];  // per piece: destination offset without the row term (OOR: none)
    mutable uint32_t lsrc[2];  // per piece: byte offset inside a row image
    mutable uint32_t wofs;     // this lane's word in a row image (tile column * 4)
    uint32_t B;
    uint8_t *img;              // this part's row image, even rows (odd rows: + P * IMG)
    // uniform state (SGPRs): prepare() derives the per-lane offsets at the epilogue, so they
    // are not live across the body
    long long col0, lo, hi;
    uint32_t out_gstride;
    int g_first, nq, sub;

    __device__ __forceinline__ void init(const FixedArgs &a, const WGInfo &w, int part, uint8_t *lds) {
        rsrc = wg_rsrc(a.out, a.out_bytes, a.out_gstride, w.g_first);
        B = a.geo.B;
        img = lds + part * S::IMG;
        col0 = w.col0;
        lo = w.lo;
        hi = w.hi;
        out_gstride = static_cast<uint32_t>(a.out_gstride);
        g_first = w.g_first;
        nq = a.geo.nq;
        sub = a.geo.sub;
    }
    // Per-lane piece offsets of the tile (called right before the first row).
    __device__ __forceinline__ void prepare() const {
        const int lane = threadIdx.x & 63;
        const int cw = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) / S::P;
        wofs = static_cast<uint32_t>(cw * 64 + lane) * 4u;
        const long long cs = col0 > lo ? col0 : lo;
        const long long ce = col0 + S::COLS < hi ? col0 + S::COLS : hi;
        Geometry geo;
        geo.B = static_cast<int>(B);
        geo.sub = sub;
        geo.nq = nq;
        geo.tail = 4;
        // Groups overlapping the tile: the first (from column cs) and the last may be partial, every
        // one between is whole (8 * nq / 4 = 2 * nq pieces). O(1) per piece: the round-4 walk over
        // the tile's groups cost up to 64 iterations of 64-bit arithmetic per piece at nq = 8
        // (B = 256: a 512-column tile spans 64 groups), a regression of (28,4,256).
        const long long g0 = cs / nq;
        const int qa0 = static_cast<int>(cs - g0 * nq);
        const int n0 = static_cast<int>(((ce < (g0 + 1) * nq ? ce : (g0 + 1) * nq) - cs) >> 2);  // chunks
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            int rem = (cw * 2 + h) * 64 + lane;  // piece index in memory order
            gdst[h] = OOR;
            lsrc[h] = 0;
            long long g;
            int b, q;
            bool ok;
            if (rem < 8 * n0) {
                g = g0;
                b = rem / n0;
                q = qa0 + 4 * (rem - b * n0);
                ok = true;
            } else {
                rem -= 8 * n0;
                const int gi = rem / (2 * nq);
                g = g0 + 1 + gi;
                rem -= gi * 2 * nq;
                const long long gend = (ce < (g + 1) * nq ? ce : (g + 1) * nq);
                const int ng = g * nq < ce ? static_cast<int>((gend - g * nq) >> 2) : 0;
                ok = rem < 8 * ng;
                b = ok ? rem / ng : 0;
                q = ok ? 4 * (rem - b * ng) : 0;
            }
            if (ok) {
                gdst[h] = static_cast<uint32_t>(g - g_first) * out_gstride +
                          col_off(q, geo) + static_cast<uint32_t>(b * geo.sub);
                lsrc[h] = static_cast<uint32_t>(b * S::ROWB) + static_cast<uint32_t>(g * nq + q - col0) * 4u;
            }
        }
    }
    // Row y's words into the row image (parity YI), barrier; then piece h of the image.
    template <int YI>
    __device__ __forceinline__ uint8_t *image(const uint32_t (&w)[8]) const {
        uint8_t *im = img + (YI & 1) * S::P * S::IMG;
#pragma unroll
        for (int b = 0; b < 8; ++b) *reinterpret_cast<uint32_t *>(im + b * S::ROWB + wofs) = w[b];
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        return im;
    }
    __device__ __forceinline__ u32x4 piece(const uint8_t *im, int h) const {
        return *reinterpret_cast<const u32x4 *>(im + lsrc[h]);
    }
    template <int YI>
    __device__ __forceinline__ void row(int y, const uint32_t (&w)[8]) const {
        const uint8_t *im = image<YI>(w);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            __builtin_amdgcn_raw_buffer_store_b128(piece(im, h), rsrc, gdst[h], static_cast<uint32_t>(y) * B, SH_STORE_AUX);
    }

    template <int YI>
    __device__ __forceinline__ void pad() const {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    }
};

// Sets up src/sink for the tile starting at column col0 (columns outside [lo, hi) are idle
// lanes) and returns this wave's part. The caller (the FIXED_KERNEL macro)
// then calls the generated run_<name> directly, so everything inlines into one function: a
// non-inlined body took `src` by reference through scratch and read the LDS ring with flat loads.
template <class S, bool DEC, class SrcT, class SinkT>
__device__ __forceinline__ int kernel_prologue(const FixedArgs &a, uint8_t *lds, SrcT &src,
                                               SinkT &sink, long long col0, long long lo, long long hi) {
    const WGInfo w = tile_info<S>(a.geo.nq, col0, lo, hi);
    const int part = w.wave % S::P;
    const int nq = a.geo.nq;
    // The row images of the epilogue alias the start of the ring: they are used only after the
    // last step, behind Src::release()'s barrier, so the ring gets that LDS as extra slots.
    uint8_t *lds_pos = lds + S::R * S::IMG;
    if (DEC) {
        const int ng = a.groups_per_wg;
        const int ghi = static_cast<int>(hi / nq);
        constexpr int TW = (S::KP + S::MP) / 4;
        for (int i = threadIdx.x; i < ng * TW; i += S::NT) {
            const int lg = i / TW, t = i - lg * TW;
            const int gg = w.g_first + lg;
            uint32_t v = 0xFFFFFFFFu;
            if (gg < ghi) {
                v = (t < S::KP / 4)
                        ? reinterpret_cast<const uint32_t *>(a.pos + gg * static_cast<long long>(S::KP))[t]
                        : reinterpret_cast<const uint32_t *>(a.rpos + gg * static_cast<long long>(S::MP))[t - S::KP / 4];
            }
            reinterpret_cast<uint32_t *>(lds_pos)[i] = v;
        }
        __syncthreads();
    }
    src.init(a, w, lds, lds_pos);
    sink.init(a, w, part, lds);
    return part;  // the generated body issues the ring's first DMAs
}

// Measurement builds only (SH_HSACO_DIR, fixed_dispatch.cpp): launch the kernel `tag` from a
// code object of that directory instead (tools/il_reorder.py layouts); *used = false: none.
hipError_t module_launch(const char *tag, const FixedArgs &a, unsigned blocks, unsigned threads, size_t lds,
                         hipStream_t s, bool *used);

// One tile per workgroup. VAR: the kernel is a var-k instantiation (it alone reads FixedArgs::first).
template <class S, bool DEC, bool VAR>
inline hipError_t launch_shape(FixedArgs a, hipStream_t s, void (*kern)(FixedArgs), const char *tag) {
    if (VAR != (a.first != nullptr)) return hipErrorNotSupported;
    a.groups_per_wg = (S::COLS - 1) / a.geo.nq + 2;
    // ring (the row images of the epilogue alias it)
    constexpr size_t ring = static_cast<size_t>(S::R) * S::IMG;
    static_assert(2 * S::P * S::IMG <= S::R * S::IMG, "row images must fit inside the ring");
    // (+4: Src::pre4 reads up to 3 bytes past the last group's table)
    const size_t lds = ring + (DEC ? static_cast<size_t>(a.groups_per_wg) * (S::KP + S::MP) + 4 : 0);
    const long long cols = static_cast<long long>(a.groups) * a.geo.nq;
    const unsigned blocks = static_cast<unsigned>((cols + S::COLS - 1) / S::COLS);
    if (tag) {
        bool used = false;
        const hipError_t e = module_launch(tag, a, blocks, S::NT, lds, s, &used);
        if (used) return e;
    }
    hipLaunchKernelGGL(kern, dim3(blocks), dim3(S::NT), lds, s, a);
    return hipGetLastError();
}

}  // namespace fixed
}  // namespace sh

// One kernel + launcher of a generated (k, m): MODE enc (DEC = false) or dec (DEC = true);
// MINW = waves per SIMD the registers are allocated for. The host routes shapes with
// nq % 4 != 0 (a 16-byte chunk could straddle two groups) or sub < 16 to the generic kernel.
// Workgroup b codes tile xcd_tile(b, grid), one tile each. The `tile < 0` exit is never taken
// (xcd_tile is a bijection onto [0, grid)), but the compiler cannot prove that: the test is part
// of the compiled kernels, FIXED_KERNEL_VAR's have none, and this is all that keeps the two macros
// from being one without a change to the device code.
#define FIXED_KERNEL(NAME, K, M, P, CW, R, MINW, MODE, DEC, DMA)                                  \
    namespace sh {                                                                                \
    namespace fixed {                                                                             \
    using Shape_##NAME##_##MODE = Shape<K, M, P, CW, R, DMA>;                                     \
    __global__ __launch_bounds__(64 * CW * P, MINW) void kern_##NAME##_##MODE(FixedArgs a) {      \
        extern __shared__ __attribute__((aligned(16))) uint8_t lds[];                             \
        using S = Shape_##NAME##_##MODE;                                                          \
        Src<S, DEC> src;                                                                          \
        RowSink<S> sink;                                                                          \
        const long long cols_ = static_cast<long long>(a.groups) * a.geo.nq;                      \
        const int tile = xcd_tile(blockIdx.x, gridDim.x);                                         \
        if (tile < 0) return;                                                                     \
        const long long c0 = static_cast<long long>(tile) * S::COLS;                              \
        const int part = kernel_prologue<S, DEC>(a, lds, src, sink, c0, 0, cols_);                \
        run_##NAME##_##MODE(part, src, sink);                                                     \
    }                                                                                             \
    hipError_t launch_##NAME##_##MODE(FixedArgs a, hipStream_t s) {                               \
        return launch_shape<Shape_##NAME##_##MODE, DEC, false>(a, s, kern_##NAME##_##MODE,        \
                                                               #NAME "_" #MODE);                  \
    }                                                                                             \
    }                                                                                             \
    }

// The var-k form of a generated (k, m) (FixedArgs::first, Src<S, DEC, true>): the same generated
// program over the per-group source, one tile per workgroup, as kern_<name>_<mode>v.
#define FIXED_KERNEL_VAR(NAME, K, M, P, CW, R, MINW, MODE, DEC)                                   \
    namespace sh {                                                                                \
    namespace fixed {                                                                             \
    using Shape_##NAME##_##MODE##v = Shape<K, M, P, CW, R>;                                       \
    __global__ __launch_bounds__(64 * CW * P, MINW) void kern_##NAME##_##MODE##v(FixedArgs a) {   \
        extern __shared__ __attribute__((aligned(16))) uint8_t lds[];                             \
        using S = Shape_##NAME##_##MODE##v;                                                       \
        Src<S, DEC, true> src;                                                                    \
        RowSink<S> sink;                                                                          \
        const long long cols_ = static_cast<long long>(a.groups) * a.geo.nq;                      \
        const long long c0 = static_cast<long long>(xcd_tile(blockIdx.x, gridDim.x)) * S::COLS;   \
        const int part = kernel_prologue<S, DEC>(a, lds, src, sink, c0, 0, cols_);                \
        run_##NAME##_##MODE(part, src, sink);                                                     \
    }                                                                                             \
    hipError_t launch_##NAME##_##MODE##v(FixedArgs a, hipStream_t s) {                            \
        return launch_shape<Shape_##NAME##_##MODE##v, DEC, true>(a, s, kern_##NAME##_##MODE##v,   \
                                                                 nullptr);                        \
    }                                                                                             \
    }                                                                                             \
    }
