// Device-resident datagrams in send order (include/shorthair_tx.h): what Send (Shorthair.cpp:966-1022),
// SendCheckSymbol (:631-649) and Tick (:1079-1089) put on the wire, for a whole batch, as a
// variable-length gather.
//
// Three launches, none of which waits on another workgroup:
//   txd_lengths  a lane per datagram: the schedule entry, its slot's first[] pair and descriptor, the
//                payload's (off, len), a binary search of d_pong_at, the rule; class and length out, a
//                32-byte descriptor (header bytes, source, lengths) to scratch; the workgroup's in-tile
//                exclusive scan of the aligned lengths goes into the descriptor, its sum to sums[tile],
//                the tile's six class counts to tile_stat
//   txd_scan     one workgroup turns sums[] into exclusive tile bases, SHORTHAIR_TX_TILE_PASS per pass with
//                a running carry, and writes the total, d_state_out (it is the only kernel that reads the
//                state after txd_lengths and the only one that writes it, so in and out may alias), the
//                summary and the malformed count
//   txd_copy     source-driven: a sub-group of 1 << lshift lanes per datagram reads its descriptor once and
//                copies it (tx_datagram_copy.hpp); a datagram that does not fit is not written, and its
//                first lane corrects class, length and the summary
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "block_scan.hpp"
#include "tx_datagram.hpp"

namespace sh {
namespace {

constexpr int TXD_THREADS = 256;
constexpr int TXD_WAVES = TXD_THREADS / 64;
constexpr int TXD_TILE = SHORTHAIR_TX_TILE;
constexpr int TXD_TILE_PASS = SHORTHAIR_TX_TILE_PASS;
constexpr int TXD_STATS = 6;  // written, originals, recovery, holes, pong, malformed
constexpr int TXD_PER_LANE = TXD_TILE_PASS / TXD_THREADS;  // tile sums a lane of txd_scan takes per pass
static_assert(TXD_TILE == TXD_THREADS && TXD_TILE_PASS % TXD_THREADS == 0, "a lane per datagram, whole lanes");
static_assert(sizeof(TxDesc) == 32 && sizeof(ShorthairTxGroupDesc) == 16, "descriptor layouts");

// The payload j as a body: false when (off, len) is malformed by shorthair_tx.h step 4.
__device__ __forceinline__ bool payload_body(const TxDatagramArgs &a, int j, long long &src, int &blen) {
    const long long off = a.off[j];
    const int len = a.len[j];
    src = off;
    blen = len;
    return len >= 0 && len <= 65535 && off >= 0 && off <= a.payload_bytes - len;
}

__global__ __launch_bounds__(TXD_THREADS) void txd_lengths(TxDatagramArgs a) {
    __shared__ int wsum[TXD_WAVES];
    __shared__ int stat[TXD_STATS];
    if (threadIdx.x < TXD_STATS) stat[threadIdx.x] = 0;
    const uint32_t i = blockIdx.x * static_cast<uint32_t>(TXD_TILE) + threadIdx.x;
    const bool in = i < static_cast<uint32_t>(a.datagrams);
    int cls = -1, hlen = 0, blen = 0, rec = 0;
    long long src = 0;
    uint64_t h0 = 0, h1 = 0;
    if (in) {
        const int e = a.sched[i];
        const uint32_t seq = static_cast<uint32_t>(a.state_in[0] + static_cast<int>(i)) & 0xffffu;
        // the pong of datagram i, if d_pong_at lists it: lower bound by bisection
        int lo = 0, hi = a.n_pong;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (a.pong_at[mid] < static_cast<int>(i)) lo = mid + 1; else hi = mid;
        }
        const bool pong = lo < a.n_pong && a.pong_at[lo] == static_cast<int>(i);
        uint64_t seen = 0, total = 0;
        if (pong) {
            seen = a.pong_val[2 * lo];
            total = a.pong_val[2 * lo + 1];
        }
        // [seq u16][0x81][seen u32][total u32] = 11 bytes: 8 in p0, 3 in p1
        const uint64_t p0 = seq | (0x81ull << 16) | (seen << 24) | (total << 56);
        const uint64_t p1 = total >> 8;
        if (e == -1) {
            cls = 3;
            if (pong) {
                cls = 3 + 8;
                hlen = 11;
                h0 = p0;
                h1 = p1;
            }
        } else if (e >= 0 && (e >> 9) < a.groups) {
            const int g = e >> 9, x = e & 511;
            const int f0 = a.first[g], f1 = a.first[g + 1];
            const long long kk = static_cast<long long>(f1) - f0;
            const uint64_t g7 = static_cast<uint32_t>(a.state_in[1] + g) & 0x7fu;
            if (f0 >= 0 && f1 <= a.total && kk >= 1 && kk <= 255) {
                const int k = static_cast<int>(kk);
                if (x < 256) {
                    if (x < k && payload_body(a, f0 + x, src, blen)) {
                        // [g7][x][x] behind the sequence number, or behind the pong
                        const uint64_t t = g7 | (static_cast<uint64_t>(x) << 8) | (static_cast<uint64_t>(x) << 16);
                        if (pong) {
                            cls = 8;
                            hlen = 14;
                            h0 = p0;
                            h1 = p1 | (t << 24);
                        } else {
                            cls = 0;
                            hlen = 5;
                            h0 = seq | (t << 16);
                        }
                    }
                } else if (!pong) {
                    const int y = x - 256;
                    ShorthairTxGroupDesc d;
                    if (a.group) {
                        __builtin_memcpy(&d, &a.group[g], 16);  // one 16-byte load
                    } else {
                        d.rec_off = static_cast<long long>(g) * a.m * a.B;
                        d.m = a.m;
                        d.block_bytes = a.B;
                    }
                    if (d.m >= 1 && y < d.m && k + d.m <= 256) {
                        if (k == 1) {
                            if (payload_body(a, f0, src, blen)) {
                                cls = 2;
                                hlen = 5;
                                h0 = seq | (g7 << 16) | (1ull << 24);  // [g7][1][0]
                            }
                        } else if (d.block_bytes >= 8 && d.block_bytes % 8 == 0 &&
                                   d.block_bytes <= SHORTHAIR_TX_MAX_BLOCK_BYTES && d.rec_off >= 0 &&
                                   d.rec_off % 8 == 0 &&
                                   d.rec_off <= a.recovery_bytes - static_cast<long long>(d.m) * d.block_bytes) {
                            cls = 1;
                            hlen = 6;
                            rec = TXD_REC;
                            blen = d.block_bytes;
                            src = d.rec_off + static_cast<long long>(y) * d.block_bytes;
                            h0 = seq | (g7 << 16) | (static_cast<uint64_t>(k + y) << 24) |
                                 (static_cast<uint64_t>(k - 1) << 32) | (static_cast<uint64_t>(d.m - 1) << 40);
                        }
                    }
                }
            }
        }
        if (cls < 0) blen = 0;
    }
    const int L = hlen + blen;                        // <= SHORTHAIR_TX_MAX_DATAGRAM_BYTES
    const int v = (L + a.align - 1) & ~(a.align - 1);  // <= 69,632: a tile sums to < 2^25
    const Scanned<int> sc = block_scan<TXD_THREADS>(v, wsum);  // (its barrier also publishes stat[] = 0)
    if (in) {
        a.dg_len[i] = L;
        a.dg_class[i] = cls;
        TxDesc d;
        d.h0 = h0;
        d.h1 = h1;
        d.src = src;
        d.meta = blen | (hlen << TXD_HLEN_SHIFT) | rec;
        d.local = sc.excl;
        a.desc[i] = d;
    }
    if (threadIdx.x == 0) a.sums[blockIdx.x] = sc.total;
    // class counts: ballots, one LDS atomic per wave and class
    const bool flag[TXD_STATS] = {in && L > 0,      in && (cls == 0 || cls == 8), in && (cls == 1 || cls == 2),
                                  in && (cls & ~8) == 3 && cls >= 0, in && cls >= 8,              in && cls == -1};
#pragma unroll
    for (int c = 0; c < TXD_STATS; ++c) {
        const int n = __popcll(__ballot(flag[c]));
        if (n && (threadIdx.x & 63) == 0) atomicAdd(&stat[c], n);
    }
    __syncthreads();
    if (threadIdx.x < TXD_STATS) a.tile_stat[blockIdx.x * TXD_STATS + threadIdx.x] = stat[threadIdx.x];
}

__global__ __launch_bounds__(TXD_THREADS) void txd_scan(TxDatagramArgs a) {
    __shared__ long long wsum[TXD_WAVES];
    __shared__ int stat[TXD_STATS];
    if (threadIdx.x < TXD_STATS) stat[threadIdx.x] = 0;
    const int s0 = a.state_in[0], s1 = a.state_in[1];
    int mine[TXD_STATS] = {0, 0, 0, 0, 0, 0};
    const long long carry = scan_passes<TXD_THREADS, TXD_PER_LANE>(
        a.tiles, wsum,
        [&](long long t) {
#pragma unroll
            for (int c = 0; c < TXD_STATS; ++c) mine[c] += a.tile_stat[t * TXD_STATS + c];
            return a.sums[t];
        },
        [&](long long t, long long base, long long) { a.sums[t] = base; });
    __syncthreads();  // stat[] = 0 is visible, and every lane has read the state (out may alias in)
#pragma unroll
    for (int c = 0; c < TXD_STATS; ++c)
        if (mine[c]) atomicAdd(&stat[c], mine[c]);
    __syncthreads();
    if (threadIdx.x == 0) {
        a.sums[a.tiles] = carry;
        a.dg_off[a.datagrams] = carry;
        a.state_out[0] = s0 + a.datagrams;
        a.state_out[1] = s1 + a.advance;
        for (int c = 0; c < TXD_STATS; ++c) a.summary[c] = stat[c];
        a.summary[6] = 0;
        a.summary[7] = 0;
        if (stat[5]) atomicAdd(a.errors, stat[5]);
    }
}

__global__ __launch_bounds__(TXD_THREADS) void txd_copy(TxDatagramArgs a) {
    const LaneSplit ls = lane_split(static_cast<long long>(blockIdx.x) * TXD_THREADS + threadIdx.x, a.lshift);
    const bool ok = ls.item < a.datagrams;
    const uint32_t i = ok ? static_cast<uint32_t>(ls.item) : 0;  // (a lane past the last datagram reads datagram 0's descriptor and drops it)
    const TxDesc d = a.desc[i];
    const long long off = a.sums[i / TXD_TILE] + d.local;
    TxCopy c = txd_plan(d, a.payload, a.payload_bytes, a.recovery);
    const bool over = c.L > 0 && off > a.ring_bytes - c.L;  // not written at all
    const bool first = ok && ls.sub == 0;
    if (first) a.dg_off[i] = off;
    if (ok && !over) txd_copy_lane(c, a.ring + off, ls.sub, ls.step);
    // datagrams that do not fit: the first lane takes the class back out of the summary
    const unsigned long long b = __ballot(first && over);
    if (b) {  // wave-uniform
        int cls = 0;
        if (first && over) {
            cls = a.dg_class[i];
            a.dg_class[i] = -2;
            a.dg_len[i] = 0;
        }
        const int n = __popcll(b);
        const int n1 = __popcll(__ballot(first && over && (cls & ~8) == 0));
        const int n2 = __popcll(__ballot(first && over && ((cls & ~8) == 1 || (cls & ~8) == 2)));
        const int n3 = __popcll(__ballot(first && over && (cls & ~8) == 3));
        const int n4 = __popcll(__ballot(first && over && cls >= 8));
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(a.errors, n);
            atomicAdd(&a.summary[6], n);
            atomicSub(&a.summary[0], n);
            if (n1) atomicSub(&a.summary[1], n1);
            if (n2) atomicSub(&a.summary[2], n2);
            if (n3) atomicSub(&a.summary[3], n3);
            if (n4) atomicSub(&a.summary[4], n4);
        }
    }
}

}  // namespace

long long tx_datagram_scratch_bytes(long long datagrams) {
    const long long tiles = (datagrams + TXD_TILE - 1) / TXD_TILE;
    return 32 * datagrams + 8 * (tiles + 1) + 4 * TXD_STATS * tiles;
}

hipError_t launch_tx_datagram(TxDatagramArgs a, void *scratch, hipStream_t stream) {
    a.tiles = (a.datagrams + TXD_TILE - 1) / TXD_TILE;
    a.desc = static_cast<TxDesc *>(scratch);
    a.sums = reinterpret_cast<long long *>(a.desc + a.datagrams);
    a.tile_stat = reinterpret_cast<int *>(a.sums + a.tiles + 1);
    a.lshift = lshift_for(a.B > 0 ? a.B + 14 + 15 : 512);  // (15: a piece more where the destination is unaligned)
    if (a.tiles > 0) hipLaunchKernelGGL(txd_lengths, dim3(static_cast<unsigned>(a.tiles)), dim3(TXD_THREADS), 0, stream, a);
    hipLaunchKernelGGL(txd_scan, dim3(1), dim3(TXD_THREADS), 0, stream, a);
    if (a.tiles > 0) {
        // datagrams <= INT_MAX, 32 lanes each at most: always within a grid
        const long long wgs = ((static_cast<long long>(a.datagrams) << a.lshift) + TXD_THREADS - 1) / TXD_THREADS;
        hipLaunchKernelGGL(txd_copy, dim3(static_cast<unsigned>(wgs)), dim3(TXD_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace sh
