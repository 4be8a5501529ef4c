// Device-resident grouping of received datagrams (include/shorthair_rx.h, shorthair_rx_group_batch): the
// header rule of ShorthairCodec::Recv / OnOOB / OnData (Shorthair.cpp:1192-1211, :664-699, :766-780) and
// the 7-bit group expansion of Counter.h:297-316 for a whole batch of datagrams in GPU memory, in arrival
// order, and the CSR by group that shorthair_rx_list_batch reads.
//
// The expansion is a scan. A data datagram with partial p moves the group number u by s7(p - (u & 127)),
// after which u = p (mod 128). A run of datagrams is therefore the function
//     u -> u                                        without a data datagram
//     u -> u + s7(fp - (u & 127)) + sum             fp: its first partial, sum: the steps between its own
// and two runs compose into one of the same form (the first run ends at (fp + sum) & 127). That is the
// monoid `Agg` below; the "last valid partial" and the "sum of steps" are one scan over it.
//
// Six launches, none of which waits on another workgroup:
//   rxg_classify    a lane per datagram, a workgroup per tile of RXG_TILE: offset and length (coalesced),
//                   byte 2, byte 11 behind a pong. The code (kind, pong, h, p) goes to scratch, the tile's
//                   Agg to tile_fp / tile_sum. All lanes of the grid also clear the slot counters and
//                   write d_slot_group.
//   rxg_scan_tiles  one workgroup scans the tile Aggs, RXG_TILE_PASS tiles per pass with a running group
//                   number: tile_u[t] is the group number in front of tile t. Writes d_state_out, after it
//                   has copied d_state_in to scratch for the kernels behind it (the two may alias).
//   rxg_down        a workgroup per tile scans its datagrams' Aggs from tile_u[t]: u, the slot, the final
//                   class. A binned datagram takes a position in its slot from the slot's counter: the
//                   wave combines equal slots with ballots, one atomic per distinct slot. Per tile: the
//                   count of datagrams not binned and of the four summary classes.
//   rxg_scan_slots  one workgroup: the exclusive sums of tile_nb, the sums of tile_stat, then the slot
//                   counters into d_pkt_first, RXG_SLOT_PASS slots per pass as rx_scan does; d_summary and
//                   the error counter.
//   rxg_scatter     a workgroup per tile: a binned datagram's index goes to d_pkt_dg at d_pkt_first[slot] +
//                   position, any other to d_other at the tile's base + its rank in the tile (a workgroup
//                   scan, no atomics). The tails of the four lists.
//   rxg_order       a wave per slot: up to SHORTHAIR_RX_MAX_PACKETS datagram indices are ranked in LDS
//                   into ascending (= arrival) order; d_pkt_dg, d_pkt_off and d_pkt_len are written from
//                   them. Indices within RXG_SPAN of the slot's lowest -- a sender's interleaving -- are
//                   ranked through a bitmap (a bit per index, the rank is the popcount below); a wider
//                   spread by counting the indices below each. A longer slot keeps the counter's order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/shorthair_rx.h"
#include "block_scan.hpp"
#include "bytes.hpp"
#include "rx_group.hpp"

namespace sh {
namespace {

constexpr int RXG_THREADS = 256;
constexpr int RXG_WAVES = RXG_THREADS / 64;
constexpr int RXG_TILE = SHORTHAIR_RX_GROUP_TILE;
constexpr int RXG_TILE_PASS = SHORTHAIR_RX_GROUP_TILE_PASS;
constexpr int RXG_TILES_PER_LANE = RXG_TILE_PASS / RXG_THREADS;
constexpr int RXG_SLOT_TILE = SHORTHAIR_RX_GROUP_SLOT_TILE;
constexpr int RXG_SLOT_PASS = SHORTHAIR_RX_GROUP_SLOT_PASS;
constexpr int RXG_MAX = SHORTHAIR_RX_MAX_PACKETS;
constexpr int RXG_PER_LANE = RXG_MAX / 64;  // indices a lane of rxg_order ranks
constexpr int RXG_SPAN = 64 * 32;           // widest spread of a slot's datagram indices that rxg_order ranks by bitmap
static_assert(RXG_TILE == RXG_THREADS, "a lane per datagram");
static_assert(RXG_TILE_PASS % RXG_THREADS == 0 && RXG_SLOT_PASS == RXG_SLOT_TILE * RXG_THREADS, "whole lanes");
static_assert(RXG_MAX % 64 == 0, "whole waves");

// code in scratch: kind | pong << 4 | h << 8 | p << 16
constexpr int K_DATA = 0, K_OOB = 1, K_PONG = 2, K_SHORT = 3, K_WINDOW = 4, K_BAD = 7;
constexpr int PONG = 16;

__device__ __forceinline__ int s7(int x) { return ((x & 127) ^ 64) - 64; }

struct Agg {
    int fp, sum;  // fp < 0: no data datagram
};
__device__ __forceinline__ int add_wrap(int a, int b) {
    return static_cast<int>(static_cast<unsigned>(a) + static_cast<unsigned>(b));
}
__device__ __forceinline__ Agg combine(Agg a, Agg b) {
    if (a.fp < 0) return b;
    if (b.fp < 0) return a;
    const int last = add_wrap(a.fp, a.sum) & 127;
    return Agg{a.fp, add_wrap(add_wrap(a.sum, s7(b.fp - last)), b.sum)};
}
__device__ __forceinline__ int apply(int u, Agg a) {
    return a.fp < 0 ? u : add_wrap(add_wrap(u, s7(a.fp - (u & 127))), a.sum);
}
// block_scan and scan_passes over Aggs, in datagram order.
constexpr Agg AGG_NONE{-1, 0};
struct AggCombine {
    __device__ __forceinline__ Agg operator()(Agg a, Agg b) const { return combine(a, b); }
};

// Steps 1 to 3 for datagram i.
__device__ __forceinline__ int classify(const RxGroupArgs &a, long long i) {
    const long long off = a.dg_off[i];
    const int len = a.dg_len[i];
    if (len < 3 || off < 0 || off > a.ring_bytes - len) return K_BAD;
    const uint8_t *d = a.ring + off;
    const int f = d[2];
    int h = 2, b = f, pong = 0;
    if ((f & 0x80) && (f & 1)) {
        if (len < 11) return K_BAD;
        pong = PONG;
        if (len == 11) return K_PONG | pong;
        h = 11;
        b = d[11];
    }
    if (b & 0x80) return K_OOB | pong | (h << 8);
    if (len - h - 1 <= 2) return K_SHORT | pong | (h << 8);
    return K_DATA | pong | (h << 8) | ((b & 127) << 16);
}

__device__ __forceinline__ Agg code_agg(int code) { return (code & 15) == K_DATA ? Agg{(code >> 16) & 127, 0} : Agg{-1, 0}; }

__global__ __launch_bounds__(RXG_THREADS) void rxg_classify(RxGroupArgs a) {
    __shared__ Agg wagg[RXG_WAVES];
    const int state = a.state_in[0];
    const long long step = static_cast<long long>(gridDim.x) * RXG_THREADS;
    for (long long s = static_cast<long long>(blockIdx.x) * RXG_THREADS + threadIdx.x; s < a.groups; s += step) {
        a.cnt[s] = 0;
        a.slot_group[s] = add_wrap(add_wrap(state, -a.back), static_cast<int>(s));
    }
    if (static_cast<int>(blockIdx.x) >= a.tiles) return;
    const long long i = static_cast<long long>(blockIdx.x) * RXG_TILE + threadIdx.x;
    int code = K_BAD;  // (past the end: no data datagram)
    if (i < a.datagrams) {
        code = classify(a, i);
        a.code[i] = code;
    }
    const Agg total = block_scan<RXG_THREADS>(code_agg(code), wagg, AGG_NONE, AggCombine{}).total;
    if (threadIdx.x == 0) {
        a.tile_fp[blockIdx.x] = total.fp;
        a.tile_sum[blockIdx.x] = total.sum;
    }
}

__global__ __launch_bounds__(RXG_THREADS) void rxg_scan_tiles(RxGroupArgs a) {
    __shared__ Agg wagg[RXG_WAVES];
    const int u = a.state_in[0];
    __syncthreads();  // every lane has read the state before lane 0 writes d_state_out, which may alias it
    if (threadIdx.x == 0) a.hdr[0] = u;
    // the tiles in front of tile t compose into one Agg: applied to u, it gives the group number in front of t
    const Agg all = scan_passes<RXG_THREADS, RXG_TILES_PER_LANE>(
        a.tiles, wagg, [&](long long t) { return Agg{a.tile_fp[t], a.tile_sum[t]}; },
        [&](long long t, Agg in_front, Agg) { a.tile_u[t] = apply(u, in_front); }, AGG_NONE, AggCombine{});
    if (threadIdx.x == 0) a.state_out[0] = apply(u, all);
}

__global__ __launch_bounds__(RXG_THREADS) void rxg_down(RxGroupArgs a) {
    __shared__ Agg wagg[RXG_WAVES];
    __shared__ int wstat[RXG_WAVES][5];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int t = blockIdx.x;
    const long long i = static_cast<long long>(t) * RXG_TILE + threadIdx.x;
    const bool have = i < a.datagrams;
    const int code = have ? a.code[i] : K_BAD;
    const bool data = (code & 15) == K_DATA;
    const Agg incl = block_scan<RXG_THREADS>(code_agg(code), wagg, AGG_NONE, AggCombine{}).incl;
    // steps 4 and 5
    const int u = apply(a.tile_u[t], incl);
    const long long slot64 = static_cast<long long>(static_cast<int>(static_cast<unsigned>(u) - static_cast<unsigned>(a.hdr[0]))) + a.back;
    const bool binned = data && slot64 >= 0 && slot64 < a.groups;
    const int slot = binned ? static_cast<int>(slot64) : -1;
    const int kind = data && !binned ? K_WINDOW : code & 15;
    const bool pong = have && kind != K_BAD && (code & PONG);
    if (have) {
        a.dg_class[i] = kind == K_BAD ? -1 : kind + (pong ? 8 : 0);
        a.dg_slot[i] = slot;
    }
    // a position in the slot: one atomic per distinct slot of the wave
    int pos = 0;
    uint64_t todo = __ballot(binned);
    while (todo) {
        const int leader = __ffsll(static_cast<unsigned long long>(todo)) - 1;
        const int ls = __shfl(slot, leader);
        const uint64_t same = __ballot(binned && slot == ls);
        int base = 0;
        if (lane == leader) base = atomicAdd(&a.cnt[ls], __popcll(same));
        base = __shfl(base, leader);
        if (binned && slot == ls) pos = base + __popcll(same & lanes_below(lane));
        todo &= ~same;
    }
    if (binned) a.pos[i] = pos;
    // the tile's counts
    const int n_nb = __popcll(__ballot(have && !binned));
    const int n_bad = __popcll(__ballot(have && kind == K_BAD));
    const int n_win = __popcll(__ballot(kind == K_WINDOW));
    const int n_pong = __popcll(__ballot(pong));
    const int n_short = __popcll(__ballot(have && kind == K_SHORT));
    if (lane == 0) {
        wstat[wave][0] = n_nb;
        wstat[wave][1] = n_bad;
        wstat[wave][2] = n_win;
        wstat[wave][3] = n_pong;
        wstat[wave][4] = n_short;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        int v = 0;
        for (int w = 0; w < RXG_WAVES; ++w) v += wstat[w][threadIdx.x];
        if (threadIdx.x == 0) a.tile_nb[t] = v;
        else a.tile_stat[4 * static_cast<long long>(t) + threadIdx.x - 1] = v;
    }
}

__global__ __launch_bounds__(RXG_THREADS) void rxg_scan_slots(RxGroupArgs a) {
    __shared__ int wsum[RXG_WAVES];
    __shared__ int s_sum[8];  // d_summary
    if (threadIdx.x < 8) s_sum[threadIdx.x] = threadIdx.x == 2 ? a.groups : 0;
    __syncthreads();
    // the tiles: where each one's datagrams start in d_other, and the four class counts
    int st[4] = {0, 0, 0, 0};
    scan_passes<RXG_THREADS, RXG_TILES_PER_LANE>(
        a.tiles, wsum,
        [&](long long t) {
            for (int q = 0; q < 4; ++q) st[q] += a.tile_stat[4 * t + q];
            return a.tile_nb[t];
        },
        [&](long long t, int in_front, int) { a.tile_nb[t] = in_front; });
    for (int q = 0; q < 4; ++q)
        if (st[q]) atomicAdd(&s_sum[4 + q], st[q]);
    // the slots: d_pkt_first and the used range
    int lo = a.groups, hi = 0;
    const int records = scan_passes<RXG_THREADS, RXG_SLOT_TILE>(
        a.groups, wsum, [&](long long s) { return a.cnt[s]; },
        [&](long long s, int in_front, int c) {
            a.pkt_first[s + 1] = in_front + c;
            if (c) {
                lo = min(lo, static_cast<int>(s));
                hi = static_cast<int>(s) + 1;
            }
        });
    if (hi) {
        atomicMin(&s_sum[2], lo);
        atomicMax(&s_sum[3], hi);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        s_sum[0] = records;
        s_sum[1] = a.datagrams - records;
        a.pkt_first[0] = 0;
        if (s_sum[4]) atomicAdd(a.errors, s_sum[4]);
    }
    __syncthreads();
    if (threadIdx.x < 8) a.summary[threadIdx.x] = s_sum[threadIdx.x];
}

__global__ __launch_bounds__(RXG_THREADS) void rxg_scatter(RxGroupArgs a) {
    __shared__ int wsum[RXG_WAVES];
    const int t = blockIdx.x;
    const long long i = static_cast<long long>(t) * RXG_TILE + threadIdx.x;
    const bool have = i < a.datagrams;
    const int slot = have ? a.dg_slot[i] : 0;
    const int nb = have && slot < 0;
    const int rank = block_scan<RXG_THREADS>(nb, wsum).excl;
    if (!have) return;
    const int records = a.summary[0];
    // the tails first: [records, datagrams) of the record lists, [datagrams - records, datagrams) of d_other
    if (i >= records) {
        a.pkt_off[i] = 0;
        a.pkt_len[i] = 0;
        a.pkt_dg[i] = -1;
    }
    if (i >= a.datagrams - records) a.other[i] = -1;
    if (nb)
        a.other[a.tile_nb[t] + rank] = static_cast<int>(i);
    else
        a.pkt_dg[a.pkt_first[slot] + a.pos[i]] = static_cast<int>(i);
}

__global__ __launch_bounds__(RXG_THREADS) void rxg_order(RxGroupArgs a) {
    __shared__ int s_dg[RXG_WAVES][RXG_MAX];
    __shared__ uint32_t s_bits[RXG_WAVES][64];  // RXG_SPAN bits: the slot's datagram indices from its lowest
    __shared__ int s_pre[RXG_WAVES][64];        // bits set below each word
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long sl = static_cast<long long>(blockIdx.x) * RXG_WAVES + wave;
    int f0 = 0, n = 0;
    if (sl < a.groups) {
        f0 = a.pkt_first[sl];
        n = a.pkt_first[sl + 1] - f0;
    }
    const bool sort = n <= RXG_MAX;
    if (sort)
        for (int j = lane; j < n; j += 64) s_dg[wave][j] = a.pkt_dg[f0 + j];
    s_bits[wave][lane] = 0;
    __syncthreads();  // (the only one: from here on a wave touches its own rows of LDS alone)
    if (sort) {
        // ascending datagram index = arrival order; the indices are distinct, so the ranks are too
        int v[RXG_PER_LANE], rank[RXG_PER_LANE];
        int lo = 0x7fffffff, hi = 0;
#pragma unroll
        for (int r = 0; r < RXG_PER_LANE; ++r) {
            const bool have = lane + 64 * r < n;
            v[r] = have ? s_dg[wave][lane + 64 * r] : 0;
            rank[r] = 0;
            if (have) {
                lo = min(lo, v[r]);
                hi = max(hi, v[r]);
            }
        }
        for (int d = 32; d; d >>= 1) {
            lo = min(lo, __shfl_xor(lo, d));
            hi = max(hi, __shfl_xor(hi, d));
        }
        if (n > 0 && hi - lo < RXG_SPAN) {
            // the usual case, a sender's interleaving: the slot's datagrams lie close together. One bit per
            // datagram index from `lo`; the rank is the count of bits below
#pragma unroll
            for (int r = 0; r < RXG_PER_LANE; ++r)
                if (lane + 64 * r < n) atomicOr(&s_bits[wave][(v[r] - lo) >> 5], 1u << ((v[r] - lo) & 31));
            const int c = __popc(s_bits[wave][lane]);
            int x = c;
            for (int d = 1; d < 64; d <<= 1) {
                const int y = __shfl_up(x, d);
                if (lane >= d) x += y;
            }
            s_pre[wave][lane] = x - c;
#pragma unroll
            for (int r = 0; r < RXG_PER_LANE; ++r)
                if (lane + 64 * r < n) {
                    const int d = v[r] - lo;
                    rank[r] = s_pre[wave][d >> 5] + __popc(s_bits[wave][d >> 5] & ((1u << (d & 31)) - 1));
                }
        } else {
            // indices spread wider than the bitmap: count, for each, the indices below it
            const int rows = (n + 63) / 64;  // wave-uniform
            for (int j = 0; j < n; ++j) {
                const int x = s_dg[wave][j];
#pragma unroll
                for (int r = 0; r < RXG_PER_LANE; ++r)
                    if (r < rows) rank[r] += x < v[r];
            }
        }
#pragma unroll
        for (int r = 0; r < RXG_PER_LANE; ++r)
            if (lane + 64 * r < n) {
                const int dg = v[r], h = (a.code[dg] >> 8) & 255;
                const int j = f0 + rank[r];
                a.pkt_dg[j] = dg;
                a.pkt_off[j] = a.dg_off[dg] + h + 1;
                a.pkt_len[j] = a.dg_len[dg] - h - 1;
            }
    } else {
        for (int j = lane; j < n; j += 64) {
            const int dg = a.pkt_dg[f0 + j], h = (a.code[dg] >> 8) & 255;
            a.pkt_off[f0 + j] = a.dg_off[dg] + h + 1;
            a.pkt_len[f0 + j] = a.dg_len[dg] - h - 1;
        }
    }
}

long long tiles_of(long long datagrams) { return (datagrams + RXG_TILE - 1) / RXG_TILE; }

}  // namespace

long long rx_group_scratch_bytes(long long datagrams, long long groups) {
    return 32 + ((4 * groups + 7) & ~7ll) + 8 * datagrams + 32 * tiles_of(datagrams);
}

hipError_t launch_rx_group(RxGroupArgs a, void *scratch, hipStream_t stream) {
    if (a.groups <= 0) return hipSuccess;
    const long long tiles = tiles_of(a.datagrams);
    a.tiles = static_cast<int>(tiles);
    a.hdr = static_cast<int *>(scratch);
    a.cnt = a.hdr + 8;
    a.code = a.cnt + ((static_cast<long long>(a.groups) + 1) & ~1ll);
    a.pos = a.code + a.datagrams;
    a.tile_fp = a.pos + a.datagrams;
    a.tile_sum = a.tile_fp + tiles;
    a.tile_u = a.tile_sum + tiles;
    a.tile_nb = a.tile_u + tiles;
    a.tile_stat = a.tile_nb + tiles;
    // rxg_classify also clears the slot counters: at least enough workgroups for that to be quick
    const long long slot_wgs = std::min<long long>((static_cast<long long>(a.groups) - 1) / RXG_THREADS + 1, 2048);
    const unsigned wgs0 = static_cast<unsigned>(std::max(tiles, slot_wgs));
    hipLaunchKernelGGL(rxg_classify, dim3(wgs0), dim3(RXG_THREADS), 0, stream, a);
    hipLaunchKernelGGL(rxg_scan_tiles, dim3(1), dim3(RXG_THREADS), 0, stream, a);
    if (tiles) hipLaunchKernelGGL(rxg_down, dim3(static_cast<unsigned>(tiles)), dim3(RXG_THREADS), 0, stream, a);
    hipLaunchKernelGGL(rxg_scan_slots, dim3(1), dim3(RXG_THREADS), 0, stream, a);
    if (tiles) {
        hipLaunchKernelGGL(rxg_scatter, dim3(static_cast<unsigned>(tiles)), dim3(RXG_THREADS), 0, stream, a);
        hipLaunchKernelGGL(rxg_order, dim3(static_cast<unsigned>((a.groups - 1) / RXG_WAVES + 1)), dim3(RXG_THREADS), 0,
                           stream, a);
    }
    return hipGetLastError();
}

}  // namespace sh
