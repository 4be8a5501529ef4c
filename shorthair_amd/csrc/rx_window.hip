// Open code groups carried from one receive batch to the next (include/shorthair_rx.h,
// shorthair_rx_window_batch): what Decoder::OnData keeps between packets -- the packets of an unfinished
// group and "this group is done" (Shorthair.cpp:783-791) -- for batches of datagrams in GPU memory.
//
// Four launches, none of which waits on another workgroup:
//   rxw_slots  a lane per slot. As old slot i: the finished flag from the listings' d_info, whether the slot
//              is newly finished, whether it expires open. As group-call slot i: its records when it lies
//              below the window. As next slot i: the done code, the spans of its carried and its new
//              records, and -- walking the carried records -- their validity and the slot's carried bytes.
//              The five counts go to wg_stat per workgroup.
//   rxw_scan   one workgroup scans the per-slot (records, bytes) pairs, RXW_SCAN_PASS slots per pass with a
//              running carry. Both sums never decrease, so "ends past the capacity or the hold region" holds
//              from the first such slot on: that slot and every later one with a record is emptied. Writes
//              first, done, base, the summary and the error count; bytes[] becomes the slots' exclusive sum.
//   rxw_carry  a lane per slot walks its carried records once more and writes their off (the running sum
//              from the slot's first hold byte), len and dg = -1 at their places in the next window. The
//              places are indexed by destination, so spans of prev->first that overlap -- possible around a
//              span that runs backwards -- stay apart.
//   rxw_place  the hot path, record-driven: a sub-group of 1 << lshift lanes per record of the next window
//              finds its slot by bisection of first[]; a new record's off, len and dg are written, a carried
//              record is copied from its source to the off rxw_carry gave it (rx_window_copy.hpp); the tails
//              of the three lists.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shorthair_rx.h"
#include "block_scan.hpp"
#include "rx_window.hpp"
#include "rx_window_copy.hpp"

namespace sh {
namespace {

constexpr int RXW_THREADS = 256;
constexpr int RXW_WAVES = RXW_THREADS / 64;
constexpr int RXW_SCAN_TILE = SHORTHAIR_RX_WINDOW_SCAN_TILE;
constexpr int RXW_SCAN_PASS = SHORTHAIR_RX_WINDOW_SCAN_PASS;
constexpr int RXW_ALIGN = SHORTHAIR_RX_HOLD_ALIGN;
constexpr int RXW_STATS = 5;   // newly finished, expired, ignored, below the window, malformed
constexpr int RXW_LSHIFT = 4;  // lanes per record of rxw_place when it copies: 16 pieces of 16 bytes a step
static_assert(RXW_MAX_INFO == SHORTHAIR_RX_WINDOW_MAX_INFO, "info arrays");
static_assert(RXW_SCAN_PASS == RXW_SCAN_TILE * RXW_THREADS, "whole lanes");
static_assert(RXW_ALIGN == 16, "the copy's pieces");

__device__ __forceinline__ int sub_wrap(int a, int b) {
    return static_cast<int>(static_cast<unsigned>(a) - static_cast<unsigned>(b));
}

__device__ __forceinline__ long long round_up(int len) {
    return (static_cast<long long>(len) + RXW_ALIGN - 1) & ~static_cast<long long>(RXW_ALIGN - 1);
}

// Step 1: how far the window moves past the previous one (dp = N - P) and past the group call's (dg = N - Gb).
struct Shift {
    long long dp, dg;
    int N;
};
__device__ __forceinline__ Shift window_shift(const RxWindowArgs &a) {
    const int Gb = a.g_slot_group[0];
    Shift w{0, 0, Gb};
    if (a.has_prev) {
        const int P = a.p_base[0];
        const long long d = sub_wrap(Gb, P);
        w.dp = d > 0 ? d : 0;
        w.dg = d < 0 ? -d : 0;
        w.N = d > 0 ? Gb : P;
    }
    return w;
}

// Step 2 for old slot so: f, and d through `done`.
__device__ __forceinline__ int finished_flag(const RxWindowArgs &a, long long so, int &done) {
    int f = 0;
    for (int q = 0; q < a.n_info; ++q) {
        const int *e = a.info[q] + so * SHORTHAIR_RX_INFO_INTS;
        const int st = e[0];
        if (st == -1) f = 2;
        else if (f == 0 && (st == 1 || st == 2 || (st == 0 && e[1] >= 1 && e[4] >= e[1]))) f = 1;
    }
    const int old = a.p_done[so];
    done = old ? old : f;
    return f;
}

__global__ __launch_bounds__(RXW_THREADS) void rxw_slots(RxWindowArgs a) {
    __shared__ unsigned long long stat[RXW_STATS];
    if (threadIdx.x < RXW_STATS) stat[threadIdx.x] = 0;
    __syncthreads();
    const long long i = static_cast<long long>(blockIdx.x) * RXW_THREADS + threadIdx.x;
    const Shift w = window_shift(a);
    unsigned long long mine[RXW_STATS] = {0, 0, 0, 0, 0};
    if (i < a.groups) {
        // as old slot i: newly finished; expired while open and holding records
        if (a.has_prev) {
            int d;
            const int f = finished_flag(a, i, d);
            if (a.p_done[i] == 0 && f == 1) mine[0] = 1;
            if (i < w.dp && d == 0 && a.p_first[i + 1] > a.p_first[i]) mine[1] = 1;
        }
        // as group-call slot i below the window
        if (i < w.dg) {
            const int g0 = a.g_first[i], g1 = a.g_first[i + 1];
            if (g0 >= 0 && g1 >= g0 && g1 <= a.datagrams) mine[3] = static_cast<unsigned>(g1 - g0);
        }
        // as next slot i
        const long long so = i + w.dp, t = i + w.dg;
        int done = 0, cc = 0, srcc = 0, cn = 0, srcn = 0;
        long long bytes = 0;
        bool bad = false;
        if (a.has_prev && so < a.groups) {
            finished_flag(a, so, done);
            if (done == 0) {
                const int f0 = a.p_first[so], f1 = a.p_first[so + 1];
                if (f0 < 0 || f1 < f0 || f1 > a.p_cap) {
                    bad = true;
                } else {
                    for (int p = f0; p < f1; ++p) {
                        const long long off = a.p_off[p];
                        const int len = a.p_len[p];
                        if (len < 0 || off < 0 || off > a.ring_bytes - len) {
                            bad = true;
                            break;
                        }
                        if (a.copy) bytes += round_up(len);
                    }
                    cc = f1 - f0;
                    srcc = f0;
                }
            }
        }
        if (t < a.groups) {
            const int g0 = a.g_first[t], g1 = a.g_first[t + 1];
            const bool ok = g0 >= 0 && g1 >= g0 && g1 <= a.datagrams;
            if (done == 0 && !bad) {
                if (ok) {
                    cn = g1 - g0;
                    srcn = g0;
                } else {
                    bad = true;
                }
            } else if (ok) {
                mine[2] = static_cast<unsigned>(g1 - g0);
            }
        }
        if (bad) {
            done = 2;
            cc = cn = 0;
            bytes = 0;
            mine[4] = 1;
        }
        a.cnt_c[i] = cc;
        a.cnt_n[i] = cn;
        a.src_c[i] = srcc;
        a.src_n[i] = srcn;
        a.flag[i] = done;
        a.bytes[i] = bytes;
    }
#pragma unroll
    for (int c = 0; c < RXW_STATS; ++c)
        if (mine[c]) atomicAdd(&stat[c], mine[c]);
    __syncthreads();
    if (threadIdx.x < RXW_STATS) a.wg_stat[static_cast<long long>(blockIdx.x) * RXW_STATS + threadIdx.x] = static_cast<long long>(stat[threadIdx.x]);
}

__global__ __launch_bounds__(RXW_THREADS) void rxw_scan(RxWindowArgs a) {
    __shared__ long long wsum_r[RXW_WAVES], wsum_b[RXW_WAVES];
    __shared__ unsigned long long cut[2];                // records and bytes in front of the overflow cut
    __shared__ unsigned long long tot[RXW_STATS + 2];    // the five counts, emptied slots, carried records
    if (threadIdx.x < 2) cut[threadIdx.x] = 0;
    if (threadIdx.x < RXW_STATS + 2) tot[threadIdx.x] = 0;
    const Shift w = window_shift(a);
    unsigned long long mine[RXW_STATS + 2] = {0, 0, 0, 0, 0, 0, 0};
    for (long long q = threadIdx.x; q < static_cast<long long>(a.wgs) * RXW_STATS; q += RXW_THREADS)
        mine[q % RXW_STATS] += static_cast<unsigned long long>(a.wg_stat[q]);
    // (not scan_passes: the cut is a workgroup-wide maximum between two walks over the lane's slots)
    long long carry_r = 0, carry_b = 0;
    for (long long base = 0; base < a.groups; base += RXW_SCAN_PASS) {
        const long long s0 = base + threadIdx.x * RXW_SCAN_TILE;
        int cc[RXW_SCAN_TILE], cn[RXW_SCAN_TILE];
        long long b[RXW_SCAN_TILE], sum_r = 0, sum_b = 0;
#pragma unroll
        for (int j = 0; j < RXW_SCAN_TILE; ++j) {
            const bool in = s0 + j < a.groups;
            cc[j] = in ? a.cnt_c[s0 + j] : 0;
            cn[j] = in ? a.cnt_n[s0 + j] : 0;
            b[j] = in ? a.bytes[s0 + j] : 0;
            sum_r += static_cast<long long>(cc[j]) + cn[j];
            sum_b += b[j];
        }
        const Scanned<long long> sc_r = block_scan<RXW_THREADS>(sum_r, wsum_r);
        const Scanned<long long> sc_b = block_scan<RXW_THREADS>(sum_b, wsum_b);
        const long long r0 = carry_r + sc_r.excl, b0 = carry_b + sc_b.excl;
        // the last slot of this lane that still fits: both sums are monotone, so the largest is the cut
        long long at_r = r0, at_b = b0, fit_r = -1, fit_b = 0;
#pragma unroll
        for (int j = 0; j < RXW_SCAN_TILE; ++j) {
            at_r += static_cast<long long>(cc[j]) + cn[j];
            at_b += b[j];
            if (s0 + j < a.groups && at_r <= a.n_cap && at_b <= a.hold_bytes) {
                fit_r = at_r;
                fit_b = at_b;
            }
        }
        if (fit_r >= 0) {
            atomicMax(&cut[0], static_cast<unsigned long long>(fit_r));
            atomicMax(&cut[1], static_cast<unsigned long long>(fit_b));
        }
        __syncthreads();
        const long long cut_r = static_cast<long long>(cut[0]);
        at_r = r0;
        at_b = b0;
#pragma unroll
        for (int j = 0; j < RXW_SCAN_TILE; ++j) {
            const long long n = static_cast<long long>(cc[j]) + cn[j];
            const long long excl_b = at_b;
            at_r += n;
            at_b += b[j];
            if (s0 + j < a.groups) {
                const bool over = at_r > a.n_cap || at_b > a.hold_bytes;
                a.n_first[s0 + j + 1] = static_cast<int>(over ? cut_r : at_r);
                a.bytes[s0 + j] = excl_b;
                a.n_done[s0 + j] = static_cast<unsigned char>(over && n > 0 ? 3 : a.flag[s0 + j]);
                if (over && n > 0) mine[RXW_STATS] += 1;
                if (!over) mine[RXW_STATS + 1] += static_cast<unsigned>(cc[j]);
            }
        }
        carry_r += sc_r.total;
        carry_b += sc_b.total;
        __syncthreads();  // wsum_r and wsum_b are rewritten by the next pass
    }
#pragma unroll
    for (int c = 0; c < RXW_STATS + 2; ++c)
        if (mine[c]) atomicAdd(&tot[c], mine[c]);
    __syncthreads();
    if (threadIdx.x == 0) {
        a.n_first[0] = 0;
        a.n_base[0] = w.N;
        a.summary[0] = static_cast<long long>(cut[0]);
        a.summary[1] = static_cast<long long>(tot[RXW_STATS + 1]);
        a.summary[2] = static_cast<long long>(cut[1]);
        a.summary[3] = static_cast<long long>(tot[0]);
        a.summary[4] = static_cast<long long>(tot[1]);
        a.summary[5] = static_cast<long long>(tot[2]);
        a.summary[6] = static_cast<long long>(tot[3]);
        const unsigned long long errors = tot[4] + tot[RXW_STATS];
        a.summary[7] = static_cast<long long>(errors);
        if (errors) atomicAdd(a.errors, static_cast<int>(errors));
    }
}

__global__ __launch_bounds__(RXW_THREADS) void rxw_carry(RxWindowArgs a) {
    const long long s = static_cast<long long>(blockIdx.x) * RXW_THREADS + threadIdx.x;
    if (s >= a.groups) return;
    const int r0 = a.n_first[s], cc = a.cnt_c[s];
    if (a.n_first[s + 1] == r0) return;  // empty, or emptied by the cut
    const int p0 = a.src_c[s];
    long long at = a.hold_off + a.bytes[s];
    for (int j = 0; j < cc; ++j) {
        const int len = a.p_len[p0 + j];
        a.n_off[r0 + j] = a.copy ? at : a.p_off[p0 + j];
        a.n_len[r0 + j] = len;
        a.n_dg[r0 + j] = -1;
        at += round_up(len);
    }
}

__global__ __launch_bounds__(RXW_THREADS) void rxw_place(RxWindowArgs a) {
    const LaneSplit ls = lane_split(static_cast<long long>(blockIdx.x) * RXW_THREADS + threadIdx.x, a.lshift);
    const long long r = ls.item;
    if (r >= a.n_cap) return;
    const int sub = ls.sub;
    if (r >= a.n_first[a.groups]) {  // the tails
        if (sub == 0) {
            a.n_off[r] = 0;
            a.n_len[r] = 0;
            a.n_dg[r] = -1;
        }
        return;
    }
    // the slot of record r: the first s with first[s + 1] > r
    int lo = 0, hi = a.groups - 1;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (a.n_first[mid + 1] <= r) lo = mid + 1; else hi = mid;
    }
    const int s = lo;
    const int j = static_cast<int>(r - a.n_first[s]);
    const int cc = a.cnt_c[s];
    if (j >= cc) {  // a new record keeps its place
        if (sub == 0) {
            const long long q = static_cast<long long>(a.src_n[s]) + (j - cc);
            a.n_off[r] = a.g_off[q];
            a.n_len[r] = a.g_len[q];
            a.n_dg[r] = a.g_dg[q];
        }
        return;
    }
    if (a.copy) {  // a carried record: rxw_carry wrote its place
        const TxCopy c = rxw_copy_plan(a.ring, a.ring_bytes, a.p_off[static_cast<long long>(a.src_c[s]) + j], a.n_len[r]);
        txd_copy_lane(c, a.ring + a.n_off[r], sub, ls.step);
    }
}

long long slot_wgs(long long groups) { return (groups + RXW_THREADS - 1) / RXW_THREADS; }

}  // namespace

long long rx_window_scratch_bytes(long long groups, long long capacity) {
    (void)capacity;  // (nothing is kept per record)
    return 32 + 8 * ((5 * groups + 1) / 2) + 8 * groups + 8 * RXW_STATS * slot_wgs(groups);
}

hipError_t launch_rx_window(RxWindowArgs a, void *scratch, hipStream_t stream) {
    if (a.groups <= 0) return hipSuccess;
    const long long G = a.groups;
    a.wgs = static_cast<int>(slot_wgs(G));
    long long *q = static_cast<long long *>(scratch) + 4;  // (a header of 32 bytes, unused)
    a.bytes = q;
    a.wg_stat = a.bytes + G;
    a.cnt_c = reinterpret_cast<int *>(a.wg_stat + static_cast<long long>(a.wgs) * RXW_STATS);
    a.cnt_n = a.cnt_c + G;
    a.src_c = a.cnt_n + G;
    a.src_n = a.src_c + G;
    a.flag = a.src_n + G;
    a.copy = a.has_prev && a.hold_bytes > 0;
    a.lshift = a.copy ? RXW_LSHIFT : 0;
    hipLaunchKernelGGL(rxw_slots, dim3(static_cast<unsigned>(a.wgs)), dim3(RXW_THREADS), 0, stream, a);
    hipLaunchKernelGGL(rxw_scan, dim3(1), dim3(RXW_THREADS), 0, stream, a);
    if (a.n_cap > 0) {
        if (a.has_prev) hipLaunchKernelGGL(rxw_carry, dim3(static_cast<unsigned>(a.wgs)), dim3(RXW_THREADS), 0, stream, a);
        // capacity <= INT_MAX, 16 lanes each at most: always within a grid
        const long long wgs = ((static_cast<long long>(a.n_cap) << a.lshift) + RXW_THREADS - 1) / RXW_THREADS;
        hipLaunchKernelGGL(rxw_place, dim3(static_cast<unsigned>(wgs)), dim3(RXW_THREADS), 0, stream, a);
    }
    return hipGetLastError();
}

}  // namespace sh
