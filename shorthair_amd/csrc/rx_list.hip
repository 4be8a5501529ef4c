// Device-resident listing of received packets (include/shorthair_rx.h): the rule of OnData / CanRecover /
// RecoverGroup (Shorthair.cpp:796-898, ShorthairDetails.hpp:328-336, Shorthair.cpp:704-761), as rx_info
// (shorthair_groups.cpp) restates it for host lists, for a whole batch of groups whose records sit in
// GPU memory.
//
// Three launches, none of which waits on another workgroup:
//   rx_classify  one wave per group. Its lanes stride over the group's records 64 at a time: offset and
//                length (coalesced), then the three header bytes as byte loads at any alignment. The
//                class counts, the first and the last recovery record come from __ballot masks; the
//                headers stay in LDS for the second walk, which checks ids, lengths and repeats (a
//                256-bit seen mask in LDS, set with atomicOr). d_info[g] is written here; (status, k)
//                goes to scratch as one int per group and (id, class) as two bytes per record, so that
//                no later kernel touches the ring again.
//   rx_scan      one workgroup turns the per-group codes into slots and d_first: a lane sums RX_TILE
//                consecutive groups, the workgroup scans RX_PASS groups per pass with a running carry.
//                It also applies step 9 (blocks past the capacity), counts the statuses into d_summary
//                and adds the malformed groups to the error counter, once.
//   rx_write     one wave per group again: a listed group's records get their in-class ranks from
//                ballots over the scratch classes and are written to the four lists at d_first[slot] +
//                position. Then all lanes of the grid write the tails: zeros in [total, capacity) of the
//                lists, -1 in d_slot_group and total in d_first past the listed slots.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/shorthair_rx.h"
#include "block_scan.hpp"
#include "bytes.hpp"
#include "rx_list.hpp"

namespace sh {
namespace {

constexpr int RX_THREADS = 256;
constexpr int RX_WAVES = RX_THREADS / 64;  // groups per workgroup of rx_classify and rx_write
constexpr int RX_MAX = SHORTHAIR_RX_MAX_PACKETS;
constexpr int RX_INFO = SHORTHAIR_RX_INFO_INTS;
constexpr int RX_TILE = SHORTHAIR_RX_SCAN_TILE;
constexpr int RX_PASS = SHORTHAIR_RX_SCAN_PASS;
static_assert(RX_PASS == RX_TILE * RX_THREADS, "a lane per tile");
static_assert(RX_INFO == 8, "lanes 0..7 write d_info[g]");

// header word in LDS: id | c << 8 | class << 16
constexpr uint32_t CLS_ORIG = 1, CLS_REC = 2;

// Step 0: the records of group g, [f0, f0 + n); ok = false (and n = 0) for a malformed span.
struct Span {
    int f0, n;
    bool ok;
};
__device__ __forceinline__ Span group_span(const RxListArgs &a, int g) {
    const int f0 = a.pkt_first[g], f1 = a.pkt_first[g + 1];
    Span s;
    s.ok = f0 >= 0 && f1 >= f0 && f1 <= a.packets && f1 - f0 <= RX_MAX;
    s.f0 = f0;
    s.n = s.ok ? f1 - f0 : 0;
    return s;
}

__device__ __forceinline__ void write_info(const RxListArgs &a, int g, int lane, int status, int k, int m, int B,
                                           int n_orig, int n_rec, int slot, int first_rec) {
    if (lane >= RX_INFO) return;
    const int v = lane == 0 ? status : lane == 1 ? k : lane == 2 ? m : lane == 3 ? B : lane == 4 ? n_orig
                : lane == 5 ? n_rec : lane == 6 ? slot : first_rec;
    a.info[static_cast<long long>(g) * RX_INFO + lane] = v;
}

__global__ __launch_bounds__(RX_THREADS) void rx_classify(RxListArgs a) {
    __shared__ uint32_t s_hdr[RX_WAVES][RX_MAX];
    __shared__ int s_len[RX_WAVES][RX_MAX];
    __shared__ uint32_t s_seen[RX_WAVES][8];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane < 8) s_seen[wave][lane] = 0;
    __syncthreads();  // the only one: from here on a wave touches its own rows of LDS alone
    const long long gl = static_cast<long long>(blockIdx.x) * RX_WAVES + wave;
    if (gl >= a.groups) return;
    const int g = static_cast<int>(gl);
    const Span sp = group_span(a, g);

    // steps 1 and 3: classes, counts, the first recovery record's k, the last one's length and byte 2
    int k = 0, n_orig = 0, n_rec = 0, first_rec = -1, last_len = 0, last_b2 = 0;
    bool bad = !sp.ok, mismatch = false;
    for (int c0 = 0; c0 < sp.n; c0 += 64) {
        const int i = c0 + lane;
        const bool have = i < sp.n;
        const int p = sp.f0 + (have ? i : 0);  // (a lane past the group reads its first record's entry and drops it)
        const long long off = a.pkt_off[p];
        const int len = a.pkt_len[p];
        const bool ok = have && len >= 2 && off >= 0 && off <= a.ring_bytes - len;
        uint32_t id = 0, cc = 0, b2 = 0;
        if (ok) {
            id = a.ring[off];
            cc = a.ring[off + 1];
            if (len >= 3) b2 = a.ring[off + 2];
        }
        const bool is_rec = ok && id > cc, is_orig = ok && id <= cc;
        const uint64_t mr = __ballot(is_rec), mo = __ballot(is_orig);
        bad |= __ballot(have && !ok) != 0;
        if (mr) {
            if (first_rec < 0) {
                const int fl = __ffsll(static_cast<unsigned long long>(mr)) - 1;
                first_rec = sp.f0 + c0 + fl;
                k = __shfl(static_cast<int>(cc), fl) + 1;
            }
            const int ll = 63 - __clzll(static_cast<long long>(mr));
            last_len = __shfl(len, ll);
            last_b2 = __shfl(static_cast<int>(b2), ll);
            mismatch |= __ballot(is_rec && static_cast<int>(cc) + 1 != k) != 0;
        }
        n_orig += __popcll(mo);
        n_rec += __popcll(mr);
        if (have) {
            s_hdr[wave][i] = id | (cc << 8) | ((is_orig ? CLS_ORIG : is_rec ? CLS_REC : 0u) << 16);
            s_len[wave][i] = len;
            a.rec[p] = static_cast<uint16_t>(id | (is_rec ? 0x100u : 0u));
        }
    }

    // steps 2 to 6, on wave-uniform values
    int status, m = 0, B = 0;
    bool walk = false;
    if (bad) status = -1;
    else if (n_rec == 0) status = 0;
    else if (mismatch) status = -1;
    else if (k == 1) status = n_orig == 0 ? 2 : 0;
    else if (n_orig >= k || n_orig + n_rec < k) status = 0;
    else if (last_len < 3) status = -1;
    else {
        m = last_b2 + 1;
        B = last_len - 3;
        walk = !(B < 8 || B % 8 != 0 || k + m > 256);
        status = -1;
    }

    // step 7
    if (walk) {
        const int use = k - n_orig;
        int rr = 0;
        bool bad7 = false;
        for (int c0 = 0; c0 < sp.n; c0 += 64) {
            const int i = c0 + lane;
            const bool have = i < sp.n;
            const uint32_t h = have ? s_hdr[wave][i] : 0;
            const int len = have ? s_len[wave][i] : 0;
            const int id = h & 255, cc = (h >> 8) & 255;
            const bool is_orig = (h >> 16) == CLS_ORIG, is_rec = (h >> 16) == CLS_REC;
            const uint64_t mr = __ballot(is_rec);
            const bool used = is_rec && rr + __popcll(mr & lanes_below(lane)) < use;
            bool b = false;
            if (is_orig) b = cc >= k || len - 2 > B - 2;
            if (used) b = id < k || id >= k + m || len != B + 3;
            if (is_orig || used) {
                const uint32_t bit = 1u << (id & 31);
                b |= (atomicOr(&s_seen[wave][id >> 5], bit) & bit) != 0;
            }
            bad7 |= __ballot(b) != 0;
            rr += __popcll(mr);
        }
        if (!bad7) status = (k >= a.kmin && k <= a.kmax && m == a.m && B == a.B) ? 1 : 3;
    }

    if (status < 0)
        write_info(a, g, lane, -1, 0, 0, 0, 0, 0, -1, -1);
    else if (status == 1 || status == 3)
        write_info(a, g, lane, status, k, m, B, n_orig, n_rec, -1, first_rec);  // the slot: rx_scan
    else
        write_info(a, g, lane, status, k, 0, 0, n_orig, n_rec, -1, first_rec);
    if (lane == 0) a.code[g] = ((status == 1 ? k : 0) << 8) | (status + 1);
}

// What rx_scan scans: a group that step 8 lists is {k, 1}, any other {0, 0}. The blocks in front of a
// group can pass the capacity (step 9), the slots cannot pass INT_MAX.
struct __attribute__((packed, aligned(4))) Listed {
    long long blocks;
    int slots;
};
struct ListedAdd {
    __device__ __forceinline__ Listed operator()(Listed x, Listed y) const {
        return Listed{x.blocks + y.blocks, x.slots + y.slots};
    }
};

__global__ __launch_bounds__(RX_THREADS) void rx_scan(RxListArgs a) {
    __shared__ Listed wsum[RX_WAVES];
    __shared__ int s_sum[8];  // d_summary
    if (threadIdx.x < 8) s_sum[threadIdx.x] = 0;
    __syncthreads();
    int listed = 0, end = 0, skipped = 0, k1 = 0, other = 0, malformed = 0;
    scan_passes<RX_THREADS, RX_TILE>(
        a.groups, wsum,
        [&](long long g) {
            const int code = a.code[g], status = (code & 255) - 1;
            skipped += status == 0;
            k1 += status == 2;
            other += status == 3;
            malformed += status < 0;
            return status == 1 ? Listed{code >> 8, 1} : Listed{0, 0};
        },
        [&](long long g, Listed in_front, Listed item) {
            int at = -1;
            if (item.slots) {
                const long long b = in_front.blocks;
                const int slot = in_front.slots, k = static_cast<int>(item.blocks);
                if (b + k <= a.capacity) {
                    a.info[g * RX_INFO + 6] = slot;
                    a.slot_group[slot] = static_cast<int>(g);
                    a.first[slot + 1] = static_cast<int>(b) + k;
                    at = static_cast<int>(b);
                    end = at + k;
                    ++listed;
                } else {  // step 9; every listed group after this one fails it too
                    ++malformed;
                    int *info = a.info + g * RX_INFO;
                    info[0] = -1;
                    for (int j = 1; j < 6; ++j) info[j] = 0;
                    info[6] = info[7] = -1;
                }
            }
            a.base[g] = at;
        },
        Listed{0, 0}, ListedAdd{});
    if (listed) {
        atomicAdd(&s_sum[0], listed);
        atomicMax(&s_sum[1], end);
    }
    if (skipped) atomicAdd(&s_sum[2], skipped);
    if (k1) atomicAdd(&s_sum[3], k1);
    if (other) atomicAdd(&s_sum[4], other);
    if (malformed) atomicAdd(&s_sum[5], malformed);
    __syncthreads();
    if (threadIdx.x < 8) a.summary[threadIdx.x] = s_sum[threadIdx.x];
    if (threadIdx.x == 0) {
        a.first[0] = 0;
        if (s_sum[5]) atomicAdd(a.errors, s_sum[5]);
    }
}

__global__ __launch_bounds__(RX_THREADS) void rx_write(RxListArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long gl = static_cast<long long>(blockIdx.x) * RX_WAVES + wave;
    const int g = gl < a.groups ? static_cast<int>(gl) : 0;
    const int f = gl < a.groups ? a.base[g] : -1;
    if (f >= 0) {  // listed: every record is well formed, and blocks [f, f + k) lie below the capacity
        const int *info = a.info + static_cast<long long>(g) * RX_INFO;
        const int f0 = a.pkt_first[g], k = info[1], n_orig = info[4], n = n_orig + info[5];
        const int use = k - n_orig;
        int ro = 0, rr = 0;
        for (int c0 = 0; c0 < n && (ro < n_orig || rr < use); c0 += 64) {
            const int i = c0 + lane;
            const bool have = i < n;
            const int p = f0 + (have ? i : 0);
            const uint32_t w = a.rec[p];
            const long long off = a.pkt_off[p];
            const int len = a.pkt_len[p];
            const bool is_rec = have && (w >> 8) != 0, is_orig = have && (w >> 8) == 0;
            const uint64_t mr = __ballot(is_rec), mo = __ballot(is_orig), below = lanes_below(lane);
            const int rank = is_rec ? rr + __popcll(mr & below) : ro + __popcll(mo & below);
            if (is_orig ? rank < n_orig : (is_rec && rank < use)) {
                const int j = f + (is_rec ? n_orig + rank : rank);
                a.off[j] = off + (is_rec ? 3 : 2);
                a.len[j] = is_rec ? a.B : len - 2;
                a.raw[j] = is_rec ? 1 : 0;
                a.rows[j] = static_cast<uint8_t>(w);
            }
            ro += __popcll(mo);
            rr += __popcll(mr);
        }
    }
    // the tails, by every lane of the grid
    const int n_listed = a.summary[0], total = a.summary[1];
    const long long lim = max(static_cast<long long>(a.capacity), static_cast<long long>(a.groups) + 1);
    const long long step = static_cast<long long>(gridDim.x) * RX_THREADS;
    for (long long i = static_cast<long long>(blockIdx.x) * RX_THREADS + threadIdx.x; i < lim; i += step) {
        if (i >= total && i < a.capacity) {
            a.off[i] = 0;
            a.len[i] = 0;
            a.raw[i] = 0;
            a.rows[i] = 0;
        }
        if (i >= n_listed && i < a.groups) a.slot_group[i] = -1;
        if (i > n_listed && i <= a.groups) a.first[i] = total;
    }
}

}  // namespace

long long rx_list_scratch_bytes(long long groups, long long packets) {
    return 8 * (groups + 1) + ((2 * packets + 7) & ~7ll);
}

hipError_t launch_rx_list(RxListArgs a, void *scratch, hipStream_t stream) {
    if (a.groups <= 0) return hipSuccess;
    a.code = static_cast<int *>(scratch);
    a.base = a.code + a.groups;
    a.rec = reinterpret_cast<uint16_t *>(a.base + a.groups);
    const unsigned wgs = static_cast<unsigned>((a.groups - 1) / RX_WAVES + 1);
    hipLaunchKernelGGL(rx_classify, dim3(wgs), dim3(RX_THREADS), 0, stream, a);
    hipLaunchKernelGGL(rx_scan, dim3(1), dim3(RX_THREADS), 0, stream, a);
    hipLaunchKernelGGL(rx_write, dim3(wgs), dim3(RX_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sh
