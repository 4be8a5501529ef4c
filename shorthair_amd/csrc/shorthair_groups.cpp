// Batched packet-group framing around the codec (include/shorthair_groups.h).
//
// Sender: the reference's Encoder::EncodeQueued (Shorthair.cpp:480-576) and GenerateRecoveryBlock
// (:580-609) for many groups per call. Receiver: RecoverGroup (:704-761) over the packets OnData
// (:764-902) keeps, for many groups per call.
//
// Layer above the public batch ABI (cauchy_256_batch.h): groups are bucketed by (K, m, B) -- K the
// compiled kernel's k that codes the group (sh::fixed_kernel_k), or the group's own k without one
// -- so groups that would each run the same compiled kernel for the same K steps share a var-k
// launch (cauchy_256_*_var, blocks framed packed with first[] alongside); a bucket with a single
// distinct k makes the uniform call. A bucket is cut into chunks of ~chunk_bytes() of blocks, and chunks alternate between two pinned
// staging slots. For chunk i the host threads frame the blocks into slot i%2 while the GPU runs
// chunk i-1 (H2D, kernel, D2H on one stream); once slot i%2's previous chunk has completed its
// outputs are unframed on the host threads. So host framing, PCIe and kernels overlap, and the
// only host work per byte is the framing copy the reference also does (its memset/memcpy).
//
// shorthair_groups_set_framing(1) moves the framing to the GPU: the host threads then pack only the
// payload bytes into the pinned slot and shorthair_frame_batch builds the blocks in device memory.
//
// shorthair_groups_set_delivery(1) moves the receiver's unframing to the GPU ("Device delivery" below):
// shorthair_unframe_batch packs the recovered payloads of an m >= 2 chunk in device memory and only
// they, their lengths and rows come back, in two copies; the callbacks are the same.
//
// shorthair_groups_set_wire(1) moves the sender's packet headers to the GPU: shorthair_wire_emit_batch
// builds the "[k+y][k-1][m-1][block]" records of a chunk in device memory behind the codec's output, they
// come back whole, and the finisher copies a group's m records in one piece.
//
// There is one copy of each thing for all routes: one chunk plan (Chunks), one slot layout per chunk
// (slot_layout), one encode_bucket and one recover_bucket. The framing route decides only what
// prepare writes into the pinned slot (put_block) and what is enqueued before the codec call
// (submit_inputs); uniform or mixed k decides only which codec call runs and whether first[] exists.
#include <hip/hip_runtime.h>
#include <sched.h>
#include <emmintrin.h>

#include <algorithm>
#include <atomic>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "../../include/cauchy_256_batch.h"
#include "../../include/shorthair_frame.h"
#include "../../include/shorthair_unframe.h"
#include "../../include/shorthair_wire.h"
#include "kernels.hpp"
#include "measure.hpp"
#include "../../include/shorthair_groups.h"

namespace {

// device bytes per chunk (inputs + outputs); SH_PKT_CHUNK_MB: measurement switch
size_t chunk_bytes() {
    static const size_t b = [] {
        const char *e = SH_MEASURE_ENV("SH_PKT_CHUNK_MB");
        const int mb = e ? std::atoi(e) : 48;
        return static_cast<size_t>(std::max(1, mb)) << 20;
    }();
    return b;
}

#define SG_CHECK(expr)                                                                        \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            std::fprintf(stderr, "libcauchy256: %s failed: %s (%s:%d)\n", #expr,             \
                         hipGetErrorString(_e), __FILE__, __LINE__);                          \
            return -2;                                                                        \
        }                                                                                     \
    } while (0)

inline int roundup8(int x) { return (x + 7) & ~7; }
inline void put_u16(uint8_t *p, unsigned v) {  // WriteU16_LE (ShorthairDetails.hpp)
    p[0] = static_cast<uint8_t>(v);
    p[1] = static_cast<uint8_t>(v >> 8);
}
inline unsigned get_u16(const uint8_t *p) { return p[0] | (static_cast<unsigned>(p[1]) << 8); }

// Framing copy into the pinned staging buffer: 16-byte non-temporal stores for the aligned body
// (the staging bytes are read next by the H2D DMA, not by this core, so a cached store's
// read-for-ownership of every line is wasted memory traffic), plain copies for the ragged ends.
// Callers fence (framing_fence) before the buffer is handed to the DMA.
inline void framing_copy(uint8_t *dst, const uint8_t *src, size_t n) {
    if (n < 64) {
        std::memcpy(dst, src, n);
        return;
    }
    const size_t head = (16 - (reinterpret_cast<uintptr_t>(dst) & 15)) & 15;
    std::memcpy(dst, src, head);
    dst += head;
    src += head;
    n -= head;
    const size_t body = n & ~static_cast<size_t>(15);
    for (size_t i = 0; i < body; i += 16)
        _mm_stream_si128(reinterpret_cast<__m128i *>(dst + i),
                         _mm_loadu_si128(reinterpret_cast<const __m128i *>(src + i)));
    std::memcpy(dst + body, src + body, n - body);
}
inline void framing_fence() { _mm_sfence(); }

int host_threads() {
    static const int n = [] {
        // the cores this process may run on (its affinity mask: a job's share of a large host),
        // at most 16; SH_HOST_THREADS overrides it in measurement builds only
        cpu_set_t set;
        CPU_ZERO(&set);
        int v = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set)
                                                            : static_cast<int>(std::thread::hardware_concurrency());
        if (const char *e = SH_MEASURE_ENV("SH_HOST_THREADS")) v = std::atoi(e);
        return std::max(1, std::min(v > 0 ? v : 1, 16));
    }();
    return n;
}

// Persistent host workers for the framing copies: host_threads() - 1 threads started on first use
// and parked on a condition variable between calls (spawning and joining 15 threads per framing
// pass cost ~0.3 ms each time, two passes per chunk). Never destroyed: parked threads are fine at
// process exit.
class Workers {
  public:
    explicit Workers(int n) : nthreads_(n) {
        for (int w = 1; w < n; ++w) th_.emplace_back([this, w] { loop(w); });
        for (auto &t : th_) t.detach();
    }
    int size() const { return nthreads_; }
    // fn(i) for i in [0, n) split into t <= size() contiguous ranges; the caller runs range 0.
    // One pass owns the pool at a time; a pass from another thread that finds it busy runs its
    // whole range on its own thread instead of queueing behind the owner, so
    // concurrent shorthair_*_groups calls still overlap.
    void run(int n, int t, const std::function<void(int)> &fn) {
        std::unique_lock<std::mutex> one(run_mu_, std::try_to_lock);
        if (!one.owns_lock() || t <= 1) {
            for (int i = 0; i < n; ++i) fn(i);
            return;
        }
        {
            std::lock_guard<std::mutex> g(mu_);
            fn_ = &fn;
            n_ = n;
            t_ = t;
            pending_ = nthreads_ - 1;
            ++gen_;
        }
        cv_.notify_all();
        range(0, n, t, fn);
        std::unique_lock<std::mutex> g(mu_);
        done_.wait(g, [this] { return pending_ == 0; });
    }

  private:
    static void range(int w, int n, int t, const std::function<void(int)> &fn) {
        if (w >= t) return;
        const int a = static_cast<int>(static_cast<long long>(n) * w / t);
        const int b = static_cast<int>(static_cast<long long>(n) * (w + 1) / t);
        for (int i = a; i < b; ++i) fn(i);
    }
    void loop(int w) {
        unsigned long long seen = 0;
        for (;;) {
            const std::function<void(int)> *fn;
            int n, t;
            {
                std::unique_lock<std::mutex> g(mu_);
                cv_.wait(g, [&] { return gen_ != seen; });
                seen = gen_;
                fn = fn_;
                n = n_;
                t = t_;
            }
            range(w, n, t, *fn);
            std::lock_guard<std::mutex> g(mu_);
            if (--pending_ == 0) done_.notify_one();
        }
    }
    const int nthreads_;
    std::vector<std::thread> th_;
    std::mutex run_mu_, mu_;
    std::condition_variable cv_, done_;
    const std::function<void(int)> *fn_ = nullptr;
    int n_ = 0, t_ = 0, pending_ = 0;
    unsigned long long gen_ = 0;
};

Workers &workers() {
    static Workers *w = new Workers(host_threads());
    return *w;
}

// fn(i) for i in [0, n) on up to host_threads() threads (contiguous ranges).
void parallel_for(int n, const std::function<void(int)> &fn) {
    const int t = std::min(host_threads(), std::max(1, n / 4));
    if (t <= 1) {
        for (int i = 0; i < n; ++i) fn(i);
        return;
    }
    workers().run(n, t, fn);
}

// Two pinned + device staging slots on one stream; each slot remembers how to finish the chunk
// it carries (unframe outputs once its event has fired).
struct Slot {
    void *h = nullptr, *d = nullptr;
    size_t nh = 0, nd = 0;
    hipEvent_t ev = nullptr;
    std::function<int()> finish;  // empty: nothing pending; returns 0 or the call's error
    std::function<int()> late;    // device delivery: set by finish, run once the next chunk is prepared
};

struct Staging {
    std::mutex mu;  // one packet-group call at a time (shared slots)
    bool ready = false;
    hipStream_t stream = nullptr;
    hipStream_t stream2 = nullptr;  // device delivery: the second-phase D2H copies (created on first use)
    Slot slot[2];
};

Staging &staging() {
    static Staging s;
    return s;
}

// nh pinned bytes and nd device bytes: equal on the host-framing route (the slot is mirrored); on the
// device-framing route the pinned side holds payload bytes and outputs only, the device side the
// framed blocks as well.
int ensure_slot(Slot &s, size_t nh, size_t nd) {
    if (!s.ev) SG_CHECK(hipEventCreateWithFlags(&s.ev, hipEventDisableTiming));
    if (nh > s.nh) {
        if (s.h) (void)hipHostFree(s.h);
        s.h = nullptr;
        s.nh = 0;
        SG_CHECK(hipHostMalloc(&s.h, nh, hipHostMallocDefault));
        s.nh = nh;
    }
    if (nd > s.nd) {
        if (s.d) (void)hipFree(s.d);
        s.d = nullptr;
        s.nd = 0;
        SG_CHECK(hipMalloc(&s.d, nd));
        s.nd = nd;
    }
    return 0;
}

int ensure_staging(Staging &st) {
    if (st.ready) return 0;
    if (cauchy_256_batch_init(-1) != 0) return -2;
    SG_CHECK(hipStreamCreateWithFlags(&st.stream, hipStreamNonBlocking));
    st.ready = true;
    return 0;
}

// Wait for the slot's previous chunk and unframe its outputs.
int drain(Slot &s) {
    if (!s.finish) return 0;
    SG_CHECK(hipEventSynchronize(s.ev));
    auto f = std::move(s.finish);
    s.finish = nullptr;
    return f();
}

int run_late(Slot &s) {
    if (!s.late) return 0;
    auto f = std::move(s.late);
    s.late = nullptr;
    return f();
}

// Run `chunks` chunks through the two slots: prepare(i, slot) frames chunk i into the slot's
// pinned buffer, submit(i, slot) enqueues its copies and kernels and returns the finisher. The
// first error -- of a call, a copy or a finisher -- ends the run: both streams are waited for and
// the finishers still pending are dropped.
template <class Prep, class Submit>
int pipeline(Staging &st, int chunks, size_t slot_h, size_t slot_d, Prep prepare, Submit submit) {
    int err = 0;
    for (int i = 0; i < chunks && !err; ++i) {
        Slot &s = st.slot[i & 1];
        if ((err = drain(s))) break;
        if ((err = ensure_slot(s, slot_h, slot_d))) break;
        prepare(i, s);
        if ((err = run_late(s))) break;  // (the slot's previous chunk: its second-phase copy ran beside prepare)
        std::function<int()> fin;
        if ((err = submit(i, s, fin))) break;
        if (hipEventRecord(s.ev, st.stream) != hipSuccess) {
            err = -2;
            break;
        }
        s.finish = std::move(fin);
    }
    for (Slot &s : st.slot) {
        if (!err) err = drain(s);
        if (!err) err = run_late(s);
    }
    if (err) {
        (void)hipStreamSynchronize(st.stream);
        if (st.stream2) (void)hipStreamSynchronize(st.stream2);
        for (Slot &s : st.slot) s.finish = s.late = nullptr;
    }
    return err;
}

// shorthair_groups_stats: batched codec launches issued and groups coded by them.
std::atomic<long long> g_launches{0}, g_groups{0};
void count_launch(int groups) {
    g_launches.fetch_add(1, std::memory_order_relaxed);
    g_groups.fetch_add(groups, std::memory_order_relaxed);
}

// shorthair_groups_traffic: bytes the two calls copied host->device and device->host.
std::atomic<long long> g_h2d{0}, g_d2h{0};
hipError_t copy_h2d(void *dst, const void *src, size_t n, hipStream_t stream) {
    g_h2d.fetch_add(static_cast<long long>(n), std::memory_order_relaxed);
    return hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, stream);
}
hipError_t copy_d2h(void *dst, const void *src, size_t n, hipStream_t stream) {
    g_d2h.fetch_add(static_cast<long long>(n), std::memory_order_relaxed);
    return hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToHost, stream);
}
// `height` rows of `width` bytes, spitch apart on the device, dpitch apart on the host
hipError_t copy_d2h_2d(void *dst, size_t dpitch, const void *src, size_t spitch, size_t width, size_t height,
                       hipStream_t stream) {
    g_d2h.fetch_add(static_cast<long long>(width * height), std::memory_order_relaxed);
    return hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, stream);
}

// shorthair_groups_set_framing: 0 = host threads frame the blocks, 1 = the GPU does.
std::atomic<int> g_framing{0};

// shorthair_groups_set_delivery: 0 = whole recovered blocks come back and the host unframes them,
// 1 = the GPU unframes them and only the packed payloads come back.
std::atomic<int> g_delivery{0};

// shorthair_groups_set_wire: 0 = bare recovery blocks come back and the host writes the packet headers,
// 1 = the GPU emits the wire records and they come back whole.
std::atomic<int> g_wire{0};

// Bucket key of a group: the K of the compiled kernel that codes (k, m, B), or k itself.
int bucket_k(int k, int m, int B) {
    const int K = sh::fixed_kernel_k(k, m, B);
    return K > 0 ? K : k;
}

// Chunks of a var-k bucket: groups [start[c], start[c + 1]) of `ids`, cut so that a chunk's blocks
// plus per_group_out bytes per group stay within chunk_bytes() (at least one group per chunk).
std::vector<int> var_chunks(const std::vector<int> &ids, const std::function<int(int)> &k_of, int B,
                            size_t per_group_out) {
    std::vector<int> start{0};
    size_t bytes = 0;
    for (int j = 0; j < static_cast<int>(ids.size()); ++j) {
        const size_t need = static_cast<size_t>(k_of(ids[j])) * B + per_group_out;
        if (j > start.back() && bytes + need > chunk_bytes()) {
            start.push_back(j);
            bytes = 0;
        }
        bytes += need;
    }
    start.push_back(static_cast<int>(ids.size()));
    return start;
}
std::vector<int> uniform_chunks(int n, int per) {
    std::vector<int> start;
    for (int g = 0; g < n; g += per) start.push_back(g);
    start.push_back(n);
    return start;
}

// The k of a bucket's first group, the largest k in it, and whether its groups differ in k.
struct BucketK {
    int k, kmax;
    bool mixed;
};
template <class Info>
BucketK bucket_ks(const std::vector<Info> &info, const std::vector<int> &ids) {
    BucketK b{info[ids[0]].k, info[ids[0]].k, false};
    for (int id : ids) {
        b.mixed |= info[id].k != b.k;
        b.kmax = std::max(b.kmax, info[id].k);
    }
    return b;
}

// The chunk plan of a bucket, on every route. Chunk c is groups [start[c], start[c + 1]) of `ids`;
// blk0[j] / pay0[j] are the first block and the first payload byte of group j counted from the
// bucket's start (a group's payload bytes: what the device-framing route packs for it).
struct Chunks {
    std::vector<int> start;
    std::vector<long long> blk0, pay0;
    int chunks() const { return static_cast<int>(start.size()) - 1; }
    int g0(int c) const { return start[c]; }
    int gn(int c) const { return start[c + 1] - start[c]; }
    int nb(int c) const { return static_cast<int>(blk0[start[c + 1]] - blk0[start[c]]); }
    size_t pay(int c) const { return static_cast<size_t>(pay0[start[c + 1]] - pay0[start[c]]); }
    // group j of chunk c, counted from the chunk's start (j == gn(c): the chunk's end)
    long long blk(int c, int j) const { return blk0[start[c] + j] - blk0[start[c]]; }
    long long payoff(int c, int j) const { return pay0[start[c] + j] - pay0[start[c]]; }
    void put_first(int c, int *first) const {  // first[gn + 1] of the var-k codec calls
        for (int j = 0; j <= gn(c); ++j) first[j] = static_cast<int>(blk(c, j));
    }
};
// A uniform bucket is cut every chunk_bytes() / per_group groups, a mixed one by var_chunks with
// var_extra bytes per group; k_of(id) and pay_of(id) give a group's blocks and payload bytes
// (pay_of empty on the host-framing route, which has no use for pay0).
Chunks plan_chunks(const std::vector<int> &ids, bool mixed, int B, size_t per_group, size_t var_extra,
                   const std::function<int(int)> &k_of, const std::function<long long(int)> &pay_of) {
    const int n = static_cast<int>(ids.size());
    Chunks ch;
    ch.start = mixed ? var_chunks(ids, k_of, B, var_extra)
                     : uniform_chunks(n, static_cast<int>(std::max<size_t>(1, chunk_bytes() / per_group)));
    ch.blk0.assign(n + 1, 0);
    ch.pay0.assign(n + 1, 0);
    for (int j = 0; j < n; ++j) {
        ch.blk0[j + 1] = ch.blk0[j] + k_of(ids[j]);
        if (pay_of) ch.pay0[j + 1] = ch.pay0[j] + pay_of(ids[j]);
    }
    return ch;
}

// ---------------------------------------------------------------------------------------------
// Device delivery (shorthair_groups_set_delivery(1)), every m >= 2 bucket on both framing routes. After
// the decode call shorthair_unframe_batch packs the chunk's delivered payloads in a device-only region
// behind the slot's delivery-0 layout, and the D2H copy has two phases, as the host cannot know the
// payload total before the decode:
//   device region: payload[slots * min(B - 2, 65535)] | off[slots + 1] | len[slots] | scratch
//   pinned region: total (8 B) | len[slots] (4 B each) | rows[slots] | pad to 16 | the packed payloads
//   1. on the staging stream: len[], the decode's out rows and off[slots] (the total);
//   2. in the finisher, after the slot's event: `total` packed bytes on Staging::stream2 -- nothing
//      else is pending on the device for that region, and the staging stream keeps running the next
//      chunk. The wait for that copy and the on_packet calls from the pinned packed buffer, in
//      delivery 0's order, are the slot's `late` step: the pipeline runs it once the host threads have
//      framed the slot's next chunk (which touches neither region), before that chunk is submitted.
// ---------------------------------------------------------------------------------------------
inline size_t up16(size_t x) { return (x + 15) & ~size_t(15); }
struct D1Layout {
    size_t cap;                        // bytes of the packed-payload buffers
    size_t d_off, d_len, d_scr, d_end;  // device region (the payload at 0)
    size_t h_len, h_rows, h_pay, h_end;  // pinned region (the total at 0)
};
D1Layout d1_layout(size_t gn, int emax, int B) {
    const size_t slots = gn * emax;
    D1Layout L;
    L.cap = slots * static_cast<size_t>(std::min(B - 2, 65535));
    L.d_off = up16(L.cap);
    L.d_len = L.d_off + 8 * (slots + 1);
    L.d_scr = up16(L.d_len + 4 * slots);
    L.d_end = L.d_scr + static_cast<size_t>(shorthair_unframe_scratch_bytes(static_cast<int>(gn), emax));
    L.h_len = 16;
    L.h_rows = L.h_len + 4 * slots;
    L.h_pay = up16(L.h_rows + slots);
    L.h_end = L.h_pay + L.cap;
    return L;
}

// ---------------------------------------------------------------------------------------------
// The slot layout of one chunk: nb blocks in gn groups, `pay` payload bytes. One rule on every route:
// blocks and out are 16-byte aligned, count is 4-byte aligned, the delivery-1 regions are 16-byte
// aligned; route 0's rows and first[], copies of their own, start 16-byte aligned as well.
//
// Host framing (route 0): the pinned slot mirrors the device slot, and blocks, rows (receiver) and
// first[] (mixed-k buckets) go over in a copy each:
//   blocks[nb][B] | pad to 16 | rows[nb] | pad to 16 | first[gn + 1] (4 B each) | pad to 16 | outputs
// Device framing (route 1): the pinned slot carries only what the GPU cannot know, back to back, and
// goes over in one copy of h2d bytes; shorthair_frame_batch builds the blocks behind it:
//   off[nb] (8 B each) | len[nb] (4 B) | first[gn + 1] | rows[nb] | raw[nb] (receiver) | pad to 16 |
//   the payload bytes packed (recovery bodies among them, raw = 1) | pad to 16 | blocks[nb][B]
//   (device only) | pad to 16 | outputs; on the pinned side the outputs follow the copy, at up16(h2d).
// Outputs, sender: out[gn][m][B]. Receiver: out[gn][emax][B] (m == 1: [gn][B], pinned side only) |
// out rows[gn][emax] | pad to 4 | count[gn] (device only). The delivery-1 regions (d1_layout) do not
// follow the chunk's own end but the largest end among the bucket's chunks (slot_bytes), 16-byte
// aligned: a chunk's pinned region is still read by its `late` step after the slot's next chunk has
// been prepared, so no chunk's inputs or outputs may reach it.
// Wire route 1 (sender): wire[gn * m][3 + B] follows the layout above on the device side, 16-byte aligned
// and device only; on the pinned side the records take out's place, at h_out.
// ---------------------------------------------------------------------------------------------
struct SlotLayout {
    size_t off, len, first, rows, raw, pay, h2d;  // inputs (off, len, raw, pay, h2d: route 1 only)
    size_t blk, out, orow, cnt;                    // device side
    size_t wire, wire_n;                           // device side, wire route 1: the records and their bytes
    size_t h_out, h_orow;                          // pinned side
    size_t out_g;                                  // out bytes per group
    size_t h_end, d_end;                           // 16-byte aligned ends of all of the above
    size_t h_d1n, d_d1n;                           // bytes of the chunk's delivery-1 regions (0 without)
};
SlotLayout slot_layout(bool rx, int framing, bool mixed, size_t nb, size_t gn, size_t pay, int m, int emax,
                       int B, bool d1, bool wire = false) {
    const size_t F = mixed ? 4 * (gn + 1) : 0, R = rx ? nb : 0, orows = rx ? gn * emax : 0;
    SlotLayout L{};
    L.out_g = static_cast<size_t>(rx ? (m >= 2 ? emax : 1) : m) * B;
    if (framing == 1) {
        L.len = 8 * nb;
        L.first = L.len + 4 * nb;
        L.rows = L.first + F;
        L.raw = L.rows + R;
        L.pay = up16(L.raw + R);
        L.h2d = L.pay + pay;
        L.blk = up16(L.h2d);
        L.out = up16(L.blk + nb * B);
        L.h_out = up16(L.h2d);
    } else {
        L.rows = up16(nb * B);
        L.first = up16(L.rows + R);
        L.out = L.h_out = up16(L.first + F);
    }
    L.orow = L.out + gn * L.out_g;
    L.h_orow = L.h_out + gn * L.out_g;
    L.cnt = (L.orow + orows + 3) & ~size_t(3);
    L.d_end = up16(L.cnt + (rx ? 4 * gn : 0));
    L.h_end = up16(L.h_orow + orows);
    if (wire) {
        L.wire = L.d_end;
        L.wire_n = gn * m * (static_cast<size_t>(B) + 3);
        L.d_end = up16(L.wire + L.wire_n);
        L.h_end = up16(L.h_out + L.wire_n);
    }
    L.d_d1n = d1 ? d1_layout(gn, emax, B).d_end : 0;
    L.h_d1n = d1 ? d1_layout(gn, emax, B).h_end : 0;
    return L;
}

// Block x of a chunk into the pinned slot; its payload starts p bytes into the chunk's payload bytes.
// Route 0 frames it as the reference does, "[len u16 LE][payload][zeros up to B]" (EncodeQueued
// :540-557, RecoverGroup :710-725), or copies a recovery packet's block verbatim (raw, len == B:
// :727-735). Route 1 packs the bytes alone and notes off and len: the GPU frames them.
inline void put_block(int framing, uint8_t *h, const SlotLayout &L, int B, long long x, long long p,
                      const void *src, int len, bool raw) {
    const uint8_t *from = static_cast<const uint8_t *>(src);
    if (framing == 1) {
        reinterpret_cast<long long *>(h + L.off)[x] = p;
        reinterpret_cast<int *>(h + L.len)[x] = len;
        framing_copy(h + L.pay + p, from, len);
        return;
    }
    uint8_t *blk = h + L.blk + static_cast<size_t>(x) * B;
    if (raw) {
        framing_copy(blk, from, B);
        return;
    }
    put_u16(blk, len);
    framing_copy(blk + 2, from, len);
    std::memset(blk + 2 + len, 0, B - 2 - len);
}

// What a chunk's codec call reads, from the pinned slot prepare() filled to the device slot: route 0
// copies blocks, rows and first[]; route 1 copies the head and frames the blocks on the GPU.
int submit_inputs(Staging &st, Slot &s, int framing, const SlotLayout &L, bool rx, bool mixed, int nb, int gn,
                  size_t pay, int B) {
    uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
    if (framing == 1) {
        SG_CHECK(copy_h2d(d, h, L.h2d, st.stream));
        return shorthair_frame_batch(B, nb, d + L.pay, static_cast<long long>(pay),
                                     reinterpret_cast<const long long *>(d + L.off),
                                     reinterpret_cast<const int *>(d + L.len), rx ? d + L.raw : nullptr, d + L.blk,
                                     st.stream);
    }
    SG_CHECK(copy_h2d(d + L.blk, h + L.blk, static_cast<size_t>(nb) * B, st.stream));
    if (rx) SG_CHECK(copy_h2d(d + L.rows, h + L.rows, nb, st.stream));
    if (mixed) SG_CHECK(copy_h2d(d + L.first, h + L.first, (gn + 1) * sizeof(int), st.stream));
    return 0;
}

// Pinned and device bytes a bucket's slots need. The delivery-1 regions of every chunk start at
// h_d1 / d_d1, behind the largest chunk's layout; the slot ends behind the largest such region.
struct SlotBytes {
    size_t h_d1 = 0, d_d1 = 0, nh = 0, nd = 0;
};
template <class LayoutOf>
SlotBytes slot_bytes(const Chunks &ch, LayoutOf layout) {
    SlotBytes b;
    for (int c = 0; c < ch.chunks(); ++c) {
        const SlotLayout L = layout(c);
        b.h_d1 = std::max(b.h_d1, L.h_end);
        b.d_d1 = std::max(b.d_d1, L.d_end);
        b.nh = std::max(b.nh, L.h_d1n);
        b.nd = std::max(b.nd, L.d_d1n);
    }
    b.nh += b.h_d1;
    b.nd += b.d_d1;
    return b;
}

// ---------------------------------------------------------------------------------------------
// Sender
// ---------------------------------------------------------------------------------------------
struct TxInfo {
    int k, m, B;  // m after truncation to 256 - k; B = block bytes (k >= 2)
};

bool tx_info(const ShorthairTxGroup &g, TxInfo &t) {
    if (g.k < 1 || g.k > 255 || g.m < 1 || !g.lens || !g.packets || !g.out) return false;
    int largest = 0;
    for (int x = 0; x < g.k; ++x) {
        if (!g.packets[x]) return false;
        largest = std::max(largest, static_cast<int>(g.lens[x]));
    }
    t.k = g.k;
    t.m = std::min(g.m, 256 - g.k);                   // Shorthair.cpp:501-504
    t.B = g.k == 1 ? largest : roundup8(2 + largest);  // :531-537 (k == 1: the payload itself)
    return true;
}

// GenerateRecoveryBlock :598-608: "[k+i][k-1][m-1][block i]" for a group's m recovery blocks rec[m][B]
void write_recovery_packets(ShorthairTxGroup &g, int m, int B, const uint8_t *rec) {
    for (int y = 0; y < m; ++y) {
        uint8_t *p = g.out + static_cast<size_t>(y) * g.out_stride;
        p[0] = static_cast<uint8_t>(g.k + y);
        p[1] = static_cast<uint8_t>(g.k - 1);
        p[2] = static_cast<uint8_t>(m - 1);
        std::memcpy(p + 3, rec + static_cast<size_t>(y) * B, B);
    }
}

// One (K, m, B) bucket of the sender, groups `ids`, through the pipeline on framing route `framing`;
// wire: the GPU emits the recovery packets.
int encode_bucket(Staging &st, int framing, bool wire, ShorthairTxGroup *groups, const std::vector<TxInfo> &info,
                  const std::vector<int> &ids, int m, int B) {
    const BucketK bk = bucket_ks(info, ids);
    const size_t out_g = static_cast<size_t>(m) * B;
    std::function<long long(int)> pay_of;
    if (framing == 1)
        pay_of = [&](int id) {
            long long p = 0;
            for (int x = 0; x < groups[id].k; ++x) p += groups[id].lens[x];
            return p;
        };
    const Chunks ch = plan_chunks(ids, bk.mixed, B, static_cast<size_t>(bk.k) * B + out_g, out_g + 4,
                                  [&](int id) { return info[id].k; }, pay_of);
    auto layout = [&](int c) {
        return slot_layout(false, framing, bk.mixed, ch.nb(c), ch.gn(c), ch.pay(c), m, 0, B, false, wire);
    };
    const SlotBytes sb = slot_bytes(ch, layout);
    auto prepare = [&](int c, Slot &s) {
        const SlotLayout L = layout(c);
        uint8_t *h = static_cast<uint8_t *>(s.h);
        if (bk.mixed) ch.put_first(c, reinterpret_cast<int *>(h + L.first));
        parallel_for(ch.gn(c), [&](int j) {
            const ShorthairTxGroup &g = groups[ids[ch.g0(c) + j]];
            long long p = ch.payoff(c, j);
            for (int x = 0; x < g.k; ++x) {
                put_block(framing, h, L, B, ch.blk(c, j) + x, p, g.packets[x], g.lens[x], false);
                p += g.lens[x];
            }
            framing_fence();
        });
    };
    auto submit = [&](int c, Slot &s, std::function<int()> &fin) -> int {
        const int g0 = ch.g0(c), gn = ch.gn(c), nb = ch.nb(c);
        const SlotLayout L = layout(c);
        uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
        int rc = submit_inputs(st, s, framing, L, false, bk.mixed, nb, gn, ch.pay(c), B);
        if (rc != 0) return rc;
        rc = bk.mixed ? cauchy_256_encode_batch_var(bk.kmax, m, B, gn, reinterpret_cast<const int *>(d + L.first), nb,
                                                    d + L.blk, d + L.out, st.stream)
                      : cauchy_256_encode_batch(bk.k, m, B, gn, d + L.blk, d + L.out, st.stream);
        if (rc != 0) return rc;
        count_launch(gn);
        // wire route 1: the packets are built on the GPU and come back instead of the bare blocks
        if (wire) {
            rc = shorthair_wire_emit_batch(bk.mixed ? bk.kmax : bk.k, m, B, gn,
                                           bk.mixed ? reinterpret_cast<const int *>(d + L.first) : nullptr, nb,
                                           d + L.out, d + L.wire, st.stream);
            if (rc != 0) return rc;
        }
        SG_CHECK(copy_d2h(h + L.h_out, d + (wire ? L.wire : L.out), wire ? L.wire_n : gn * out_g, st.stream));
        const uint8_t *rec = h + L.h_out;
        const size_t wire_g = static_cast<size_t>(m) * (3 + B);  // a group's m records, laid out as g.out is
        fin = [&, g0, gn, rec, wire_g]() {
            parallel_for(gn, [&](int j) {
                ShorthairTxGroup &g = groups[ids[g0 + j]];
                if (wire)
                    std::memcpy(g.out, rec + static_cast<size_t>(j) * wire_g, wire_g);
                else
                    write_recovery_packets(g, m, B, rec + static_cast<size_t>(j) * out_g);
            });
            return 0;
        };
        return 0;
    };
    return pipeline(st, ch.chunks(), sb.nh, sb.nd, prepare, submit);
}

}  // namespace

extern "C" int shorthair_recovery_packet_bytes(int k, const unsigned short *lens) {
    if (k < 1 || k > 255 || !lens) return -1;
    int largest = 0;
    for (int x = 0; x < k; ++x) largest = std::max(largest, static_cast<int>(lens[x]));
    return k == 1 ? 2 + largest : 3 + roundup8(2 + largest);
}

extern "C" int shorthair_encode_groups(ShorthairTxGroup *groups, int count) {
    if (count < 0 || (count > 0 && !groups)) return -1;
    const int framing = g_framing.load(std::memory_order_relaxed);
    const bool wire = g_wire.load(std::memory_order_relaxed) == 1;
    std::vector<TxInfo> info(count);
    for (int i = 0; i < count; ++i) {
        if (!tx_info(groups[i], info[i])) return -1;
        const TxInfo &t = info[i];
        const long long stride = t.k == 1 ? 2 + t.B : 3 + t.B;
        if (static_cast<long long>(groups[i].out_capacity) < stride * t.m) return -1;
    }
    // k == 1: "[1][0][payload]" for every request (GenerateRecoveryBlock :587-596), no codec
    std::map<std::tuple<int, int, int>, std::vector<int>> buckets;
    for (int i = 0; i < count; ++i) {
        ShorthairTxGroup &g = groups[i];
        const TxInfo &t = info[i];
        g.m_out = t.m;
        if (t.k == 1) {
            g.out_stride = 2 + t.B;
            for (int y = 0; y < t.m; ++y) {
                uint8_t *p = g.out + static_cast<size_t>(y) * g.out_stride;
                p[0] = 1;
                p[1] = 0;
                std::memcpy(p + 2, g.packets[0], g.lens[0]);
            }
        } else {
            g.out_stride = 3 + t.B;
            buckets[std::make_tuple(bucket_k(t.k, t.m, t.B), t.m, t.B)].push_back(i);
        }
    }
    if (buckets.empty()) return 0;
    Staging &st = staging();
    std::lock_guard<std::mutex> lock(st.mu);
    if (int rc = ensure_staging(st)) return rc;
    for (auto &kv : buckets)
        if (int rc = encode_bucket(st, framing, wire, groups, info, kv.second, std::get<1>(kv.first),
                                   std::get<2>(kv.first)))
            return rc;
    return 0;
}

// ---------------------------------------------------------------------------------------------
// Receiver
// ---------------------------------------------------------------------------------------------
namespace {

struct RxInfo {
    int k = 0, m = 0, B = 0, use = 0;  // use: recovery packets listed (k - n_orig); 0 = skip
};

// -1 malformed, 0 skip, 1 decode (k >= 2), 2 k == 1 special form
int rx_info(const ShorthairRxGroup &g, RxInfo &r) {
    if (g.n_orig < 0 || g.n_rec < 0 || (g.n_orig && (!g.orig_ids || !g.orig_data || !g.orig_lens)) ||
        (g.n_rec && (!g.rec_packets || !g.rec_lens)))
        return -1;
    if (g.n_rec == 0) return 0;  // nothing to decode from
    for (int j = 0; j < g.n_rec; ++j)
        if (!g.rec_packets[j] || g.rec_lens[j] < 2) return -1;
    const int k = g.rec_packets[0][1] + 1;  // "[id][k-1]..." (OnData :785-786)
    for (int j = 1; j < g.n_rec; ++j)
        if (g.rec_packets[j][1] + 1 != k) return -1;
    r.k = k;
    if (k == 1) return g.n_orig == 0 ? 2 : 0;  // :858-866 ("a redundant packet won")
    if (g.n_orig >= k || g.n_orig + g.n_rec < k) return 0;  // CanRecover() (ShorthairDetails.hpp:328)
    const uint8_t *last = g.rec_packets[g.n_rec - 1];
    r.m = last[2] + 1;                       // :878 recovery_count = data[0] + 1
    r.B = g.rec_lens[g.n_rec - 1] - 3;       // :877 largest_len = data_len - 1
    if (r.B < 8 || r.B % 8 != 0 || k + r.m > 256) return -1;
    bool seen[256] = {false};
    for (int i = 0; i < g.n_orig; ++i) {
        const int id = g.orig_ids[i];
        if (id >= k || seen[id] || g.orig_lens[i] > r.B - 2 || !g.orig_data[i]) return -1;
        seen[id] = true;
    }
    r.use = k - g.n_orig;  // RecoverGroup :727-735: recovery packets until k blocks
    for (int j = 0; j < r.use; ++j) {
        const int id = g.rec_packets[j][0];
        if (id < k || id >= k + r.m || seen[id] || g.rec_lens[j] != r.B + 3) return -1;
        seen[id] = true;
    }
    return 1;
}

// The delivery-1 tail of a chunk of gn groups (chunk-local group j = ids[g0 + j]) whose decode call has
// been enqueued: d_out [gn][emax][B], d_orow [gn][emax], d_cnt [gn] in device memory; the regions
// start d_base / h_base bytes into the slot. A failure in the finisher is what it returns.
int deliver1_tail(Staging &st, Slot &s, size_t d_base, size_t h_base, int B, int gn, int emax,
                  const uint8_t *d_out, const uint8_t *d_orow, const int *d_cnt,
                  const ShorthairRxGroup *groups, const std::vector<RxInfo> &info, const std::vector<int> &ids,
                  int g0, shorthair_on_packet_fn on_packet, void *cb_ctx, std::function<int()> &fin) {
    const D1Layout L = d1_layout(gn, emax, B);
    const size_t slots = static_cast<size_t>(gn) * emax;
    uint8_t *h = static_cast<uint8_t *>(s.h) + h_base, *d = static_cast<uint8_t *>(s.d) + d_base;
    if (!st.stream2) SG_CHECK(hipStreamCreateWithFlags(&st.stream2, hipStreamNonBlocking));
    const int rc = shorthair_unframe_batch(B, gn, emax, emax, d_out, d_cnt, d, static_cast<long long>(L.cap),
                                           reinterpret_cast<long long *>(d + L.d_off),
                                           reinterpret_cast<int *>(d + L.d_len), d + L.d_scr, st.stream);
    if (rc != 0) return rc;
    SG_CHECK(copy_d2h(h, d + L.d_off + 8 * slots, 8, st.stream));
    SG_CHECK(copy_d2h(h + L.h_len, d + L.d_len, 4 * slots, st.stream));
    SG_CHECK(copy_d2h(h + L.h_rows, d_orow, slots, st.stream));
    hipStream_t second = st.stream2;
    fin = [=, &s, &info, &ids]() {
        long long total;
        std::memcpy(&total, h, 8);
        if (total < 0 || static_cast<unsigned long long>(total) > L.cap) return -2;
        if (total > 0 && copy_d2h(h + L.h_pay, d, static_cast<size_t>(total), second) != hipSuccess) return -2;
        s.late = [=, &info, &ids]() {
            if (hipStreamSynchronize(second) != hipSuccess) return -2;
            if (!on_packet) return 0;
            const int *len = reinterpret_cast<const int *>(h + L.h_len);
            const uint8_t *pay = h + L.h_pay;
            for (int j = 0; j < gn; ++j) {  // RecoverGroup :741-756; the prefix rule was applied on the GPU
                const int gi = ids[g0 + j];
                const int e = info[gi].k - groups[gi].n_orig;
                for (int i = 0; i < emax; ++i) {
                    const int l = len[static_cast<size_t>(j) * emax + i];
                    if (l < 0) continue;
                    if (i < e) on_packet(cb_ctx, gi, h[L.h_rows + static_cast<size_t>(j) * emax + i], pay, l);
                    pay += l;
                }
            }
            return 0;
        };
        return 0;
    };
    return 0;
}

// Group g's k blocks and rows[] into the pinned slot from block x / payload byte p of its chunk: the
// originals in arrival order (RecoverGroup :710-725), then the `use` recovery packets' blocks (:727-735).
void put_rx_group(int framing, uint8_t *h, const SlotLayout &L, int B, const ShorthairRxGroup &g, int use,
                  long long x, long long p) {
    uint8_t *rows = h + L.rows, *raw = h + L.raw;  // raw[]: route 1 only
    for (int i = 0; i < g.n_orig; ++i, ++x) {
        rows[x] = g.orig_ids[i];
        if (framing == 1) raw[x] = 0;
        put_block(framing, h, L, B, x, p, g.orig_data[i], g.orig_lens[i], false);
        p += g.orig_lens[i];
    }
    for (int i = 0; i < use; ++i, ++x, p += B) {
        rows[x] = g.rec_packets[i][0];
        if (framing == 1) raw[x] = 1;
        put_block(framing, h, L, B, x, p, g.rec_packets[i] + 3, B, true);
    }
    framing_fence();
}

// The host delivery of a chunk whose outputs are in the pinned slot (RecoverGroup :741-756): the
// recovered blocks out[gn][out_g] whose length prefix fits, ids from orow[gn][emax] (m >= 2) or the
// one missing original (m == 1).
void deliver_host(const ShorthairRxGroup *groups, const std::vector<RxInfo> &info, const int *ids, int gn, int m,
                  int emax, int B, const uint8_t *out, size_t out_g, const uint8_t *orow,
                  shorthair_on_packet_fn on_packet, void *cb_ctx) {
    for (int j = 0; j < gn; ++j) {
        const int gi = ids[j];
        const ShorthairRxGroup &g = groups[gi];
        const int kg = info[gi].k, e = kg - g.n_orig;
        int missing = -1;
        if (m < 2) {
            bool seen[256] = {false};
            for (int i = 0; i < g.n_orig; ++i) seen[g.orig_ids[i]] = true;
            for (int x = 0; x < kg && missing < 0; ++x)
                if (!seen[x]) missing = x;
        }
        for (int i = 0; i < e; ++i) {
            const uint8_t *blk = out + static_cast<size_t>(j) * out_g + static_cast<size_t>(i) * B;
            const int id = m >= 2 ? orow[static_cast<size_t>(j) * emax + i] : missing;
            const int len = static_cast<int>(get_u16(blk));
            if (len <= B - 2) on_packet(cb_ctx, gi, id, blk + 2, len);
        }
    }
}

// One (K, m, B) bucket of the receiver, groups `ids`, through the pipeline on framing route `framing`;
// d1: device delivery (m >= 2).
int recover_bucket(Staging &st, int framing, bool d1, const ShorthairRxGroup *groups,
                   const std::vector<RxInfo> &info, const std::vector<int> &ids, int m, int B,
                   shorthair_on_packet_fn on_packet, void *cb_ctx) {
    const BucketK bk = bucket_ks(info, ids);
    const int emax = std::min(bk.kmax, m);
    const size_t out_g = static_cast<size_t>(m >= 2 ? emax : 1) * B;
    // per group: blocks k*B, rows k; out; out rows emax; count 4
    std::function<long long(int)> pay_of;
    if (framing == 1)
        pay_of = [&](int id) {
            long long p = static_cast<long long>(info[id].use) * B;
            for (int i = 0; i < groups[id].n_orig; ++i) p += groups[id].orig_lens[i];
            return p;
        };
    const Chunks ch = plan_chunks(ids, bk.mixed, B, static_cast<size_t>(bk.k) * B + bk.k + out_g + emax + 4,
                                  out_g + emax + 8 + 256, [&](int id) { return info[id].k; }, pay_of);
    auto layout = [&](int c) {
        return slot_layout(true, framing, bk.mixed, ch.nb(c), ch.gn(c), ch.pay(c), m, emax, B, d1);
    };
    const SlotBytes sb = slot_bytes(ch, layout);
    auto prepare = [&](int c, Slot &s) {
        const SlotLayout L = layout(c);
        uint8_t *h = static_cast<uint8_t *>(s.h);
        if (bk.mixed) ch.put_first(c, reinterpret_cast<int *>(h + L.first));
        parallel_for(ch.gn(c), [&](int j) {
            const int gi = ids[ch.g0(c) + j];
            put_rx_group(framing, h, L, B, groups[gi], info[gi].use, ch.blk(c, j), ch.payoff(c, j));
        });
    };
    auto submit = [&](int c, Slot &s, std::function<int()> &fin) -> int {
        const int g0 = ch.g0(c), gn = ch.gn(c), nb = ch.nb(c);
        const SlotLayout L = layout(c);
        uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
        int rc = submit_inputs(st, s, framing, L, true, bk.mixed, nb, gn, ch.pay(c), B);
        if (rc != 0) return rc;
        int *d_cnt = reinterpret_cast<int *>(d + L.cnt);
        if (m < 2)  // (a uniform bucket) the one erasure lands in place in block k-1 of each group
            rc = cauchy_256_decode_batch(bk.k, m, B, gn, d + L.blk, d + L.rows, st.stream);
        else if (bk.mixed)
            rc = cauchy_256_decode_batch_out_var(bk.kmax, m, B, gn, reinterpret_cast<const int *>(d + L.first), nb,
                                                 d + L.blk, d + L.rows, d + L.out, d + L.orow, d_cnt, st.stream);
        else
            rc = cauchy_256_decode_batch_out(bk.k, m, B, gn, d + L.blk, d + L.rows, d + L.out, d + L.orow, d_cnt,
                                             st.stream);
        if (rc != 0) return rc;
        count_launch(gn);
        if (d1)
            return deliver1_tail(st, s, sb.d_d1, sb.h_d1, B, gn, emax, d + L.out, d + L.orow, d_cnt, groups, info, ids,
                                 g0, on_packet, cb_ctx, fin);
        if (m >= 2) {
            SG_CHECK(copy_d2h(h + L.h_out, d + L.out, gn * out_g, st.stream));
            SG_CHECK(copy_d2h(h + L.h_orow, d + L.orow, gn * static_cast<size_t>(emax), st.stream));
        } else {
            SG_CHECK(copy_d2h_2d(h + L.h_out, B, d + L.blk + static_cast<size_t>(bk.k - 1) * B,
                                 static_cast<size_t>(bk.k) * B, B, gn, st.stream));
        }
        // (decode only, no on_packet: the empty finisher still makes the pipeline wait for the chunk
        // before the slot is reused and before the call returns)
        const uint8_t *out = h + L.h_out, *orow = h + L.h_orow;
        fin = [&, g0, gn, out, orow]() {
            if (on_packet)
                deliver_host(groups, info, ids.data() + g0, gn, m, emax, B, out, out_g, orow, on_packet, cb_ctx);
            return 0;
        };
        return 0;
    };
    return pipeline(st, ch.chunks(), sb.nh, sb.nd, prepare, submit);
}

}  // namespace

extern "C" int shorthair_recover_groups(const ShorthairRxGroup *groups, int count,
                                        shorthair_on_packet_fn on_packet, void *cb_ctx) {
    if (count < 0 || (count > 0 && !groups)) return -1;
    const int framing = g_framing.load(std::memory_order_relaxed);
    const int delivery = g_delivery.load(std::memory_order_relaxed);
    std::vector<RxInfo> info(count);
    std::vector<int> kind(count);
    for (int i = 0; i < count; ++i)
        if ((kind[i] = rx_info(groups[i], info[i])) < 0) return -1;
    int decoded = 0;
    std::map<std::tuple<int, int, int>, std::vector<int>> buckets;
    for (int i = 0; i < count; ++i) {
        if (kind[i] == 2) {
            const ShorthairRxGroup &g = groups[i];
            if (on_packet) on_packet(cb_ctx, i, 0, g.rec_packets[0] + 2, g.rec_lens[0] - 2);
            ++decoded;
        } else if (kind[i] == 1) {
            buckets[std::make_tuple(info[i].m >= 2 ? bucket_k(info[i].k, info[i].m, info[i].B) : info[i].k,
                                    info[i].m, info[i].B)]
                .push_back(i);
        }
    }
    if (buckets.empty()) return decoded;
    Staging &st = staging();
    std::lock_guard<std::mutex> lock(st.mu);
    if (int rc = ensure_staging(st)) return rc;
    for (auto &kv : buckets) {
        const int m = std::get<1>(kv.first), B = std::get<2>(kv.first);
        if (int rc = recover_bucket(st, framing, delivery == 1 && m >= 2, groups, info, kv.second, m, B, on_packet,
                                    cb_ctx))
            return rc;
        decoded += static_cast<int>(kv.second.size());
    }
    return decoded;
}

extern "C" int shorthair_groups_stats(long long *launches, long long *groups) {
    if (launches) *launches = g_launches.load(std::memory_order_relaxed);
    if (groups) *groups = g_groups.load(std::memory_order_relaxed);
    return 0;
}

extern "C" int shorthair_groups_set_framing(int where) {
    if (where != 0 && where != 1) return -1;
    return g_framing.exchange(where, std::memory_order_relaxed);
}

extern "C" int shorthair_groups_set_delivery(int where) {
    if (where != 0 && where != 1) return -1;
    return g_delivery.exchange(where, std::memory_order_relaxed);
}

extern "C" int shorthair_groups_set_wire(int where) {
    if (where != 0 && where != 1) return -1;
    return g_wire.exchange(where, std::memory_order_relaxed);
}

extern "C" int shorthair_groups_traffic(long long *h2d_bytes, long long *d2h_bytes) {
    if (h2d_bytes) *h2d_bytes = g_h2d.load(std::memory_order_relaxed);
    if (d2h_bytes) *d2h_bytes = g_d2h.load(std::memory_order_relaxed);
    return 0;
}
