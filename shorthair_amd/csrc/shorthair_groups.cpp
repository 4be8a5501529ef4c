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
// shorthair_groups_set_framing(1) moves the framing to the GPU ("Device framing" below): the host
// threads then pack only the payload bytes into the pinned slot, shorthair_frame_batch builds the
// blocks in device memory, and everything else -- buckets, chunks, codec calls, finishers -- is shared.
//
// shorthair_groups_set_delivery(1) moves the receiver's unframing to the GPU ("Device delivery" below):
// shorthair_unframe_batch packs the recovered payloads of an m >= 2 chunk in device memory and only
// they, their lengths and rows come back, in two copies; the callbacks are the same.
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
    std::function<void()> finish;  // empty: nothing pending
    std::function<void()> late;    // device delivery: set by finish, run once the next chunk is prepared
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
    f();
    return 0;
}

void run_late(Slot &s) {
    if (!s.late) return;
    auto f = std::move(s.late);
    s.late = nullptr;
    f();
}

// Run `chunks` chunks through the two slots: prepare(i, slot) frames chunk i into the slot's
// pinned buffer, submit(i, slot) enqueues its copies and kernels and returns the finisher.
template <class Prep, class Submit>
int pipeline(Staging &st, int chunks, size_t slot_h, size_t slot_d, Prep prepare, Submit submit) {
    int err = 0;
    for (int i = 0; i < chunks && !err; ++i) {
        Slot &s = st.slot[i & 1];
        if ((err = drain(s))) break;
        if ((err = ensure_slot(s, slot_h, slot_d))) break;
        prepare(i, s);
        run_late(s);  // (the slot's previous chunk: its second-phase copy ran beside prepare)
        std::function<void()> fin;
        if ((err = submit(i, s, fin))) break;
        if (hipEventRecord(s.ev, st.stream) != hipSuccess) {
            err = -2;
            break;
        }
        s.finish = std::move(fin);
    }
    for (Slot &s : st.slot) {
        if (err) {
            (void)hipStreamSynchronize(st.stream);
            if (st.stream2) (void)hipStreamSynchronize(st.stream2);
            s.finish = nullptr;
            s.late = nullptr;
        } else if (int e = drain(s)) {
            err = e;
        } else {
            run_late(s);
        }
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

// shorthair_groups_set_framing: 0 = host threads frame the blocks, 1 = the GPU does.
std::atomic<int> g_framing{0};

// shorthair_groups_set_delivery: 0 = whole recovered blocks come back and the host unframes them,
// 1 = the GPU unframes them and only the packed payloads come back.
std::atomic<int> g_delivery{0};

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

// ---------------------------------------------------------------------------------------------
// Device framing (shorthair_groups_set_framing(1)). A chunk's pinned slot carries only what the GPU
// cannot know, back to back, and goes over in one H2D copy:
//   off[nb] (8 B each) | len[nb] (4 B) | first[gn + 1] (4 B, mixed-k buckets) | rows[nb] | raw[nb]
//   (receiver) | pad to 16 | the payload bytes packed (recovery bodies among them, raw = 1)
// shorthair_frame_batch builds blocks[nb][B] from it in a device-only region behind the copy, the
// codec call of the host-framing route runs on those blocks, and the outputs follow them. The
// pinned side holds the outputs right behind the copy (DevLayout::h2d rounded up to 16).
// Buckets, chunk cuts (device bytes of blocks + outputs), launches and finishers are those of the
// host-framing route.
// ---------------------------------------------------------------------------------------------
struct DevLayout {
    size_t o_len, o_first, o_rows, o_raw, o_pay, h2d;  // h2d = o_pay + payload bytes
};
inline size_t up16(size_t x) { return (x + 15) & ~size_t(15); }
DevLayout dev_layout(size_t nb, size_t gn, size_t pay, bool mixed, bool rx) {
    DevLayout L;
    L.o_len = 8 * nb;
    L.o_first = L.o_len + 4 * nb;
    L.o_rows = L.o_first + (mixed ? 4 * (gn + 1) : 0);
    L.o_raw = L.o_rows + (rx ? nb : 0);
    L.o_pay = up16(L.o_raw + (rx ? nb : 0));
    L.h2d = L.o_pay + pay;
    return L;
}

// Chunk c of a bucket is groups [start[c], start[c + 1]) of `ids`; blk0[j] / pay0[j] are the first
// block and the first payload byte of group j counted from the bucket's start.
struct DevChunks {
    std::vector<int> start;
    std::vector<long long> blk0, pay0;
    int chunks() const { return static_cast<int>(start.size()) - 1; }
    int g0(int c) const { return start[c]; }
    int gn(int c) const { return start[c + 1] - start[c]; }
    int nb(int c) const { return static_cast<int>(blk0[start[c + 1]] - blk0[start[c]]); }
    size_t pay(int c) const { return static_cast<size_t>(pay0[start[c + 1]] - pay0[start[c]]); }
};
std::vector<int> uniform_chunks(int n, int per) {
    std::vector<int> start;
    for (int g = 0; g < n; g += per) start.push_back(g);
    start.push_back(n);
    return start;
}

int encode_bucket_dev(Staging &st, ShorthairTxGroup *groups, const std::vector<TxInfo> &info,
                      const std::vector<int> &ids, int m, int B, int k, int kmax, bool mixed) {
    const int n = static_cast<int>(ids.size());
    const size_t out_g = static_cast<size_t>(m) * B;
    DevChunks ch;
    if (mixed)
        ch.start = var_chunks(ids, [&](int id) { return info[id].k; }, B, out_g + 4);
    else
        ch.start = uniform_chunks(n, static_cast<int>(std::max<size_t>(1, chunk_bytes() / (static_cast<size_t>(k) * B + out_g))));
    ch.blk0.assign(n + 1, 0);
    ch.pay0.assign(n + 1, 0);
    for (int j = 0; j < n; ++j) {
        const ShorthairTxGroup &g = groups[ids[j]];
        long long p = 0;
        for (int x = 0; x < g.k; ++x) p += g.lens[x];
        ch.blk0[j + 1] = ch.blk0[j] + g.k;
        ch.pay0[j + 1] = ch.pay0[j] + p;
    }
    size_t nh = 0, nd = 0;
    for (int c = 0; c < ch.chunks(); ++c) {
        const size_t head = up16(dev_layout(ch.nb(c), ch.gn(c), ch.pay(c), mixed, false).h2d);
        nh = std::max(nh, head + ch.gn(c) * out_g);
        nd = std::max(nd, head + static_cast<size_t>(ch.nb(c)) * B + ch.gn(c) * out_g);
    }
    auto prepare = [&](int c, Slot &s) {
        const int g0 = ch.g0(c), gn = ch.gn(c);
        const DevLayout L = dev_layout(ch.nb(c), gn, ch.pay(c), mixed, false);
        uint8_t *h = static_cast<uint8_t *>(s.h);
        long long *off = reinterpret_cast<long long *>(h);
        int *len = reinterpret_cast<int *>(h + L.o_len), *first = reinterpret_cast<int *>(h + L.o_first);
        if (mixed)
            for (int j = 0; j <= gn; ++j) first[j] = static_cast<int>(ch.blk0[g0 + j] - ch.blk0[g0]);
        parallel_for(gn, [&](int j) {
            const ShorthairTxGroup &g = groups[ids[g0 + j]];
            const long long b = ch.blk0[g0 + j] - ch.blk0[g0];
            long long p = ch.pay0[g0 + j] - ch.pay0[g0];
            for (int x = 0; x < g.k; ++x) {  // EncodeQueued :540-557: the payload only; the GPU frames it
                const int l = g.lens[x];
                off[b + x] = p;
                len[b + x] = l;
                framing_copy(h + L.o_pay + p, static_cast<const uint8_t *>(g.packets[x]), l);
                p += l;
            }
            framing_fence();
        });
    };
    auto submit = [&](int c, Slot &s, std::function<void()> &fin) -> int {
        const int g0 = ch.g0(c), gn = ch.gn(c), nb = ch.nb(c);
        const DevLayout L = dev_layout(nb, gn, ch.pay(c), mixed, false);
        uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
        const size_t o_blk = up16(L.h2d), o_out = o_blk + static_cast<size_t>(nb) * B, h_out = up16(L.h2d);
        SG_CHECK(copy_h2d(d, h, L.h2d, st.stream));
        int rc = shorthair_frame_batch(B, nb, d + L.o_pay, static_cast<long long>(ch.pay(c)),
                                       reinterpret_cast<const long long *>(d), reinterpret_cast<const int *>(d + L.o_len),
                                       nullptr, d + o_blk, st.stream);
        if (rc != 0) return rc;
        rc = mixed ? cauchy_256_encode_batch_var(kmax, m, B, gn, reinterpret_cast<const int *>(d + L.o_first), nb,
                                                 d + o_blk, d + o_out, st.stream)
                   : cauchy_256_encode_batch(k, m, B, gn, d + o_blk, d + o_out, st.stream);
        if (rc != 0) return rc;
        count_launch(gn);
        SG_CHECK(copy_d2h(h + h_out, d + o_out, gn * out_g, st.stream));
        fin = [&, g0, gn, h, h_out, out_g]() {
            parallel_for(gn, [&](int j) {  // GenerateRecoveryBlock :598-608: "[k+i][k-1][m-1][block i]"
                ShorthairTxGroup &g = groups[ids[g0 + j]];
                const uint8_t *rec = h + h_out + static_cast<size_t>(j) * out_g;
                for (int y = 0; y < m; ++y) {
                    uint8_t *p = g.out + static_cast<size_t>(y) * g.out_stride;
                    p[0] = static_cast<uint8_t>(g.k + y);
                    p[1] = static_cast<uint8_t>(g.k - 1);
                    p[2] = static_cast<uint8_t>(m - 1);
                    std::memcpy(p + 3, rec + static_cast<size_t>(y) * B, B);
                }
            });
        };
        return 0;
    };
    return pipeline(st, ch.chunks(), nh, nd, prepare, submit);
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
    for (auto &kv : buckets) {
        const int m = std::get<1>(kv.first), B = std::get<2>(kv.first);
        const std::vector<int> &ids = kv.second;
        int k = info[ids[0]].k, kmax = k;
        bool mixed = false;
        for (int id : ids) {
            mixed |= info[id].k != k;
            kmax = std::max(kmax, info[id].k);
        }
        if (framing == 1) {
            if (int rc = encode_bucket_dev(st, groups, info, ids, m, B, k, kmax, mixed)) return rc;
            continue;
        }
        if (mixed) {
            // One var-k launch per chunk. Slot: blocks packed | recovery [gn][m][B] | first[gn + 1]
            const size_t out_g = static_cast<size_t>(m) * B;
            const std::vector<int> start = var_chunks(ids, [&](int id) { return info[id].k; }, B, out_g + 4);
            const int chunks = static_cast<int>(start.size()) - 1;
            size_t max_blocks = 0, max_gn = 0;
            std::vector<std::vector<int>> first(chunks);
            for (int c = 0; c < chunks; ++c) {
                first[c].push_back(0);
                for (int j = start[c]; j < start[c + 1]; ++j) first[c].push_back(first[c].back() + info[ids[j]].k);
                max_blocks = std::max<size_t>(max_blocks, first[c].back());
                max_gn = std::max<size_t>(max_gn, start[c + 1] - start[c]);
            }
            const size_t o_out = (max_blocks * B + 15) & ~size_t(15), o_first = o_out + max_gn * out_g;
            const size_t slot_bytes = o_first + (max_gn + 1) * sizeof(int);
            auto prepare = [&](int c, Slot &s) {
                const int g0 = start[c], gn = start[c + 1] - g0;
                uint8_t *h = static_cast<uint8_t *>(s.h);
                std::memcpy(h + o_first, first[c].data(), (gn + 1) * sizeof(int));
                parallel_for(gn, [&](int j) {
                    const ShorthairTxGroup &g = groups[ids[g0 + j]];
                    uint8_t *blk = h + static_cast<size_t>(first[c][j]) * B;
                    for (int x = 0; x < g.k; ++x, blk += B) {  // EncodeQueued :540-557, as below
                        const int len = g.lens[x];
                        put_u16(blk, len);
                        framing_copy(blk + 2, static_cast<const uint8_t *>(g.packets[x]), len);
                        std::memset(blk + 2 + len, 0, B - 2 - len);
                    }
                    framing_fence();
                });
            };
            auto submit = [&](int c, Slot &s, std::function<void()> &fin) -> int {
                const int g0 = start[c], gn = start[c + 1] - g0, total = first[c].back();
                uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
                SG_CHECK(copy_h2d(d, h, static_cast<size_t>(total) * B, st.stream));
                SG_CHECK(copy_h2d(d + o_first, h + o_first, (gn + 1) * sizeof(int), st.stream));
                const int rc = cauchy_256_encode_batch_var(kmax, m, B, gn, reinterpret_cast<const int *>(d + o_first),
                                                           total, d, d + o_out, st.stream);
                if (rc != 0) return rc;
                count_launch(gn);
                SG_CHECK(copy_d2h(h + o_out, d + o_out, gn * out_g, st.stream));
                fin = [&, g0, gn, h]() {
                    parallel_for(gn, [&](int j) {  // GenerateRecoveryBlock :598-608, as below
                        ShorthairTxGroup &g = groups[ids[g0 + j]];
                        const uint8_t *rec = h + o_out + static_cast<size_t>(j) * out_g;
                        for (int y = 0; y < m; ++y) {
                            uint8_t *p = g.out + static_cast<size_t>(y) * g.out_stride;
                            p[0] = static_cast<uint8_t>(g.k + y);
                            p[1] = static_cast<uint8_t>(g.k - 1);
                            p[2] = static_cast<uint8_t>(m - 1);
                            std::memcpy(p + 3, rec + static_cast<size_t>(y) * B, B);
                        }
                    });
                };
                return 0;
            };
            if (int rc = pipeline(st, chunks, slot_bytes, slot_bytes, prepare, submit)) return rc;
            continue;
        }
        const size_t in_g = static_cast<size_t>(k) * B, out_g = static_cast<size_t>(m) * B;
        const int per = static_cast<int>(std::max<size_t>(1, chunk_bytes() / (in_g + out_g)));
        const int n = static_cast<int>(ids.size());
        const int chunks = (n + per - 1) / per;
        const size_t slot_bytes = static_cast<size_t>(std::min(per, n)) * (in_g + out_g);
        auto prepare = [&](int c, Slot &s) {
            const int g0 = c * per, gn = std::min(per, n - g0);
            uint8_t *h = static_cast<uint8_t *>(s.h);
            // EncodeQueued :540-557: "[len u16 LE][payload][zeros up to B]" per original
            parallel_for(gn, [&](int j) {
                const ShorthairTxGroup &g = groups[ids[g0 + j]];
                uint8_t *blk = h + static_cast<size_t>(j) * in_g;
                for (int x = 0; x < k; ++x, blk += B) {
                    const int len = g.lens[x];
                    put_u16(blk, len);
                    framing_copy(blk + 2, static_cast<const uint8_t *>(g.packets[x]), len);
                    std::memset(blk + 2 + len, 0, B - 2 - len);
                }
                framing_fence();
            });
        };
        auto submit = [&](int c, Slot &s, std::function<void()> &fin) -> int {
            const int g0 = c * per, gn = std::min(per, n - g0);
            uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
            const size_t in_bytes = gn * in_g, out_bytes = gn * out_g;
            SG_CHECK(copy_h2d(d, h, in_bytes, st.stream));
            const int rc = cauchy_256_encode_batch(k, m, B, gn, d, d + in_bytes, st.stream);
            if (rc != 0) return rc;
            count_launch(gn);
            SG_CHECK(copy_d2h(h + in_bytes, d + in_bytes, out_bytes, st.stream));
            fin = [&, g0, gn, h, in_bytes]() {
                // GenerateRecoveryBlock :598-608: "[k+i][k-1][m-1][block i]"
                parallel_for(gn, [&](int j) {
                    ShorthairTxGroup &g = groups[ids[g0 + j]];
                    const uint8_t *rec = h + in_bytes + static_cast<size_t>(j) * out_g;
                    for (int y = 0; y < m; ++y) {
                        uint8_t *p = g.out + static_cast<size_t>(y) * g.out_stride;
                        p[0] = static_cast<uint8_t>(k + y);
                        p[1] = static_cast<uint8_t>(k - 1);
                        p[2] = static_cast<uint8_t>(m - 1);
                        std::memcpy(p + 3, rec + static_cast<size_t>(y) * B, B);
                    }
                });
            };
            return 0;
        };
        if (int rc = pipeline(st, chunks, slot_bytes, slot_bytes, prepare, submit)) return rc;
    }
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

// The delivery-1 tail of a chunk of gn groups (chunk-local group j = ids[g0 + j]) whose decode call has
// been enqueued: d_out [gn][emax][B], d_orow [gn][emax], d_cnt [gn] in device memory; the regions
// start d_base / h_base bytes into the slot. A failure in the finisher lands in *err.
int deliver1_tail(Staging &st, Slot &s, size_t d_base, size_t h_base, int B, int gn, int emax,
                  const uint8_t *d_out, const uint8_t *d_orow, const int *d_cnt,
                  const ShorthairRxGroup *groups, const std::vector<RxInfo> &info, const std::vector<int> &ids,
                  int g0, shorthair_on_packet_fn on_packet, void *cb_ctx, int *err, std::function<void()> &fin) {
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
        if (total < 0 || static_cast<unsigned long long>(total) > L.cap) {
            *err = -2;
            return;
        }
        if (total > 0 && copy_d2h(h + L.h_pay, d, static_cast<size_t>(total), second) != hipSuccess) {
            *err = -2;
            return;
        }
        s.late = [=, &info, &ids]() {
            if (hipStreamSynchronize(second) != hipSuccess) {
                *err = -2;
                return;
            }
            if (!on_packet) return;
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
        };
    };
    return 0;
}

// Device framing, receiver (layout above): originals as payload bytes, the recovery packets' bodies
// as raw blocks.
int recover_bucket_dev(Staging &st, const ShorthairRxGroup *groups, const std::vector<RxInfo> &info,
                       const std::vector<int> &ids, int m, int B, int k, int kmax, bool mixed,
                       shorthair_on_packet_fn on_packet, void *cb_ctx, bool d1, int *d1_err) {
    const int n = static_cast<int>(ids.size());
    const int emax = std::min(mixed ? kmax : k, m);
    const size_t out_g = m >= 2 ? static_cast<size_t>(emax) * B : static_cast<size_t>(B);
    DevChunks ch;
    if (mixed) {
        ch.start = var_chunks(ids, [&](int id) { return info[id].k; }, B, out_g + emax + 8 + 256);
    } else {
        const size_t per_g = static_cast<size_t>(k) * B + k + out_g + emax + 4;
        ch.start = uniform_chunks(n, static_cast<int>(std::max<size_t>(1, chunk_bytes() / per_g)));
    }
    ch.blk0.assign(n + 1, 0);
    ch.pay0.assign(n + 1, 0);
    for (int j = 0; j < n; ++j) {
        const ShorthairRxGroup &g = groups[ids[j]];
        const RxInfo &r = info[ids[j]];
        long long p = static_cast<long long>(r.use) * B;
        for (int i = 0; i < g.n_orig; ++i) p += g.orig_lens[i];
        ch.blk0[j + 1] = ch.blk0[j] + r.k;
        ch.pay0[j + 1] = ch.pay0[j] + p;
    }
    size_t nh = 0, nd = 0;
    for (int c = 0; c < ch.chunks(); ++c) {
        const size_t head = up16(dev_layout(ch.nb(c), ch.gn(c), ch.pay(c), mixed, true).h2d);
        const size_t outs = ch.gn(c) * out_g + static_cast<size_t>(ch.gn(c)) * emax;
        nh = std::max(nh, head + outs);
        nd = std::max(nd, head + static_cast<size_t>(ch.nb(c)) * B + outs + 4 + ch.gn(c) * sizeof(int));
    }
    const size_t h_d1 = up16(nh), d_d1 = up16(nd);  // device delivery: its regions behind the layout above
    if (d1 && m >= 2) {
        size_t max_gn = 0;
        for (int c = 0; c < ch.chunks(); ++c) max_gn = std::max<size_t>(max_gn, ch.gn(c));
        nh = h_d1 + d1_layout(max_gn, emax, B).h_end;
        nd = d_d1 + d1_layout(max_gn, emax, B).d_end;
    }
    auto prepare = [&](int c, Slot &s) {
        const int g0 = ch.g0(c), gn = ch.gn(c);
        const DevLayout L = dev_layout(ch.nb(c), gn, ch.pay(c), mixed, true);
        uint8_t *h = static_cast<uint8_t *>(s.h);
        long long *off = reinterpret_cast<long long *>(h);
        int *len = reinterpret_cast<int *>(h + L.o_len), *first = reinterpret_cast<int *>(h + L.o_first);
        uint8_t *rows = h + L.o_rows, *raw = h + L.o_raw;
        if (mixed)
            for (int j = 0; j <= gn; ++j) first[j] = static_cast<int>(ch.blk0[g0 + j] - ch.blk0[g0]);
        parallel_for(gn, [&](int j) {
            const ShorthairRxGroup &g = groups[ids[g0 + j]];
            const RxInfo &r = info[ids[g0 + j]];
            long long x = ch.blk0[g0 + j] - ch.blk0[g0];
            long long p = ch.pay0[g0 + j] - ch.pay0[g0];
            for (int i = 0; i < g.n_orig; ++i, ++x) {  // RecoverGroup :710-725: the payload only
                const int l = g.orig_lens[i];
                off[x] = p;
                len[x] = l;
                raw[x] = 0;
                rows[x] = g.orig_ids[i];
                framing_copy(h + L.o_pay + p, static_cast<const uint8_t *>(g.orig_data[i]), l);
                p += l;
            }
            for (int i = 0; i < r.use; ++i, ++x) {  // :727-735: the packet's block, verbatim
                off[x] = p;
                len[x] = B;
                raw[x] = 1;
                rows[x] = g.rec_packets[i][0];
                framing_copy(h + L.o_pay + p, g.rec_packets[i] + 3, B);
                p += B;
            }
            framing_fence();
        });
    };
    auto submit = [&](int c, Slot &s, std::function<void()> &fin) -> int {
        const int g0 = ch.g0(c), gn = ch.gn(c), nb = ch.nb(c);
        const DevLayout L = dev_layout(nb, gn, ch.pay(c), mixed, true);
        uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
        const size_t o_blk = up16(L.h2d), o_out = o_blk + static_cast<size_t>(nb) * B;
        const size_t o_orow = o_out + gn * out_g, o_cnt = (o_orow + static_cast<size_t>(gn) * emax + 3) & ~size_t(3);
        const size_t h_out = up16(L.h2d), h_orow = h_out + gn * out_g;
        SG_CHECK(copy_h2d(d, h, L.h2d, st.stream));
        int rc = shorthair_frame_batch(B, nb, d + L.o_pay, static_cast<long long>(ch.pay(c)),
                                       reinterpret_cast<const long long *>(d), reinterpret_cast<const int *>(d + L.o_len),
                                       d + L.o_raw, d + o_blk, st.stream);
        if (rc != 0) return rc;
        if (m >= 2) {
            rc = mixed ? cauchy_256_decode_batch_out_var(kmax, m, B, gn, reinterpret_cast<const int *>(d + L.o_first), nb,
                                                         d + o_blk, d + L.o_rows, d + o_out, d + o_orow,
                                                         reinterpret_cast<int *>(d + o_cnt), st.stream)
                       : cauchy_256_decode_batch_out(k, m, B, gn, d + o_blk, d + L.o_rows, d + o_out, d + o_orow,
                                                     reinterpret_cast<int *>(d + o_cnt), st.stream);
            if (rc != 0) return rc;
            count_launch(gn);
            if (d1)
                return deliver1_tail(st, s, d_d1, h_d1, B, gn, emax, d + o_out, d + o_orow,
                                     reinterpret_cast<const int *>(d + o_cnt), groups, info, ids, g0, on_packet,
                                     cb_ctx, d1_err, fin);
            SG_CHECK(copy_d2h(h + h_out, d + o_out, gn * out_g, st.stream));
            SG_CHECK(copy_d2h(h + h_orow, d + o_orow, gn * static_cast<size_t>(emax), st.stream));
        } else {
            // m == 1 (a uniform bucket): the one erasure lands in place in block k-1 of each group
            rc = cauchy_256_decode_batch(k, m, B, gn, d + o_blk, d + L.o_rows, st.stream);
            if (rc != 0) return rc;
            count_launch(gn);
            SG_CHECK(hipMemcpy2DAsync(h + h_out, B, d + o_blk + static_cast<size_t>(k - 1) * B, static_cast<size_t>(k) * B,
                                      B, gn, hipMemcpyDeviceToHost, st.stream));
            g_d2h.fetch_add(static_cast<long long>(gn) * B, std::memory_order_relaxed);
        }
        if (!on_packet) {
            fin = [] {};
            return 0;
        }
        fin = [&, g0, gn, h, h_out, h_orow, out_g, emax]() {
            for (int j = 0; j < gn; ++j) {  // RecoverGroup :741-756: deliver blocks whose length prefix fits
                const int gi = ids[g0 + j];
                const ShorthairRxGroup &g = groups[gi];
                const int kg = info[gi].k, e = kg - g.n_orig;
                const uint8_t *out = h + h_out + static_cast<size_t>(j) * out_g;
                int missing = -1;
                if (m < 2) {
                    bool seen[256] = {false};
                    for (int i = 0; i < g.n_orig; ++i) seen[g.orig_ids[i]] = true;
                    for (int x = 0; x < kg && missing < 0; ++x)
                        if (!seen[x]) missing = x;
                }
                for (int i = 0; i < e; ++i) {
                    const uint8_t *blk = out + static_cast<size_t>(i) * B;
                    const int id = m >= 2 ? h[h_orow + static_cast<size_t>(j) * emax + i] : missing;
                    const int len = static_cast<int>(get_u16(blk));
                    if (len <= B - 2) on_packet(cb_ctx, gi, id, blk + 2, len);
                }
            }
        };
        return 0;
    };
    return pipeline(st, ch.chunks(), nh, nd, prepare, submit);
}

}  // namespace

extern "C" int shorthair_recover_groups(const ShorthairRxGroup *groups, int count,
                                        shorthair_on_packet_fn on_packet, void *cb_ctx) {
    if (count < 0 || (count > 0 && !groups)) return -1;
    const int framing = g_framing.load(std::memory_order_relaxed);
    const int delivery = g_delivery.load(std::memory_order_relaxed);
    int d1_err = 0;  // a failure in a delivery-1 finisher
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
        const std::vector<int> &ids = kv.second;
        int k = info[ids[0]].k, kmax = k;
        bool mixed = false;
        for (int id : ids) {
            mixed |= info[id].k != k;
            kmax = std::max(kmax, info[id].k);
        }
        if (framing == 1) {
            if (int rc = recover_bucket_dev(st, groups, info, ids, m, B, k, kmax, mixed, on_packet, cb_ctx,
                                            delivery == 1 && m >= 2, &d1_err))
                return rc;
            if (d1_err) return d1_err;
            decoded += static_cast<int>(ids.size());
            continue;
        }
        if (mixed) {  // m >= 2 (bucket key)
            // One var-k launch per chunk. Slot: blocks packed | rows packed | out [gn][emax][B] |
            // out rows [gn][emax] | count [gn] | first[gn + 1]
            const int emax = std::min(kmax, m);
            const size_t out_g = static_cast<size_t>(emax) * B;
            const std::vector<int> start = var_chunks(ids, [&](int id) { return info[id].k; }, B,
                                                      out_g + emax + 8 + 256);
            const int chunks = static_cast<int>(start.size()) - 1;
            size_t max_blocks = 0, max_gn = 0;
            std::vector<std::vector<int>> first(chunks);
            for (int c = 0; c < chunks; ++c) {
                first[c].push_back(0);
                for (int j = start[c]; j < start[c + 1]; ++j) first[c].push_back(first[c].back() + info[ids[j]].k);
                max_blocks = std::max<size_t>(max_blocks, first[c].back());
                max_gn = std::max<size_t>(max_gn, start[c + 1] - start[c]);
            }
            const size_t o_rows = max_blocks * B, o_out = (o_rows + max_blocks + 15) & ~size_t(15);
            const size_t o_orow = o_out + max_gn * out_g, o_cnt = (o_orow + max_gn * emax + 3) & ~size_t(3);
            const size_t o_first = o_cnt + max_gn * sizeof(int);
            const size_t slot_bytes = o_first + (max_gn + 1) * sizeof(int);
            const bool d1 = delivery == 1;
            const size_t base_d1 = up16(slot_bytes);  // device delivery: its regions behind the layout above
            const size_t slot_h = d1 ? base_d1 + d1_layout(max_gn, emax, B).h_end : slot_bytes;
            const size_t slot_d = d1 ? base_d1 + d1_layout(max_gn, emax, B).d_end : slot_bytes;
            auto prepare = [&](int c, Slot &s) {
                const int g0 = start[c], gn = start[c + 1] - g0;
                uint8_t *h = static_cast<uint8_t *>(s.h);
                std::memcpy(h + o_first, first[c].data(), (gn + 1) * sizeof(int));
                parallel_for(gn, [&](int j) {
                    const ShorthairRxGroup &g = groups[ids[g0 + j]];
                    const RxInfo &r = info[ids[g0 + j]];
                    uint8_t *blk = h + static_cast<size_t>(first[c][j]) * B;
                    uint8_t *rows = h + o_rows + first[c][j];
                    int x = 0;
                    for (int i = 0; i < g.n_orig; ++i, ++x, blk += B) {  // RecoverGroup :710-725, as below
                        const int len = g.orig_lens[i];
                        put_u16(blk, len);
                        framing_copy(blk + 2, static_cast<const uint8_t *>(g.orig_data[i]), len);
                        std::memset(blk + 2 + len, 0, B - 2 - len);
                        rows[x] = g.orig_ids[i];
                    }
                    for (int i = 0; i < r.use; ++i, ++x, blk += B) {  // :727-735
                        framing_copy(blk, g.rec_packets[i] + 3, B);
                        rows[x] = g.rec_packets[i][0];
                    }
                    framing_fence();
                });
            };
            auto submit = [&](int c, Slot &s, std::function<void()> &fin) -> int {
                const int g0 = start[c], gn = start[c + 1] - g0, total = first[c].back();
                uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
                SG_CHECK(copy_h2d(d, h, static_cast<size_t>(total) * B, st.stream));
                SG_CHECK(copy_h2d(d + o_rows, h + o_rows, total, st.stream));
                SG_CHECK(copy_h2d(d + o_first, h + o_first, (gn + 1) * sizeof(int), st.stream));
                const int rc = cauchy_256_decode_batch_out_var(kmax, m, B, gn, reinterpret_cast<const int *>(d + o_first),
                                                               total, d, d + o_rows, d + o_out, d + o_orow,
                                                               reinterpret_cast<int *>(d + o_cnt), st.stream);
                if (rc != 0) return rc;
                count_launch(gn);
                if (d1)
                    return deliver1_tail(st, s, base_d1, base_d1, B, gn, emax, d + o_out, d + o_orow,
                                         reinterpret_cast<const int *>(d + o_cnt), groups, info, ids, g0, on_packet,
                                         cb_ctx, &d1_err, fin);
                SG_CHECK(copy_d2h(h + o_out, d + o_out, gn * out_g, st.stream));
                SG_CHECK(copy_d2h(h + o_orow, d + o_orow, gn * static_cast<size_t>(emax), st.stream));
                if (!on_packet) {
                    fin = [] {};
                    return 0;
                }
                fin = [&, g0, gn, h]() {
                    for (int j = 0; j < gn; ++j) {  // RecoverGroup :741-756, as below
                        const int gi = ids[g0 + j];
                        const int e = info[gi].k - groups[gi].n_orig;
                        const uint8_t *out = h + o_out + static_cast<size_t>(j) * out_g;
                        for (int i = 0; i < e; ++i) {
                            const uint8_t *blk = out + static_cast<size_t>(i) * B;
                            const int id = h[o_orow + static_cast<size_t>(j) * emax + i];
                            const int len = static_cast<int>(get_u16(blk));
                            if (len <= B - 2) on_packet(cb_ctx, gi, id, blk + 2, len);
                        }
                    }
                };
                return 0;
            };
            if (int rc = pipeline(st, chunks, slot_h, slot_d, prepare, submit)) return rc;
            if (d1_err) return d1_err;
            decoded += static_cast<int>(ids.size());
            continue;
        }
        const int emax = std::min(k, m);
        // per group: blocks k*B, rows k; out emax*B; out rows emax; count 4 (m >= 2 only)
        const size_t in_g = static_cast<size_t>(k) * B;
        const size_t out_g = m >= 2 ? static_cast<size_t>(emax) * B : static_cast<size_t>(B);
        const size_t per_g = in_g + k + out_g + emax + 4;
        const int per = static_cast<int>(std::max<size_t>(1, chunk_bytes() / per_g));
        const int n = static_cast<int>(ids.size());
        const int chunks = (n + per - 1) / per;
        const int cap = std::min(per, n);
        const size_t slot_bytes = static_cast<size_t>(cap) * per_g + 64;
        // slot layout (chunk of gn groups, offsets for cap groups): blocks | rows | out | out rows | count
        // (device delivery reads d_out in 8-byte words: aligned then, within the 64 bytes of slack)
        const bool d1 = delivery == 1 && m >= 2;
        const size_t o_rows = cap * in_g, o_out = d1 ? up16(o_rows + cap * static_cast<size_t>(k)) : o_rows + cap * static_cast<size_t>(k);
        const size_t o_orow = o_out + cap * out_g, o_cnt = (o_orow + cap * static_cast<size_t>(emax) + 3) & ~size_t(3);
        const size_t base_d1 = up16(slot_bytes);  // device delivery: its regions behind the layout above
        const size_t slot_h = d1 ? base_d1 + d1_layout(cap, emax, B).h_end : slot_bytes;
        const size_t slot_d = d1 ? base_d1 + d1_layout(cap, emax, B).d_end : slot_bytes;
        auto prepare = [&](int c, Slot &s) {
            const int g0 = c * per, gn = std::min(per, n - g0);
            uint8_t *h = static_cast<uint8_t *>(s.h);
            parallel_for(gn, [&](int j) {
                const ShorthairRxGroup &g = groups[ids[g0 + j]];
                const RxInfo &r = info[ids[g0 + j]];
                uint8_t *blk = h + static_cast<size_t>(j) * in_g;
                uint8_t *rows = h + o_rows + static_cast<size_t>(j) * k;
                int x = 0;
                // RecoverGroup :710-725: originals "[len][payload]" zero-padded to B
                for (int i = 0; i < g.n_orig; ++i, ++x, blk += B) {
                    const int len = g.orig_lens[i];
                    put_u16(blk, len);
                    framing_copy(blk + 2, static_cast<const uint8_t *>(g.orig_data[i]), len);
                    std::memset(blk + 2 + len, 0, B - 2 - len);
                    rows[x] = g.orig_ids[i];
                }
                for (int i = 0; i < r.use; ++i, ++x, blk += B) {  // :727-735
                    framing_copy(blk, g.rec_packets[i] + 3, B);
                    rows[x] = g.rec_packets[i][0];
                }
                framing_fence();
            });
        };
        auto submit = [&](int c, Slot &s, std::function<void()> &fin) -> int {
            const int g0 = c * per, gn = std::min(per, n - g0);
            uint8_t *h = static_cast<uint8_t *>(s.h), *d = static_cast<uint8_t *>(s.d);
            SG_CHECK(copy_h2d(d, h, gn * in_g, st.stream));
            SG_CHECK(copy_h2d(d + o_rows, h + o_rows, gn * static_cast<size_t>(k), st.stream));
            if (m >= 2) {
                const int rc = cauchy_256_decode_batch_out(k, m, B, gn, d, d + o_rows, d + o_out, d + o_orow,
                                                           reinterpret_cast<int *>(d + o_cnt), st.stream);
                if (rc != 0) return rc;
                count_launch(gn);
                if (d1)
                    return deliver1_tail(st, s, base_d1, base_d1, B, gn, emax, d + o_out, d + o_orow,
                                         reinterpret_cast<const int *>(d + o_cnt), groups, info, ids, g0, on_packet,
                                         cb_ctx, &d1_err, fin);
                SG_CHECK(copy_d2h(h + o_out, d + o_out, gn * out_g, st.stream));
                SG_CHECK(copy_d2h(h + o_orow, d + o_orow, gn * static_cast<size_t>(emax), st.stream));
            } else {
                // m == 1 (cauchy_decode_m1): the one erasure lands in place in block k-1, the
                // single recovery block (n_orig = k-1 originals precede it)
                const int rc = cauchy_256_decode_batch(k, m, B, gn, d, d + o_rows, st.stream);
                if (rc != 0) return rc;
                count_launch(gn);
                SG_CHECK(hipMemcpy2DAsync(h + o_out, B, d + static_cast<size_t>(k - 1) * B, in_g, B, gn,
                                          hipMemcpyDeviceToHost, st.stream));
                g_d2h.fetch_add(static_cast<long long>(gn) * B, std::memory_order_relaxed);
            }
            if (!on_packet) {  // decode only (no delivery): still wait for the chunk before the
                fin = [] {};   // slot is reused and before the call returns
                return 0;
            }
            fin = [&, g0, gn, h]() {
                // RecoverGroup :741-756: deliver recovered blocks whose length prefix fits
                for (int j = 0; j < gn; ++j) {
                    const int gi = ids[g0 + j];
                    const ShorthairRxGroup &g = groups[gi];
                    const int e = k - g.n_orig;
                    const uint8_t *out = h + o_out + static_cast<size_t>(j) * out_g;
                    int missing = -1;
                    if (m < 2) {
                        bool seen[256] = {false};
                        for (int i = 0; i < g.n_orig; ++i) seen[g.orig_ids[i]] = true;
                        for (int x = 0; x < k && missing < 0; ++x)
                            if (!seen[x]) missing = x;
                    }
                    for (int i = 0; i < e; ++i) {
                        const uint8_t *blk = out + static_cast<size_t>(i) * B;
                        const int id = m >= 2 ? h[o_orow + static_cast<size_t>(j) * emax + i] : missing;
                        const int len = static_cast<int>(get_u16(blk));
                        if (len <= B - 2) on_packet(cb_ctx, gi, id, blk + 2, len);
                    }
                }
            };
            return 0;
        };
        if (int rc = pipeline(st, chunks, slot_h, slot_d, prepare, submit)) return rc;
        if (d1_err) return d1_err;
        decoded += n;
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

extern "C" int shorthair_groups_traffic(long long *h2d_bytes, long long *d2h_bytes) {
    if (h2d_bytes) *h2d_bytes = g_h2d.load(std::memory_order_relaxed);
    if (d2h_bytes) *d2h_bytes = g_d2h.load(std::memory_order_relaxed);
    return 0;
}
