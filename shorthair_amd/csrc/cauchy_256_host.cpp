// Host side of libcauchy256.so: the drop-in cauchy_256.h ABI and the batched device ABI.
//
// Every coding call runs on the GPU. The single-group reference entry points
// (cauchy_256_encode / cauchy_256_decode, reference cauchy_256.cpp:1479 / :1233) gather the
// caller's host blocks into pinned staging, run the batched kernels with groups = 1 and scatter
// the result back; there is deliberately no CPU implementation of the codec in this library.
// Without a usable GPU every call prints an error and returns -2.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <algorithm>
#include <cstring>
#include <array>
#include <atomic>
#include <condition_variable>
#include <memory>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "../../include/cauchy_256.h"
#include "../../include/cauchy_256_batch.h"
#include "cauchy_math.hpp"
#include "colsnip.h"
#include "kernels.hpp"
#include "measure.hpp"
#include "stagea_route.hpp"
#include "stream_call.hpp"

namespace {

#define SH_CHECK(expr)                                                                        \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) {                                                               \
            std::fprintf(stderr, "libcauchy256: %s failed: %s (%s:%d)\n", #expr,             \
                         hipGetErrorString(_e), __FILE__, __LINE__);                          \
            return -2;                                                                        \
        }                                                                                     \
    } while (0)

inline int round4(int x) { return (x + 3) & ~3; }

// Grow-only device buffer. `owner` (if any) is the only stream that uses it: growing waits for
// that stream before freeing the old allocation.
struct DevBuf {
    void *p = nullptr;
    size_t n = 0;
    int ensure(size_t bytes, hipStream_t owner = nullptr) {
        if (bytes <= n) return 0;
        if (p) {
            (void)hipStreamSynchronize(owner);
            (void)hipFree(p);
        }
        p = nullptr;
        n = 0;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            std::fprintf(stderr, "libcauchy256: hipMalloc(%zu) failed\n", bytes);
            return -2;
        }
        n = bytes;
        return 0;
    }
};

struct PinnedBuf {
    void *p = nullptr;
    size_t n = 0;
    int ensure(size_t bytes) {
        if (bytes <= n) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        n = 0;
        if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) {
            std::fprintf(stderr, "libcauchy256: hipHostMalloc(%zu) failed\n", bytes);
            return -2;
        }
        n = bytes;
        return 0;
    }
};

// Per-stream decode state: the workspace and the malformed-group counter of the decodes enqueued
// on that stream. `mu` is held from the workspace lookup until the call's kernels are enqueued, so a
// concurrent grow (another thread on the same stream, or cauchy_256_batch_reserve_stream) can never
// free a buffer that a call is about to use; calls on one stream are then ordered by the stream.
struct StreamState {
    std::mutex mu;
    DevBuf ws;
    int *d_errors = nullptr;
};

// One launch of the tile kernels: output rows [row0, row0 + nrows) with its snippet-address table.
struct TileLaunch {
    int row0, nrows, nsteps;
    long long tstride;
    uint32_t *targets;  // device [parts][tstride]
    bool col;           // column snippets (2 dwords per step) instead of per-row snippets (8)
    uint32_t hi;        // high dword of every snippet address of the launch
};

// Staging of one single-group call (cauchy_256_encode / cauchy_256_decode): pinned host and
// device buffers and its own stream, so calls from different threads -- e.g. two Shorthair codec
// objects -- copy and compute concurrently instead of queueing on one buffer and one stream. The
// reference codec is reentrant per call (cauchy_256.cpp keeps no state beyond its init tables).
struct StageSlot {
    hipStream_t stream = nullptr;
    PinnedBuf h;
    DevBuf d;
};
constexpr size_t kMaxStageSlots = 8;  // concurrent single-group calls; more threads wait for a slot

struct Context {
    std::mutex mu;          // guards lazy state (tables, caches, the stream map, profiling events)
    bool ready = false;
    int device = 0;
    hipStream_t stream = nullptr;
    uint64_t snip_base = 0;           // stage-B snippet table address (code object)
    uint64_t col_base[SH_COL_TUS] = {};  // column-snippet tables (csrc/gen/colsnip_<t>.hip)
    bool col_ok = false;              // ... all inside one 4 GB page (the kernels take low dwords)
    uint64_t *d_rowbytes = nullptr;   // 256 x 8 bytes
    uint8_t *d_exp = nullptr;         // 512
    uint16_t *d_log = nullptr;        // 256
    // (k, m) -> device generator: [m][round4(k)] coefficients (row 0 = ones) for encode,
    // followed by the raw (m-1) x k rows 1..m-1 and the Cauchy parameters X'[k], Y'[m] for
    // decode setup.
    std::map<std::pair<int, int>, uint8_t *> gens;
    // (k, m, dec) -> launches of the runtime-coefficient tile kernels (csrc/tile_snip.hip)
    std::map<std::array<int, 3>, std::vector<TileLaunch>> tiles;
    // Decode state per stream: two decodes in flight on different streams never share scratch.
    std::map<hipStream_t, std::unique_ptr<StreamState>> streams;
    std::atomic<size_t> ws_reserve{0};  // cauchy_256_batch_reserve: minimum size of a workspace
    // stage timing (cauchy_256_profile): per profiled decode, events around setup / stage A /
    // stage B, in a ring of `evq.size()` quadruples (no host synchronisation while recording)
    std::vector<std::array<hipEvent_t, 4>> evq;
    int ev_next = 0, ev_count = 0;
    bool ev_stage_a_only = false;  // cauchy_256_profile(-n): two events per decode, around stage A
    // single-group staging slots (SlotLease): a call holds one for its whole duration
    std::mutex stage_mu;
    std::condition_variable stage_cv;
    std::vector<std::unique_ptr<StageSlot>> stage_all;
    std::vector<StageSlot *> stage_free;
};

Context &ctx() {
    static Context c;
    return c;
}

int init_locked(Context &c, int device) {
    if (c.ready) return 0;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) {
        std::fprintf(stderr, "libcauchy256: no HIP device available; the codec runs only on the GPU\n");
        return -2;
    }
    if (device < 0 || device >= n) device = 0;
    SH_CHECK(hipSetDevice(device));
    SH_CHECK(hipStreamCreateWithFlags(&c.stream, hipStreamNonBlocking));
    const sh::GF256 &f = sh::gf();
    uint64_t rb[256];
    for (int v = 0; v < 256; ++v) {
        uint64_t w = 0;
        for (int b = 0; b < 8; ++b) w |= static_cast<uint64_t>(f.row_bytes[v][b]) << (8 * b);
        rb[v] = w;
    }
    SH_CHECK(hipMalloc(&c.d_rowbytes, sizeof rb));
    SH_CHECK(hipMemcpy(c.d_rowbytes, rb, sizeof rb, hipMemcpyHostToDevice));
    SH_CHECK(hipMalloc(&c.d_exp, 512));
    SH_CHECK(hipMemcpy(c.d_exp, f.exp, 512, hipMemcpyHostToDevice));
    SH_CHECK(hipMalloc(&c.d_log, 512));
    SH_CHECK(hipMemcpy(c.d_log, f.log, 512, hipMemcpyHostToDevice));
    SH_CHECK(sh::stageb_snip_base(&c.snip_base, c.stream));
    SH_CHECK(sh::colsnip_bases(c.col_base, SH_COL_TUS, c.stream));
    {
        // every column-snippet address must share one high dword and have a non-zero low dword
        // (0 means "no call" to the kernels)
        const uint64_t hi0 = c.col_base[0] >> 32;
        bool ok = true;
        for (int t = 0; t < SH_COL_TUS; ++t) {
            const uint64_t n = static_cast<uint64_t>(SH_COL_BLOCKS_PER_TU) * 256 + (t == 0 ? 9 : 0);
            const uint64_t lo = c.col_base[t], hi = lo + n * SH_COL_STRIDE;
            ok = ok && (lo >> 32) == hi0 && (hi >> 32) == hi0 && static_cast<uint32_t>(lo) != 0;
        }
        c.col_ok = ok;
    }
    c.device = device;
    c.ready = true;
    return 0;
}

// Every entry point runs on the library's device, whatever the calling thread had current (HIP's
// current device is per thread; allocations and launches follow it), and gives the thread its
// previous device back when it returns: construct one at the top of each entry point.
struct DeviceScope {
    int rc = 0, prev = -1, dev = -1;
    explicit DeviceScope(Context &c) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        {
            std::lock_guard<std::mutex> g(c.mu);
            rc = init_locked(c, c.device);
        }
        if (rc) return;
        dev = c.device;
        if (prev != dev && hipSetDevice(dev) != hipSuccess) {
            std::fprintf(stderr, "libcauchy256: hipSetDevice(%d) failed\n", dev);
            rc = -2;
        }
    }
    ~DeviceScope() {
        if (prev >= 0 && dev >= 0 && prev != dev) (void)hipSetDevice(prev);
    }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};

// The decode state of `stream` (created on first use, never destroyed: the map owns it).
StreamState *stream_state(Context &c, hipStream_t stream) {
    std::lock_guard<std::mutex> g(c.mu);
    auto &slot = c.streams[stream];
    if (!slot) {
        auto st = std::make_unique<StreamState>();
        if (hipMalloc(&st->d_errors, sizeof(int)) != hipSuccess) return nullptr;
        if (hipMemset(st->d_errors, 0, sizeof(int)) != hipSuccess) {
            (void)hipFree(st->d_errors);
            return nullptr;
        }
        slot = std::move(st);
    }
    return slot.get();
}

// A stream's workspace, locked for one call: at least `bytes` (and the reserve), valid while the
// lease lives. Kernels enqueued under the lease are ordered before any later grow's free by the
// grow's stream synchronisation.
struct WsLease {
    std::unique_lock<std::mutex> lk;
    uint8_t *p = nullptr;
    int *errors = nullptr;
};

// reserve = false: the single-group calls' staging streams, sized by their own need only (up to
// 8 of them; cauchy_256_batch_reserve is for the batched calls' streams).
int lease_workspace(Context &c, hipStream_t stream, size_t bytes, WsLease &out, bool reserve = true) {
    StreamState *st = stream_state(c, stream);
    if (!st) return -2;
    out.lk = std::unique_lock<std::mutex>(st->mu);
    if (st->ws.ensure(reserve ? std::max(bytes, c.ws_reserve.load()) : bytes, stream)) return -2;
    out.p = static_cast<uint8_t *>(st->ws.p);
    out.errors = st->d_errors;
    return 0;
}

// Device generator for (k, m), m >= 2, k + m <= 256. Cached; created once per shape.
uint8_t *generator(Context &c, int k, int m) {
    std::lock_guard<std::mutex> g(c.mu);
    auto it = c.gens.find({k, m});
    if (it != c.gens.end()) return it->second;
    const std::vector<uint8_t> G = sh::generator_matrix(k, m);
    std::vector<uint8_t> xp, yp;
    sh::cauchy_params(k, m, xp, yp);
    const int ld = round4(k);
    const size_t raw = static_cast<size_t>(m) * ld;
    const size_t par = raw + static_cast<size_t>(m - 1) * k;
    std::vector<uint8_t> host(par + k + m, 0);
    for (int y = 0; y < m; ++y) std::memcpy(&host[static_cast<size_t>(y) * ld], &G[static_cast<size_t>(y) * k], k);
    std::memcpy(&host[raw], &G[k], static_cast<size_t>(m - 1) * k);
    std::memcpy(&host[par], xp.data(), k);
    std::memcpy(&host[par + k], yp.data(), m);
    uint8_t *d = nullptr;
    if (hipMalloc(&d, host.size()) != hipSuccess) return nullptr;
    if (hipMemcpy(d, host.data(), host.size(), hipMemcpyHostToDevice) != hipSuccess) return nullptr;
    c.gens[{k, m}] = d;
    return d;
}

// Whether (k, m, B) can run on the runtime-coefficient tile kernels: fixed_geometry's 16-byte
// chunks (B/8 >= 16; tile_shape_ok, the half a host without a GPU answers) and a snippet table
// inside one 4 GB page (the kernels form the snippet addresses from their low dwords).
bool tile_shape_ok(int k, int m, int B) {
    if (k < 2 || m < 2 || k + m > 256 || !sh::tile_ok(B)) return false;
    return !SH_MEASURE_ENV("SH_NO_TILE");  // measurement switch: the older generic kernels
}
bool tile_usable(Context &c, int k, int m, int B) {
    const uint64_t lo = c.snip_base, hi = c.snip_base + static_cast<uint64_t>(sh::SNIP_NULL + 1) * sh::SNIP_STRIDE;
    return tile_shape_ok(k, m, B) && (lo >> 32) == (hi >> 32);
}

// Launch plan of the tile kernels for (k, m): <= 128 rows per launch; per launch and part-wave a
// table of snippet-address low dwords, [step][8] per part (reference generator cauchy_matrix(),
// cauchy_256.cpp:423-481, row 0 = ones). Decode (stage A): steps 0..k-1 are the received columns,
// step k + i adds recovery row row0 + i into its residual row (coefficient 1 on that row only).
const std::vector<TileLaunch> *tile_plan(Context &c, int k, int m, bool dec) {
    std::lock_guard<std::mutex> g(c.mu);
    auto it = c.tiles.find({k, m, dec ? 1 : 0});
    if (it != c.tiles.end()) return &it->second;
    const std::vector<uint8_t> G = sh::generator_matrix(k, m);  // [m][k], row 0 = ones
    const uint32_t base = static_cast<uint32_t>(c.snip_base);
    auto addr = [&](int cf) { return base + static_cast<uint32_t>(cf ? cf : sh::SNIP_NULL) * sh::SNIP_STRIDE; };
    // Decode stage A at m >= 7 runs column snippets (csrc/gen/colsnip_<t>.hip: one call per 4
    // rows, addressed by the input's Cauchy parameter X'_x, as the rows' Y' are the same for every
    // m; no VGPR-index mode): (150,40) 1.231 vs 1.317 ms, (180,76) 2.72 vs 2.82, (120,136) 3.83 vs
    // 4.37, (90,49) 0.98 vs 1.12 against the per-row snippets. Encode keeps the per-row snippets
    // ((180,76) 2.30 vs 2.43 ms; the others within 5 %): a column snippet's table (16 KB per
    // generator row) misses the instruction cache where the 18 KB per-row table stays resident.
    // SH_NO_COL / SH_COL_ENC: measurement switches.
    static const bool no_col = SH_MEASURE_ENV("SH_NO_COL") != nullptr;
    static const bool col_enc = SH_MEASURE_ENV("SH_COL_ENC") != nullptr;
    const bool col = m >= 7 && c.col_ok && !no_col && (dec || col_enc);
    std::vector<uint8_t> xp, yp;
    if (col) sh::cauchy_params(k, m, xp, yp);
    auto col_addr = [&](int blk, int v) {  // block = 4 generator rows
        const int tu = blk / SH_COL_BLOCKS_PER_TU, loc = blk - tu * SH_COL_BLOCKS_PER_TU;
        return static_cast<uint32_t>(c.col_base[tu] + (static_cast<uint64_t>(loc) * 256 + v) * SH_COL_STRIDE);
    };
    std::vector<TileLaunch> plan;
    for (int row0 = 0; row0 < m; row0 += 128) {
        TileLaunch L{};
        L.row0 = row0;
        L.nrows = std::min(128, m - row0);
        L.nsteps = k + (dec ? L.nrows : 0);
        L.col = col;
        L.hi = static_cast<uint32_t>((col ? c.col_base[0] : c.snip_base) >> 32);
        const int parts = sh::tile_parts(L.nrows);
        const int S = sh::tile_steps_per_group(parts);
        const int per = col ? 2 : 8;
        L.tstride = static_cast<long long>((L.nsteps + S - 1) / S) * S * per;
        // + 128 dwords of slack: a step slice's last scalar loads may run up to S - 1 steps past
        // the part's table (into the next part's, or this slack after the last)
        std::vector<uint32_t> t(static_cast<size_t>(parts) * L.tstride + 128, 0u);  // 0: no call
        const int nb4 = (L.nrows + 3) / 4;
        for (int p = 0; p < parts; ++p) {
            if (col) {
                // part p: 4-row blocks [b0, b1) (one or two; tile_snip.hip computes the same)
                const int b0 = p * nb4 / parts, b1 = (p + 1) * nb4 / parts;
                const int yend = std::min(4 * b1, L.nrows);
                for (int x = 0; x < L.nsteps; ++x) {
                    uint32_t *e = &t[static_cast<size_t>(p) * L.tstride + static_cast<size_t>(x) * 2];
                    if (x < k) {
                        for (int i = 0; i < b1 - b0; ++i) e[i] = col_addr(row0 / 4 + b0 + i, xp[x]);
                    } else {
                        const int yy = x - k;  // decode: recovery row yy into its residual row
                        if (yy >= 4 * b0 && yy < yend)
                            e[0] = static_cast<uint32_t>(c.col_base[0] + SH_COL_UNIT((yy - 4 * b0 + 4 * (b0 & 1)) & 7));
                    }
                }
                continue;
            }
            // part p: rows [p * nrows / parts, (p + 1) * nrows / parts) (tile_snip.hip)
            const int y0 = p * L.nrows / parts, y1 = (p + 1) * L.nrows / parts;
            for (int x = 0; x < L.nsteps; ++x) {
                uint32_t *e = &t[static_cast<size_t>(p) * L.tstride + static_cast<size_t>(x) * 8];
                if (x >= k) {  // decode recovery-row step: the unit snippet on its row, no other call
                    const int yy = x - k;
                    if (yy >= y0 && yy < y1) e[yy - y0] = addr(1);
                    continue;
                }
                for (int j = 0; j < y1 - y0; ++j) {  // zero coefficient: no call
                    const int cf = G[static_cast<size_t>(row0 + y0 + j) * k + x];
                    e[j] = cf ? addr(cf) : 0u;
                }
            }
        }
        if (hipMalloc(&L.targets, t.size() * sizeof(uint32_t)) != hipSuccess) return nullptr;
        if (hipMemcpy(L.targets, t.data(), t.size() * sizeof(uint32_t), hipMemcpyHostToDevice) != hipSuccess)
            return nullptr;
        plan.push_back(L);
    }
    return &(c.tiles[{k, m, dec ? 1 : 0}] = std::move(plan));
}

// Batched calls take the caller's stream verbatim (NULL = the null stream, as in HIP itself).
hipStream_t pick(void *stream) { return static_cast<hipStream_t>(stream); }

// A var-k batch (cauchy_256_*_var): group g owns blocks first[g] .. first[g + 1] - 1 of a packed
// array of `total` blocks; `first` is device memory and is never read on the host.
struct VarSpec {
    const int *first = nullptr;
    int total = 0;
};

// What only the single-group ABI (cauchy_256_encode / cauchy_256_decode) asks of the batched
// paths, which get nullptr from the batch ABI. The last four are decode's.
struct SingleGroupOpts {
    // kSliceCap * m * B device bytes that let one group's steps (and stage B's input rows) run as
    // parallel slices (latency); nullptr = the throughput kernels
    uint8_t *slice_scratch = nullptr;
    // pinned host buffer that receives group 0's e_dense recovered rows densely, instead of the
    // device scatter (the caller knows the recovery positions and places them itself)
    uint8_t *h_dense = nullptr;
    int e_dense = 0;
    uint8_t *ws_ext = nullptr;  // the workspace, carved by the caller in its staging buffer (no lease)
    bool host_setup = false;    // ... whose setup fields the host wrote (host_decode_setup): no setup kernel
    // pinned host int that receives group 0's e, copied on the stream while the workspace is still
    // leased to the call (the caller reads it after synchronising)
    int *e_host = nullptr;
};

// Workspace carve for decode of `groups` groups.
struct DecodeWS {
    sh::StageAPlan stage_a;  // stage-A kernels (stagea_route.hpp); .kp: position-table stride (a
                             // compiled K > k codes k, sh::fixed_kernel_k; entries past k stay 0xFF)
    bool full_residual;     // stage A (compile-time or tile kernels) leaves all m residual rows, and
                            // the setup writes position tables instead of stage-A coefficients
    sh::StageBRoute route;  // stage-B kernel (stageb_route.hpp); Snip iff !full_residual
    int emax, ldA, ldB, nres;  // nres: residual rows per group (m when full_residual, else emax)
    int *e;
    uint8_t *rec_idx, *erasures, *coefA, *coefB, *residual, *recovered, *pos, *rpos, *rrow;
    uint64_t *targets;
    long long coefA_gs, coefB_gs;
};

// One pass of encode or of decode stage A over the batch, in the terms every route understands.
struct StageAJob {
    int k, m, B, groups;  // var: k = kmax
    const uint8_t *in;
    long long in_gs;  // 0 with var: the input is the packed block array
    uint8_t *out;
    int n_out;        // output rows per group: m, or emax after a Generic decode stage A
    const DecodeWS *w;   // decode: its position tables (Fixed, Tile) or per-group coefficients (Generic)
    const uint8_t *gen;  // Generic encode: the generator's rows [m][round4(k)], shared by the groups
    const VarSpec *var;
    uint8_t *slice_scratch;  // StageAPlan::sliced: room for the slices' partial outputs
};

// Argument block of the compile-time and the tile kernels (they build their buffer descriptors per
// workgroup, so 32-bit offsets never limit the batch size).
sh::FixedArgs fixed_args(const StageAJob &j) {
    const long long out_gs = static_cast<long long>(j.n_out) * j.B;
    sh::FixedArgs a{};
    a.in = j.in;
    a.in_gstride = j.in_gs;
    a.in_bytes = static_cast<long long>(j.groups) * j.in_gs;
    a.out = j.out;
    a.out_gstride = out_gs;
    a.out_bytes = static_cast<long long>(j.groups) * out_gs;
    a.groups = j.groups;
    a.geo = sh::fixed_geometry(j.B);
    a.pos = j.w ? j.w->pos : nullptr;
    a.rpos = j.w ? j.w->rpos : nullptr;
    if (j.var) {
        a.first = j.var->first;
        a.total_blocks = j.var->total;
        a.in_bytes = static_cast<long long>(j.var->total) * j.B;
    }
    return a;
}

// Argument block of apply_generic: encode shares the generator's rows between the groups (row 0 =
// coefficient 1 everywhere: M(1) is the identity, i.e. plain XOR; column x of the (kmax, m)
// generator is column x of every (k <= kmax, m)), decode has per-group rows and row counts.
sh::ApplyArgs apply_args(Context &c, const StageAJob &j) {
    sh::ApplyArgs a{};
    a.in = j.in;
    a.in_gstride = j.in_gs;
    a.in_bstride = j.B;
    a.n_in = j.k;
    a.out = j.out;
    a.out_gstride = static_cast<long long>(j.n_out) * j.B;
    a.out_bstride = j.B;
    a.n_out = j.n_out;
    a.n_out_g = j.w ? j.w->e : nullptr;
    a.coef = j.w ? j.w->coefA : j.gen;
    a.coef_gstride = j.w ? j.w->coefA_gs : 0;
    a.coef_ld = j.w ? j.w->ldA : round4(j.k);
    a.rowbytes = c.d_rowbytes;
    a.groups = j.groups;
    a.geo = sh::make_geometry(j.B);
    if (j.var) {
        a.first = j.var->first;
        a.total_blocks = j.var->total;
    }
    return a;
}

// Step slices of the single-group latency path: the k (+ m) serial ring steps of one group are
// split over up to 32 workgroups, each XOR-ing its steps' products into a partial output, and the
// partials are XOR-reduced (the products are linear). >= 6 steps per slice.
constexpr int kSliceCap = 32;  // slice_scratch holds this many partial outputs
int latency_slices(int nsteps) {
    // SH_SLICE_MAX / SH_SLICE_STEPS: measurement switches (slices at most, steps per slice at least)
    // (200,32,1400) single-group calls: 8 x 25 steps 80 / 112 us (encode / decode), 16 x 12 74 / 104,
    // 32 x 6 70 / 104 (profiles/r05/ab_runs.txt block 13)
    static const int mx = sh::measure_int(SH_MEASURE_ENV("SH_SLICE_MAX"), 32);
    static const int st = sh::measure_int(SH_MEASURE_ENV("SH_SLICE_STEPS"), 6);
    return std::max(1, std::min(std::min(mx, kSliceCap), nsteps / std::max(st, 1)));
}

// The stage-A plan of (k, m, B) (stagea_route.hpp): the one place the route's inputs are gathered.
// tile: tile_usable(). latency: the call has slice scratch and one group (SingleGroupOpts).
// SH_FORCE_TILE=1 (measurement switch) hides the compile-time kernels, to compare the tile kernels.
sh::StageAPlan stage_a_plan(int k, int m, int B, bool tile, bool dec, bool latency) {
    static const bool force_tile = SH_MEASURE_ENV("SH_FORCE_TILE") != nullptr;
    const int slices = latency ? latency_slices(dec ? k + m : k) : 1;
    return sh::stagea_route(k, force_tile ? 0 : sh::fixed_kernel_k(k, m, B), tile, dec, slices,
                            sh::stagea_span_fits(k, m, B));
}

// One pass of the tile kernels over the batch (encode, or decode stage A with position tables).
// sliced (one group): the steps run as latency_slices() slices whose partial outputs of m * B
// bytes, in j.slice_scratch, are XOR-reduced into j.out.
int launch_tile_batch(Context &c, const StageAJob &j, bool sliced, hipStream_t s) {
    const bool dec = j.w != nullptr;
    const std::vector<TileLaunch> *plan = tile_plan(c, j.k, j.m, dec);
    if (!plan) return -2;
    const sh::FixedArgs f = fixed_args(j);
    for (const TileLaunch &L : *plan) {
        const int parts = sh::tile_parts(L.nrows);
        const int S = sh::tile_steps_per_group(parts);
        const int ns = sliced ? latency_slices(L.nsteps) : 1;
        const long long row0_bytes = static_cast<long long>(L.row0) * j.B;
        sh::TileArgs t{};
        t.f = f;
        t.f.out = j.out + row0_bytes;
        t.f.out_bytes = f.out_bytes - row0_bytes;
        t.targets = L.targets;
        t.tstride = L.tstride;
        t.snip_hi = L.hi;
        t.col = L.col ? 1 : 0;
        t.k = j.k;
        t.m = j.m;
        t.row0 = L.row0;
        t.nrows = L.nrows;
        t.nsteps = L.nsteps;
        if (ns > 1) {
            // slices of a multiple of S steps; partial p at slice_scratch + p * m * B (row r of the
            // launch at + (row0 + r) * B, like the final output)
            const int per = ((L.nsteps + ns - 1) / ns + S - 1) / S * S;
            t.slice_steps = per;
            t.slices = (L.nsteps + per - 1) / per;
            t.out_slice_bytes = f.out_gstride;
            t.f.out = j.slice_scratch + row0_bytes;
            t.f.out_bytes = f.out_gstride - row0_bytes;
        }
        SH_CHECK(sh::launch_tile(t, dec, s));
        if (ns > 1)
            SH_CHECK(sh::launch_xor_reduce(j.slice_scratch + row0_bytes, f.out_gstride, t.slices, j.out + row0_bytes,
                                           static_cast<long long>(L.nrows) * j.B, s));
    }
    return 0;
}

// Encode or decode stage A by the route of its plan.
int launch_stage_a(Context &c, const sh::StageAPlan &plan, const StageAJob &j, hipStream_t s) {
    switch (plan.route) {
    case sh::StageARoute::Fixed:
        SH_CHECK(sh::launch_fixed(j.k, j.m, fixed_args(j), j.w != nullptr, s));
        return 0;
    case sh::StageARoute::Tile:
        return launch_tile_batch(c, j, plan.sliced, s);
    default:  // Generic; decode: per-group rows
        SH_CHECK(sh::launch_apply(apply_args(c, j), j.w != nullptr, s));
        return 0;
    }
}

// ---- batched encode ----
// var (cauchy_256_encode_batch_var; parameters already checked, k = kmax): the same kernels in
// their var-k form, one launch for every k_g <= kmax, after a small launch that counts the
// malformed groups into the stream's error counter.
int encode_batch(int k, int m, int B, int groups, const VarSpec *var, const uint8_t *d_in, uint8_t *d_out,
                 hipStream_t s, const SingleGroupOpts *sg) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    const long long in_gs = var ? 0 : static_cast<long long>(k) * B, out_gs = static_cast<long long>(m) * B;
    if (groups <= 0 || m <= 0 || k <= 0 || B <= 0) return 0;  // (var: only groups can be 0)
    if (var) {
        StreamState *st = stream_state(c, s);
        if (!st) return -2;
        {
            // under the stream's lock, like a decode's count: cauchy_256_batch_errors reads and
            // clears the counter either before this call's count or after it
            std::lock_guard<std::mutex> g(st->mu);
            SH_CHECK(sh::launch_var_check(var->first, var->total, k, groups, st->d_errors, s));
        }
        if (m == 1) {
            SH_CHECK(sh::launch_xor_rows_var(d_in, var->first, var->total, k, d_out, out_gs, B, groups, s));
            return 0;
        }
    } else {
        if (k <= 1) {  // reference cauchy_256.cpp:1485-1493
            SH_CHECK(sh::launch_copy_first(d_in, in_gs, d_out, out_gs, m, B, groups, s));
            return 0;
        }
        const bool valid = (k + m <= 256) && (B % 8 == 0);
        if (m == 1 || !valid) {
            // Row 0 (plain XOR, any B) is written even when the parameters are then rejected
            // (reference cauchy_256.cpp:1496-1511).
            SH_CHECK(sh::launch_xor_rows(d_in, in_gs, k, d_out, out_gs, B, groups, s));
            return (m == 1 || valid) ? 0 : -1;  // m == 1 returns before validation (:1503-1506)
        }
    }
    StageAJob j{k, m, B, groups, d_in, in_gs, d_out, /*n_out=*/m};
    j.var = var;
    j.slice_scratch = sg ? sg->slice_scratch : nullptr;
    const bool latency = j.slice_scratch && groups == 1;
    const sh::StageAPlan plan = stage_a_plan(k, m, B, tile_usable(c, k, m, B), /*dec=*/false, latency);
    if (plan.route == sh::StageARoute::Generic && !(j.gen = generator(c, k, m))) return -2;
    return launch_stage_a(c, plan, j, s);
}

// latency: the decode has slice scratch and one group (stage_a_plan; the layout does not depend on it).
size_t carve(DecodeWS &w, uint8_t *base, int k, int m, int B, int groups, bool need_recovered, bool latency) {
    const sh::Geometry geo = sh::fixed_geometry(B);
    w.emax = std::min(k, m);
    w.stage_a = stage_a_plan(k, m, B, tile_usable(ctx(), k, m, B), /*dec=*/true, latency);
    // stage A over all m rows (compile-time or tile kernels) and position tables, where the
    // geometry lets a residual stage-B kernel follow
    w.route = sh::stageb_route(geo, w.emax, w.stage_a.route != sh::StageARoute::Generic);
    w.full_residual = w.route != sh::StageBRoute::Snip;
    const bool regs = w.route == sh::StageBRoute::Regs;
    w.ldA = w.full_residual ? 0 : round4(k);
    w.ldB = (w.emax + 7) & ~7;  // stage-B coefficients [i][ldB] (transposed, 8-entry rows)
    w.nres = w.full_residual ? m : w.emax;
    w.coefA_gs = static_cast<long long>(w.emax) * w.ldA;
    w.coefB_gs = static_cast<long long>(w.emax) * w.ldB;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        uint8_t *p = base ? base + off : nullptr;
        off += (bytes + 255) & ~static_cast<size_t>(255);
        return p;
    };
    const size_t G = static_cast<size_t>(groups);
    w.e = reinterpret_cast<int *>(take(G * sizeof(int)));
    w.rec_idx = take(G * w.emax);
    w.erasures = take(G * w.emax);
    w.coefA = w.full_residual ? nullptr : take(G * w.coefA_gs);
    // stage-B coefficients: snippet addresses for stageb_regs, bytes for every other kernel
    w.coefB = regs ? nullptr : take(G * w.coefB_gs);
    w.targets = regs ? reinterpret_cast<uint64_t *>(take(G * w.emax * w.ldB * sizeof(uint64_t))) : nullptr;
    w.rrow = w.full_residual ? take(G * round4(w.emax)) : nullptr;
    w.pos = w.full_residual ? take(G * w.stage_a.kp) : nullptr;
    w.rpos = w.full_residual ? take(G * round4(m)) : nullptr;
    w.residual = take(G * w.nres * static_cast<size_t>(B) + 256);  // + slack: word over-read
    w.recovered = need_recovered ? take(G * w.emax * static_cast<size_t>(B)) : nullptr;
    return off;
}

// Rows per stage-B slice on the single-group latency path (SH_SB_SLICE, measurement switch; 0 = one
// workgroup streams all e rows).
int stageb_row_slice() {
    static const int n = sh::measure_int(SH_MEASURE_ENV("SH_SB_SLICE"), 8);
    return std::max(0, n);
}

// slice_scratch (groups == 1, stageb_v2 only): the e input rows are split into slices of
// stageb_row_slice() rows, one workgroup each, whose partial outputs are XOR-reduced into dst.
hipError_t launch_stage_b(const DecodeWS &w, int n_in, int B, int groups, uint8_t *dst, hipStream_t s,
                          uint8_t *slice_scratch = nullptr) {
    if (w.route == sh::StageBRoute::Snip) {
        sh::StageBArgs b{};
        b.in = w.residual;
        b.in_gstride = static_cast<long long>(n_in) * B;
        b.n_in = n_in;
        b.out = dst;
        b.out_gstride = static_cast<long long>(w.emax) * B;
        b.e = w.e;
        b.coefT = w.coefB;
        b.coefT_gstride = w.coefB_gs;
        b.ldT = w.ldB;
        b.groups = groups;
        b.geo = sh::make_geometry(B);
        return sh::launch_stageb(b, w.emax, s);
    }
    sh::StageBResidualArgs f{};
    f.in = w.residual;
    f.in_gstride = static_cast<long long>(n_in) * B;
    f.out = dst;
    f.out_gstride = static_cast<long long>(w.emax) * B;
    f.e = w.e;
    f.rrow = w.rrow;
    f.ldR = round4(w.emax);
    f.coefT = w.coefB;
    f.coefT_gstride = w.coefB_gs;
    f.ldT = w.ldB;
    f.emax = w.emax;
    f.groups = groups;
    f.geo = sh::fixed_geometry(B);
    f.snip_base = ctx().snip_base;
    f.targets = w.targets;
    switch (w.route) {
    case sh::StageBRoute::Small:
        return sh::launch_stageb_small(f, s);
    case sh::StageBRoute::Regs:
        return sh::launch_stageb_regs(f, s);
    default: {  // V2
        // at most kSliceCap partial outputs fit slice_scratch (a small measurement
        // setting of SH_SB_SLICE must not write past it)
        const int rs0 = stageb_row_slice();
        const int rs = rs0 > 0 ? std::max(rs0, (w.emax + kSliceCap - 1) / kSliceCap) : 0;
        if (slice_scratch && groups == 1 && rs > 0 && w.emax > rs) {
            f.row_slice = rs;
            f.row_slices = (w.emax + rs - 1) / rs;
            f.out_slice_bytes = f.out_gstride;
            f.out = slice_scratch;
            if (hipError_t r = sh::launch_stageb_v2(f, s)) return r;
            return sh::launch_xor_reduce(slice_scratch, f.out_gstride, f.row_slices, dst, f.out_gstride, s);
        }
        return sh::launch_stageb_v2(f, s);
    }
    }
}

// Common decode core (m >= 2, valid params): writes recovered blocks densely into `dst`
// ([G][emax][B]) and leaves per-group e / rec_idx / erasures in the workspace.
int decode_core(Context &c, int k, int m, int B, int groups, const uint8_t *d_blocks,
                const uint8_t *d_rows, DecodeWS &w, int *errors, uint8_t *dst, hipStream_t s,
                const VarSpec *var, const SingleGroupOpts *sg) {
    uint8_t *slice_scratch = sg ? sg->slice_scratch : nullptr;
    uint8_t *gen = generator(c, k, m);
    if (!gen) return -2;
    sh::DecodeSetupArgs sa{};
    sa.k = k;
    sa.m = m;
    sa.rows = d_rows;
    sa.rows_gstride = k;
    sa.gen = gen + static_cast<size_t>(m) * round4(k);
    sa.xp = sa.gen + static_cast<size_t>(m - 1) * k;
    sa.yp = sa.xp + k;
    sa.gf_exp = c.d_exp;
    sa.gf_log = c.d_log;
    sa.emax = w.emax;
    sa.e_out = w.e;
    sa.rec_idx = w.rec_idx;
    sa.erasures = w.erasures;
    sa.coefA = w.coefA;
    sa.coefA_gstride = w.coefA_gs;
    sa.ldA = w.ldA;
    sa.coefB = w.coefB;
    sa.coefB_gstride = w.coefB_gs;
    sa.ldB = w.ldB;
    sa.pos = w.pos;
    sa.kp = w.stage_a.kp;
    sa.rpos = w.rpos;
    sa.rrow = w.rrow;
    sa.ldR = round4(w.emax);
    sa.targets = w.targets;
    sa.snip_base = c.snip_base;
    sa.errors = errors;
    if (var) {  // k = kmax: the generator rows and X' are kmax wide, every group has its own k_g
        sa.first = var->first;
        sa.total_blocks = var->total;
    }
    hipEvent_t *ev = nullptr;
    {  // check and claim the slot in one critical section (profile() may resize the ring)
        std::lock_guard<std::mutex> g(c.mu);
        if (!c.evq.empty()) {
            ev = c.evq[c.ev_next].data();
            c.ev_next = (c.ev_next + 1) % static_cast<int>(c.evq.size());
            c.ev_count = std::min(c.ev_count + 1, static_cast<int>(c.evq.size()));
        }
    }
    // stage-A-only profiling records ev[1] and ev[2] alone (fewer event packets in a timed loop)
    bool ev_all = false;
    if (ev) {
        std::lock_guard<std::mutex> g(c.mu);
        ev_all = !c.ev_stage_a_only;
    }
    if (ev && ev_all) SH_CHECK(hipEventRecord(ev[0], s));
    if (!(sg && sg->host_setup)) SH_CHECK(sh::launch_decode_setup(sa, groups, s));
    if (ev) SH_CHECK(hipEventRecord(ev[1], s));

    // Stage A. Fixed, Tile (compile-time generator, all m rows, erased columns read as zeros):
    //   residual_y = R_y + sum_{received x} M(C[y][x]) d_x
    // Generic (per-group coefficients, the emax rows of the received recovery blocks):
    //   residual_i = R_i + sum_{orig j} M(C[r_i][row_j]) d_j
    StageAJob j{k, m, B, groups, d_blocks, static_cast<long long>(k) * B, w.residual, /*n_out=*/w.nres, &w};
    j.var = var;
    j.slice_scratch = slice_scratch;
    if (int rc = launch_stage_a(c, w.stage_a, j, s)) return rc;
    // (the events past the setup are recorded after a full-residual stage A only)
    if (ev && w.full_residual) SH_CHECK(hipEventRecord(ev[2], s));
    // Stage B: recovered_j = sum_i M(S^-1[j][i]) (residual of the i-th received recovery block)
    SH_CHECK(launch_stage_b(w, w.nres, B, groups, dst, s, groups == 1 ? slice_scratch : nullptr));
    if (ev && ev_all && w.full_residual) SH_CHECK(hipEventRecord(ev[3], s));
    return 0;
}

int invalid_decode_status(int k, int groups, const uint8_t *d_rows, hipStream_t s) {
    std::vector<uint8_t> rows(static_cast<size_t>(groups) * k);
    SH_CHECK(hipMemcpyAsync(rows.data(), d_rows, rows.size(), hipMemcpyDeviceToHost, s));
    SH_CHECK(hipStreamSynchronize(s));
    for (uint8_t r : rows)
        if (r >= k) return -1;
    return 0;
}

// Host restatement of decode_setup (kernels.hip) for one group, written into a host image of the
// workspace carved exactly as the device's (carve()): the single-group ABI uploads it with the
// blocks, so its decode runs no setup kernel. Covers the modes whose stage B takes byte
// coefficients (stageb_v2, stageb_small) after a full-residual stage A, for m >= 7 (closed-form
// Cauchy inverse, kernels.hip decode_setup: S^-1[j][i] = a_j b_i / (x_j (x_j + y_i))); returns
// false (device setup) otherwise. rec[i]: array index of the i-th recovery block, era[j]: j-th
// erased original row (sort_blocks order, cauchy_256.cpp:522-554), 0 < e <= number of erasures.
bool host_decode_setup(const DecodeWS &w, int k, int m, const uint8_t *rows, int e, const int *rec,
                       const int *era) {
    if (!(w.route == sh::StageBRoute::V2 || w.route == sh::StageBRoute::Small) || m < 7 || !w.coefB || !w.rrow || !w.pos || !w.rpos) return false;
    const sh::GF256 &f = sh::gf();
    std::vector<uint8_t> xp, yp;
    sh::cauchy_params(k, m, xp, yp);
    *w.e = e;
    std::memset(w.rrow, 0, round4(w.emax));
    std::memset(w.pos, 0xFF, w.stage_a.kp);
    std::memset(w.rpos, 0xFF, round4(m));
    for (int j = 0; j < k; ++j) {
        if (rows[j] < k) w.pos[rows[j]] = static_cast<uint8_t>(j);
        else w.rpos[rows[j] - k] = static_cast<uint8_t>(j);
    }
    int x[256], y[256], la[256], lb[256];
    for (int t = 0; t < e; ++t) {
        w.rec_idx[t] = static_cast<uint8_t>(rec[t]);
        w.erasures[t] = static_cast<uint8_t>(era[t]);
        w.rrow[t] = static_cast<uint8_t>(rows[rec[t]] - k);
        x[t] = xp[era[t]];
        y[t] = yp[rows[rec[t]] - k];
    }
    auto mod255 = [](int v) { v %= 255; return v < 0 ? v + 255 : v; };
    for (int t = 0; t < e; ++t) {
        int a = 0, b = 0;
        for (int q = 0; q < e; ++q) {
            a += f.log[x[t] ^ y[q]];
            b += f.log[x[q] ^ y[t]];
            if (q != t) {
                a -= f.log[x[t] ^ x[q]];
                b -= f.log[y[t] ^ y[q]];
            }
        }
        la[t] = mod255(a - f.log[x[t]]);
        lb[t] = mod255(b);
    }
    std::memset(w.coefB, 0, static_cast<size_t>(w.emax) * w.ldB);  // [i][j] = S^-1[j][i], zero past e
    for (int i = 0; i < e; ++i)
        for (int j = 0; j < e; ++j)
            w.coefB[static_cast<size_t>(i) * w.ldB + j] = f.exp[mod255(la[j] + lb[i] - f.log[x[j] ^ y[i]])];
    return true;
}

int decode_batch(int k, int m, int B, int groups, uint8_t *d_blocks, uint8_t *d_rows, hipStream_t s,
                 const SingleGroupOpts *sg) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    if (groups <= 0 || k <= 0) return 0;
    if (k <= 1) {  // cauchy_256.cpp:1236-1240
        SH_CHECK(sh::launch_decode_k1(d_rows, k, groups, s));
        return 0;
    }
    if (m == 1) {  // cauchy_256.cpp:1243-1246 (no parameter check on this path)
        SH_CHECK(sh::launch_decode_m1(d_blocks, static_cast<long long>(k) * B, d_rows, k, k, B, groups, s));
        return 0;
    }
    if (k + m > 256 || B % 8 != 0) return invalid_decode_status(k, groups, d_rows, s);
    const SingleGroupOpts none, &o = sg ? *sg : none;
    const bool latency = o.slice_scratch && groups == 1;
    DecodeWS w{};
    WsLease ls;
    if (!o.ws_ext) {
        // slice_scratch: the single-group ABI (a staging stream, no batch reserve)
        const size_t need = carve(w, nullptr, k, m, B, groups, true, latency);
        if (int rc = lease_workspace(c, s, need, ls, o.slice_scratch == nullptr)) return rc;
    }
    carve(w, o.ws_ext ? o.ws_ext : ls.p, k, m, B, groups, true, latency);
    if (int rc = decode_core(c, k, m, B, groups, d_blocks, d_rows, w, o.ws_ext ? nullptr : ls.errors, w.recovered, s,
                             nullptr, sg))
        return rc;
    if (o.h_dense) {  // still under the workspace lease: the copy is ordered before any regrowth
        SH_CHECK(hipMemcpyAsync(o.h_dense, w.recovered, static_cast<size_t>(o.e_dense) * B, hipMemcpyDeviceToHost, s));
        return 0;
    }
    sh::ScatterArgs sc{};
    sc.src = w.recovered;
    sc.src_gstride = static_cast<long long>(w.emax) * B;
    sc.blocks = d_blocks;
    sc.blocks_gstride = static_cast<long long>(k) * B;
    sc.rows = d_rows;
    sc.rows_gstride = k;
    sc.e = w.e;
    sc.rec_idx = w.rec_idx;
    sc.erasures = w.erasures;
    sc.emax = w.emax;
    sc.B = B;
    SH_CHECK(sh::launch_scatter(sc, groups, s));
    if (o.e_host) SH_CHECK(hipMemcpyAsync(o.e_host, w.e, sizeof(int), hipMemcpyDeviceToHost, s));
    return 0;
}

}  // namespace

// csrc/stream_call.hpp. (Held's members leave in reverse order: the lock first, then the device.)
struct sh::StreamCall::Held {
    DeviceScope ds;
    std::unique_lock<std::mutex> lk;
    explicit Held(Context &c) : ds(c) {}
};

sh::StreamCall::StreamCall(void *stream_, bool counts) : stream(pick(stream_)) {
    Context &c = ctx();
    held_ = std::make_unique<Held>(c);
    rc = held_->ds.rc;
    if (rc || !counts) return;
    StreamState *st = stream_state(c, stream);
    if (!st) {
        rc = -2;
        return;
    }
    held_->lk = std::unique_lock<std::mutex>(st->mu);
    errors = st->d_errors;
}

sh::StreamCall::~StreamCall() = default;

// =============================================================================================
// Batched device ABI (cauchy_256_batch.h)
// =============================================================================================
extern "C" int cauchy_256_batch_init(int device) {
    Context &c = ctx();
    std::lock_guard<std::mutex> g(c.mu);
    return init_locked(c, device);
}

extern "C" int cauchy_256_encode_batch(int k, int m, int block_bytes, int groups,
                                       const void *d_data, void *d_recovery, void *stream) {
    return encode_batch(k, m, block_bytes, groups, nullptr, static_cast<const uint8_t *>(d_data),
                        static_cast<uint8_t *>(d_recovery), pick(stream), nullptr);
}

extern "C" int cauchy_256_decode_batch(int k, int m, int block_bytes, int groups, void *d_blocks,
                                       unsigned char *d_rows, void *stream) {
    return decode_batch(k, m, block_bytes, groups, static_cast<uint8_t *>(d_blocks), d_rows, pick(stream), nullptr);
}

namespace {
// cauchy_256_decode_batch_out(_var) after their parameter checks (k, m >= 2, k + m <= 256,
// B % 8 == 0, groups > 0). var: k = kmax, and the workspace is the uniform (kmax, m) decode's, so
// cauchy_256_batch_reserve(kmax, ...) covers it.
int decode_batch_out(Context &c, int k, int m, int B, int groups, const VarSpec *var, const void *d_blocks,
                     const unsigned char *d_rows, void *d_out, unsigned char *d_out_rows, int *d_out_count,
                     hipStream_t s) {
    DecodeWS w{};
    WsLease ls;
    const bool need_recovered = false, latency = false;  // straight into d_out; the throughput kernels
    if (int rc = lease_workspace(c, s, carve(w, nullptr, k, m, B, groups, need_recovered, latency), ls)) return rc;
    carve(w, ls.p, k, m, B, groups, need_recovered, latency);
    // the setup writes the erasure list ([G][emax]) and the counts ([G]) straight into the
    // caller's outputs (same layouts as the workspace's): no copies after the decode
    w.erasures = d_out_rows;
    w.e = d_out_count;
    return decode_core(c, k, m, B, groups, static_cast<const uint8_t *>(d_blocks), d_rows, w, ls.errors,
                       static_cast<uint8_t *>(d_out), s, var, nullptr);
}

// Host-checked parameters of the var-k calls (cauchy_256_batch.h): false = -1, nothing enqueued.
bool var_params_ok(int kmax, int m, int mmin, int B, int groups, int total_blocks) {
    return kmax >= 2 && kmax <= 255 && m >= mmin && kmax + m <= 256 && B > 0 && B % 8 == 0 && groups >= 0 &&
           total_blocks >= 0 && static_cast<long long>(total_blocks) <= static_cast<long long>(groups) * kmax;
}
}  // namespace

extern "C" int cauchy_256_decode_batch_out(int k, int m, int block_bytes, int groups, const void *d_blocks,
                                           const unsigned char *d_rows, void *d_out, unsigned char *d_out_rows,
                                           int *d_out_count, void *stream) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    if (groups <= 0) return 0;
    if (k < 2 || m < 2) return -1;
    hipStream_t s = pick(stream);
    if (k + m > 256 || block_bytes % 8 != 0) return invalid_decode_status(k, groups, d_rows, s);
    return decode_batch_out(c, k, m, block_bytes, groups, nullptr, d_blocks, d_rows, d_out, d_out_rows, d_out_count, s);
}

extern "C" int cauchy_256_encode_batch_var(int kmax, int m, int block_bytes, int groups, const int *d_first,
                                           int total_blocks, const void *d_data, void *d_recovery,
                                           void *stream) {
    if (!var_params_ok(kmax, m, 1, block_bytes, groups, total_blocks)) return -1;
    const VarSpec var{d_first, total_blocks};
    return encode_batch(kmax, m, block_bytes, groups, &var, static_cast<const uint8_t *>(d_data),
                        static_cast<uint8_t *>(d_recovery), pick(stream), nullptr);
}

extern "C" int cauchy_256_decode_batch_out_var(int kmax, int m, int block_bytes, int groups, const int *d_first,
                                               int total_blocks, const void *d_blocks,
                                               const unsigned char *d_rows, void *d_out,
                                               unsigned char *d_out_rows, int *d_out_count, void *stream) {
    if (!var_params_ok(kmax, m, 2, block_bytes, groups, total_blocks)) return -1;
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    if (groups <= 0) return 0;
    const VarSpec var{d_first, total_blocks};
    return decode_batch_out(c, kmax, m, block_bytes, groups, &var, d_blocks, d_rows, d_out, d_out_rows, d_out_count,
                            pick(stream));
}

extern "C" int cauchy_256_batch_reserve(int k, int m, int block_bytes, int groups) {
    return cauchy_256_batch_reserve_stream(k, m, block_bytes, groups, nullptr);
}

extern "C" int cauchy_256_batch_reserve_stream(int k, int m, int block_bytes, int groups, void *stream) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    if (k < 2 || m < 2 || k + m > 256 || block_bytes <= 0 || groups <= 0) return 0;
    DecodeWS w{};
    const size_t need = carve(w, nullptr, k, m, block_bytes, groups, /*need_recovered=*/true, /*latency=*/false);
    if (!generator(c, k, m)) return -2;
    // the tile kernels' snippet-address tables of this shape, so a later decode allocates nothing
    if (w.stage_a.route == sh::StageARoute::Tile && !tile_plan(c, k, m, true)) return -2;
    size_t cur = c.ws_reserve.load();
    while (cur < need && !c.ws_reserve.compare_exchange_weak(cur, need)) {
    }
    WsLease ls;
    return lease_workspace(c, pick(stream), need, ls);
}

extern "C" int cauchy_256_batch_errors(void *stream) {
    // Read and clear in stream order, under the stream's lock: a decode enqueued on this stream
    // (by any thread) lands either before the read or after the clear, never in between.
    sh::StreamCall call(stream);
    if (call.rc) return call.rc;
    int *n = nullptr;
    SH_CHECK(hipHostMalloc(reinterpret_cast<void **>(&n), sizeof(int), hipHostMallocDefault));
    *n = 0;
    hipError_t e = hipMemcpyAsync(n, call.errors, sizeof(int), hipMemcpyDeviceToHost, call.stream);
    if (e == hipSuccess) e = hipMemsetAsync(call.errors, 0, sizeof(int), call.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(call.stream);
    const int r = *n;
    (void)hipHostFree(n);
    if (e != hipSuccess) {
        std::fprintf(stderr, "libcauchy256: batch_errors failed: %s\n", hipGetErrorString(e));
        return -2;
    }
    return r;
}

extern "C" int cauchy_256_fill_synthetic(void *d_out, int n, int block_bytes, int groups,
                                         unsigned long long g0, unsigned long long cfg,
                                         void *stream) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    SH_CHECK(sh::launch_fill(static_cast<uint8_t *>(d_out), static_cast<long long>(n) * block_bytes,
                             n, block_bytes, groups, g0, cfg, pick(stream)));
    return 0;
}

// Synthetic erasure pattern of group g (host integers, no GPU): the same PCG32 stream and
// partial Fisher-Yates picks as the test oracle's generator (oracle/cauchy_oracle.c), so the
// benchmark's decode inputs match the parity tests'. Survivors ascending, then the chosen
// recovery rows (k + y) ascending; returns the erasure count e.
extern "C" int cauchy_256_erasure_pattern(unsigned long long g, int k, int m, unsigned long long cfg,
                                          int e_fixed, unsigned char *rows_out) {
    if (k <= 0 || m <= 0 || k + m > 256 || !rows_out) return -1;
    const uint64_t inc = (static_cast<uint64_t>(g) << 1) | 1ull;
    uint64_t state = 0;
    auto next = [&]() {
        const uint64_t old = state;
        state = old * 6364136223846793005ull + inc;
        const uint32_t xs = static_cast<uint32_t>(((old >> 18) ^ old) >> 27);
        const uint32_t rot = static_cast<uint32_t>(old >> 59);
        return (xs >> rot) | (xs << ((32u - rot) & 31u));
    };
    next();
    state += cfg ^ 0xE7A5ull;
    next();
    const int emax = std::min(k, m);
    const int e = e_fixed > 0 ? std::min(e_fixed, emax) : 1 + static_cast<int>(next() % static_cast<uint32_t>(emax));
    uint8_t pk[256], pm[256];
    bool lost[256] = {}, used[256] = {};
    for (int i = 0; i < k; ++i) pk[i] = static_cast<uint8_t>(i);
    for (int i = 0; i < m; ++i) pm[i] = static_cast<uint8_t>(i);
    for (int i = 0; i < e; ++i) {
        std::swap(pk[i], pk[i + static_cast<int>(next() % static_cast<uint32_t>(k - i))]);
        std::swap(pm[i], pm[i + static_cast<int>(next() % static_cast<uint32_t>(m - i))]);
        lost[pk[i]] = true;
        used[pm[i]] = true;
    }
    int n = 0;
    for (int x = 0; x < k; ++x)
        if (!lost[x]) rows_out[n++] = static_cast<uint8_t>(x);
    for (int y = 0; y < m; ++y)
        if (used[y]) rows_out[n++] = static_cast<uint8_t>(k + y);
    return e;
}

extern "C" int cauchy_256_batch_path(int k, int m, int block_bytes) {
    if (k < 1 || m < 1 || k + m > 256 || block_bytes <= 0 || block_bytes % 8 != 0) return -1;
    // Host-only answer (a launcher may ask before it spawns rank processes, so this never
    // initialises the GPU): the snippet table's one-4-GB-page condition needs the loaded code
    // object and is checked at launch (generic kernels otherwise); once the library is
    // initialised the answer includes it.
    Context &c = ctx();
    std::lock_guard<std::mutex> g(c.mu);
    const bool tile = c.ready ? tile_usable(c, k, m, block_bytes) : tile_shape_ok(k, m, block_bytes);
    const sh::StageARoute r = stage_a_plan(k, m, block_bytes, tile, /*dec=*/false, /*latency=*/false).route;
    return r == sh::StageARoute::Fixed ? 1 : r == sh::StageARoute::Tile ? 2 : 0;
}

extern "C" void *cauchy_256_default_stream(void) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return nullptr;
    return c.stream;
}

extern "C" int cauchy_256_profile(int capacity) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    std::lock_guard<std::mutex> g(c.mu);
    for (auto &q : c.evq)
        for (hipEvent_t e : q) (void)hipEventDestroy(e);
    c.ev_stage_a_only = capacity < 0;
    if (capacity < 0) capacity = -capacity;
    c.evq.assign(std::max(0, capacity), {});
    for (auto &q : c.evq)
        for (hipEvent_t &e : q) SH_CHECK(hipEventCreate(&e));
    c.ev_next = c.ev_count = 0;
    return 0;
}

extern "C" int cauchy_256_profile_read(float *ms) {
    Context &c = ctx();
    std::lock_guard<std::mutex> g(c.mu);
    if (c.ev_count == 0) return -1;
    double sum[3] = {0, 0, 0};
    const bool a_only = c.ev_stage_a_only;
    for (int i = 0; i < c.ev_count; ++i) {
        const auto &q = c.evq[i];
        SH_CHECK(hipEventSynchronize(q[a_only ? 2 : 3]));
        for (int t = a_only ? 1 : 0; t < (a_only ? 2 : 3); ++t) {
            float x = 0;
            SH_CHECK(hipEventElapsedTime(&x, q[t], q[t + 1]));
            sum[t] += x;
        }
    }
    for (int t = 0; t < 3; ++t) ms[t] = (a_only && t != 1) ? -1.0f : static_cast<float>(sum[t] / c.ev_count);
    return c.ev_count;
}

extern "C" int cauchy_256_sync(void *stream) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    SH_CHECK(hipStreamSynchronize(pick(stream)));
    return 0;
}

// =============================================================================================
// Drop-in single-group ABI (cauchy_256.h). One group per call through a pinned staging slot with
// its own stream (SlotLease): concurrent calls from different threads overlap on the GPU.
// =============================================================================================
// The reference's exported product/quotient tables (cauchy_256.cpp:346-347, built by GFC256Init
// :349-386 on the first _cauchy_256_init): 256 x 256 bytes each, entry (y << 8) + x = x * y and
// x / y in GF(256)/0x187, zero rows and columns for 0. Exported for symbol parity with
// cauchy_256.o; the codec itself does not read them. Null until the first successful version check.
extern "C" {
__attribute__((visibility("default"))) uint8_t *GFC256_MUL_TABLE = nullptr;
__attribute__((visibility("default"))) uint8_t *GFC256_DIV_TABLE = nullptr;
}

namespace {
void export_field_tables() {
    static std::once_flag once;
    std::call_once(once, [] {
        static uint8_t tab[2][256 * 256];
        const sh::GF256 &f = sh::gf();
        for (int y = 0; y < 256; ++y)
            for (int x = 0; x < 256; ++x) {
                tab[0][(y << 8) + x] = f.mul(static_cast<uint8_t>(x), static_cast<uint8_t>(y));
                tab[1][(y << 8) + x] = f.div(static_cast<uint8_t>(x), static_cast<uint8_t>(y));
            }
        GFC256_DIV_TABLE = tab[1];
        GFC256_MUL_TABLE = tab[0];
    });
}
}  // namespace

namespace {
// A staging slot for the duration of one call: a free one, a new one while fewer than
// kMaxStageSlots exist, else the next one released. `rc` != 0: no slot (stream creation failed).
struct SlotLease {
    Context &c;
    StageSlot *s = nullptr;
    int rc = 0;
    explicit SlotLease(Context &cx) : c(cx) {
        std::unique_lock<std::mutex> lk(c.stage_mu);
        for (;;) {
            if (!c.stage_free.empty()) {
                s = c.stage_free.back();
                c.stage_free.pop_back();
                return;
            }
            if (c.stage_all.size() < kMaxStageSlots) break;
            c.stage_cv.wait(lk);
        }
        auto slot = std::make_unique<StageSlot>();
        if (hipStreamCreateWithFlags(&slot->stream, hipStreamNonBlocking) != hipSuccess) {
            std::fprintf(stderr, "libcauchy256: hipStreamCreateWithFlags failed\n");
            rc = -2;
            return;
        }
        s = slot.get();
        c.stage_all.push_back(std::move(slot));
    }
    ~SlotLease() {
        if (!s) return;
        {
            std::lock_guard<std::mutex> g(c.stage_mu);
            c.stage_free.push_back(s);
        }
        c.stage_cv.notify_one();
    }
    SlotLease(const SlotLease &) = delete;
    SlotLease &operator=(const SlotLease &) = delete;
};
}  // namespace

extern "C" int _cauchy_256_init(int expected_version) {
    if (expected_version != CAUCHY_256_VERSION) return -1;  // reference cauchy_256.cpp:392-394
    export_field_tables();
    Context &c = ctx();
    std::lock_guard<std::mutex> g(c.mu);
    return init_locked(c, c.device);
}

extern "C" int cauchy_256_encode(int k, int m, const unsigned char *data_ptrs[],
                                 void *recovery_blocks, int block_bytes) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    if (k <= 0 || m <= 0 || block_bytes <= 0) return 0;
    const int kin = k <= 1 ? 1 : k;
    const size_t in_bytes = static_cast<size_t>(kin) * block_bytes;
    const size_t out_bytes = static_cast<size_t>(m) * block_bytes;
    SlotLease sl(c);
    if (sl.rc) return sl.rc;
    StageSlot &st = *sl.s;
    const size_t scratch = kSliceCap * out_bytes;  // step-slice partials (latency path)
    if (int rc = st.h.ensure(in_bytes + out_bytes)) return rc;
    if (int rc = st.d.ensure(in_bytes + out_bytes + scratch, st.stream)) return rc;
    uint8_t *h = static_cast<uint8_t *>(st.h.p);
    uint8_t *d = static_cast<uint8_t *>(st.d.p);
    for (int x = 0; x < kin; ++x) std::memcpy(h + static_cast<size_t>(x) * block_bytes, data_ptrs[x], block_bytes);
    SH_CHECK(hipMemcpyAsync(d, h, in_bytes, hipMemcpyHostToDevice, st.stream));
    SingleGroupOpts sg;
    sg.slice_scratch = d + in_bytes + out_bytes;
    const int rc = encode_batch(k, m, block_bytes, 1, nullptr, d, d + in_bytes, st.stream, &sg);
    if (rc == -2) {
        (void)hipStreamSynchronize(st.stream);  // the slot is released on return
        return rc;
    }
    // Like the reference, a rejected call has still written recovery row 0.
    const size_t copy = (rc == 0) ? out_bytes : static_cast<size_t>(block_bytes);
    SH_CHECK(hipMemcpyAsync(h + in_bytes, d + in_bytes, copy, hipMemcpyDeviceToHost, st.stream));
    SH_CHECK(hipStreamSynchronize(st.stream));
    std::memcpy(recovery_blocks, h + in_bytes, copy);
    return rc;
}

extern "C" int cauchy_256_decode(int k, int m, Block *blocks, int block_bytes) {
    Context &c = ctx();
    DeviceScope ds(c);
    if (ds.rc) return ds.rc;
    if (k <= 1) {  // cauchy_256.cpp:1236-1240: no data touched
        if (k == 1) blocks[0].row = 0;
        return 0;
    }
    if (block_bytes <= 0) return 0;
    // The reference's sort_blocks (cauchy_256.cpp:522-554) on the host: the recovery blocks in
    // array order receive the erased originals in increasing order. A row listed twice, a row
    // past the generator or more recovery blocks than erasures is outside the reference's
    // contract: rejected (-1) before any GPU work, as the device setup would report it.
    const bool general = m >= 2 && k + m <= 256 && block_bytes % 8 == 0;
    int rec[256], era[256], e = 0, nera = 0;
    if (general) {
        uint8_t seen[256] = {};
        for (int i = 0; i < k; ++i) {
            const int r = blocks[i].row;
            if (r >= k + m || seen[r]++) return -1;
            if (r >= k) rec[e++] = i;
        }
        for (int x = 0; x < k; ++x)
            if (!seen[x]) era[nera++] = x;
        if (e > nera) return -1;
        if (e == 0) return 0;
    }
    const size_t data_bytes = static_cast<size_t>(k) * block_bytes;
    SlotLease sl(c);
    if (sl.rc) return sl.rc;
    StageSlot &st = *sl.s;
    const size_t scratch = kSliceCap * static_cast<size_t>(std::max(m, 1)) * block_bytes;  // step-slice partials
    // staging: [blocks][rows (256)][workspace (general path)][slice partials]
    const size_t ws_off = (data_bytes + 256 + 255) & ~static_cast<size_t>(255);
    DecodeWS probe{};
    const size_t ws_bytes = general ? carve(probe, nullptr, k, m, block_bytes, 1, true, /*latency=*/true) : 0;
    if (int rc = st.h.ensure(ws_off + ws_bytes + 8)) return rc;
    if (int rc = st.d.ensure(ws_off + ws_bytes + scratch, st.stream)) return rc;
    uint8_t *h = static_cast<uint8_t *>(st.h.p);
    uint8_t *d = static_cast<uint8_t *>(st.d.p);
    for (int i = 0; i < k; ++i) {
        std::memcpy(h + static_cast<size_t>(i) * block_bytes, blocks[i].data, block_bytes);
        h[data_bytes + i] = blocks[i].row;
    }
    if (general) {
        // The decode setup runs here (host_decode_setup) where it applies: its workspace fields
        // go up with the blocks in one copy, and the recovered rows come back densely (e blocks,
        // no device scatter kernel) to be placed here.
        DecodeWS wh{};
        carve(wh, h + ws_off, k, m, block_bytes, 1, true, /*latency=*/true);
        SingleGroupOpts sg;
        sg.slice_scratch = d + ws_off + ws_bytes;
        sg.h_dense = h;
        sg.e_dense = e;
        sg.ws_ext = d + ws_off;
        sg.host_setup = host_decode_setup(wh, k, m, h + data_bytes, e, rec, era);
        const size_t up = sg.host_setup ? ws_off + static_cast<size_t>(wh.residual - (h + ws_off)) : data_bytes + k;
        SH_CHECK(hipMemcpyAsync(d, h, up, hipMemcpyHostToDevice, st.stream));
        const int rc = decode_batch(k, m, block_bytes, 1, d, d + data_bytes, st.stream, &sg);
        if (rc != 0) {
            // the staging slot is released on return: nothing queued may still read it
            (void)hipStreamSynchronize(st.stream);
            return rc;
        }
        SH_CHECK(hipStreamSynchronize(st.stream));
        for (int l = 0; l < e; ++l) {
            std::memcpy(blocks[rec[l]].data, h + static_cast<size_t>(l) * block_bytes, block_bytes);
            blocks[rec[l]].row = static_cast<uint8_t>(era[l]);
        }
        return 0;
    }
    SH_CHECK(hipMemcpyAsync(d, h, data_bytes + k, hipMemcpyHostToDevice, st.stream));
    // m == 1 (cauchy_decode_m1) and the parameter-error paths: the batch decode in place
    int *e_host = reinterpret_cast<int *>(h + ((data_bytes + k + 3) & ~static_cast<size_t>(3)));
    *e_host = 0;
    SingleGroupOpts sg;
    sg.e_host = e_host;
    sg.slice_scratch = d + data_bytes + 256;
    const int rc = decode_batch(k, m, block_bytes, 1, d, d + data_bytes, st.stream, &sg);
    if (rc != 0) {
        (void)hipStreamSynchronize(st.stream);
        return rc;
    }
    SH_CHECK(hipMemcpyAsync(h, d, data_bytes + k, hipMemcpyDeviceToHost, st.stream));
    SH_CHECK(hipStreamSynchronize(st.stream));
    if (*e_host < 0) return -1;
    for (int i = 0; i < k; ++i) {
        if (blocks[i].row >= k) {
            std::memcpy(blocks[i].data, h + static_cast<size_t>(i) * block_bytes, block_bytes);
            blocks[i].row = h[data_bytes + i];
        }
    }
    return 0;
}
