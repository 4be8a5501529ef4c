// CPU check of the copy of shorthair_rx_window_batch (csrc/rx_window_copy.hpp: tx_datagram_copy.hpp with a
// header of 0 bytes and the ring as the payload buffer) before it runs on a GPU: the kernel's per-lane
// source, compiled for the host with lane loops in place of the grid, on exact-size heap buffers under
// AddressSanitizer and UBSan (tools/rx_window_copy_check.sh). A stand-alone program: it is not loaded into
// Python and needs no GPU.
//
// Every case is a record of `len` bytes at the start, the middle or the end of a source buffer of exactly
// ring_bytes bytes, copied to all 16 destination alignments by sub-groups of 1..32 lanes. The destination
// is an allocation of its own that ends with the record's last byte; the bytes in front of it hold a canary.
// The source is compared with a copy taken before: the copy must not write it.
#define SH_TXD_FN static inline
#include "../shorthair_amd/csrc/rx_window_copy.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace sh;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return static_cast<uint32_t>(rng_state >> 33);
}

static long cases = 0;

static bool run_case(const uint8_t *ring, long long ring_bytes, long long off, int len) {
    for (int a = 0; a < 16; ++a)
        for (int step = 1; step <= 32; ++step) {
            // [16 canary][a canary][len record], the record at alignment a, the allocation ends with it
            const size_t n = 16 + static_cast<size_t>(a) + static_cast<size_t>(len);
            uint8_t *mem = nullptr;
            if (posix_memalign(reinterpret_cast<void **>(&mem), 16, n)) return false;
            std::memset(mem, 0x5C, n);
            uint8_t *dst = mem + 16 + a;
            const TxCopy c = rxw_copy_plan(ring, ring_bytes, off, len);
            for (int sub = 0; sub < step; ++sub) txd_copy_lane(c, dst, sub, step);
            bool ok = len == 0 || std::memcmp(dst, ring + off, static_cast<size_t>(len)) == 0;
            for (int i = 0; i < 16 + a; ++i) ok = ok && mem[i] == 0x5C;
            std::free(mem);
            ++cases;
            if (!ok) {
                std::fprintf(stderr, "MISMATCH len=%d off=%lld ring=%lld a=%d step=%d\n", len, off, ring_bytes, a, step);
                return false;
            }
        }
    return true;
}

int main() {
    std::vector<int> lens;
    for (int len = 0; len <= 40; ++len) lens.push_back(len);
    for (int B : {8, 136, 1400}) lens.push_back(B + 3);
    lens.push_back(65547);
    for (int len : lens)
        for (long long ring_bytes : {static_cast<long long>(len), static_cast<long long>(len) + 3, 8ll, 40ll + len}) {
            if (ring_bytes < len) continue;
            const size_t n = ring_bytes ? static_cast<size_t>(ring_bytes) : 1;
            uint8_t *ring = static_cast<uint8_t *>(std::malloc(n));
            for (long long i = 0; i < ring_bytes; ++i) ring[i] = static_cast<uint8_t>(rnd());
            std::vector<uint8_t> before(ring, ring + ring_bytes);
            for (long long off : {0ll, (ring_bytes - len) / 2, ring_bytes - len})
                if (!run_case(ring, ring_bytes, off, len)) return 1;
            if (ring_bytes && std::memcmp(ring, before.data(), static_cast<size_t>(ring_bytes)) != 0) {
                std::fprintf(stderr, "SOURCE WRITTEN len=%d ring=%lld\n", len, ring_bytes);
                return 1;
            }
            std::free(ring);
        }
    std::printf("rx_window_copy_check: %ld cases ok\n", cases);
    return 0;
}
