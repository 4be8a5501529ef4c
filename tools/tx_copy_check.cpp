// CPU check of the copy of shorthair_tx_datagram_batch (csrc/tx_datagram_copy.hpp) before it runs on a GPU:
// the kernel's per-lane source, compiled for the host with lane loops in place of the grid, on exact-size
// heap buffers under AddressSanitizer and UBSan (tools/tx_copy_check.sh). A stand-alone program: it is not
// loaded into Python and needs no GPU.
//
// Every case is a datagram of hlen header bytes (5, 6, 11, 14) and a body -- a payload somewhere in a
// payload buffer of exactly payload_bytes, first and last bytes included, or a recovery block in a buffer
// of exactly its size -- copied to all 16 destination alignments by sub-groups of 1..32 lanes. The
// destination is an allocation that ends with the datagram's last byte; the bytes in front of it hold a
// canary. Expected bytes come from the rule: header, then body.
#define SH_TXD_FN static inline
#include "../shorthair_amd/csrc/tx_datagram_copy.hpp"

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

// One datagram: header bytes hdr[0..hlen), body = buf[src..src+blen) of a buffer of buf_bytes bytes.
static bool run_case(int hlen, const uint8_t *buf, long long buf_bytes, long long src, int blen, bool rec) {
    uint8_t hdr[16] = {0};
    for (int i = 0; i < hlen; ++i) hdr[i] = static_cast<uint8_t>(0xA0 + i);
    TxDesc d;
    std::memcpy(&d.h0, hdr, 8);
    std::memcpy(&d.h1, hdr + 8, 8);
    d.src = src;
    d.meta = blen | (hlen << TXD_HLEN_SHIFT) | (rec ? TXD_REC : 0);
    d.local = 0;
    const int L = hlen + blen;
    std::vector<uint8_t> want(static_cast<size_t>(L));
    std::memcpy(want.data(), hdr, static_cast<size_t>(hlen));
    if (blen) std::memcpy(want.data() + hlen, buf + src, static_cast<size_t>(blen));
    for (int a = 0; a < 16; ++a)
        for (int step = 1; step <= 32; step *= 2) {
            // [16 canary][a canary][L datagram], the datagram at alignment a, the allocation ends with it
            const size_t n = 16 + static_cast<size_t>(a) + static_cast<size_t>(L);
            uint8_t *mem = nullptr;
            if (posix_memalign(reinterpret_cast<void **>(&mem), 16, n ? n : 16)) return false;
            std::memset(mem, 0x5C, n);
            uint8_t *dst = mem + 16 + a;
            // the payload and the recovery buffer are distinct: the one not in use is null
            const TxCopy c = txd_plan(d, rec ? nullptr : buf, rec ? 0 : buf_bytes, rec ? buf : nullptr);
            for (int sub = 0; sub < step; ++sub) txd_copy_lane(c, dst, sub, step);
            bool ok = L == 0 || std::memcmp(dst, want.data(), static_cast<size_t>(L)) == 0;
            for (int i = 0; i < 16 + a; ++i) ok = ok && mem[i] == 0x5C;
            std::free(mem);
            ++cases;
            if (!ok) {
                std::fprintf(stderr, "MISMATCH hlen=%d blen=%d src=%lld buf=%lld rec=%d a=%d step=%d\n", hlen, blen,
                             src, buf_bytes, rec, a, step);
                return false;
            }
        }
    return true;
}

int main() {
    const int hlens[4] = {5, 6, 11, 14};
    const int Bs[5] = {8, 16, 24, 136, 1352};
    // payloads: every length class at the start, the end and the middle of an exact-size buffer
    for (int B : Bs) {
        std::vector<int> lens = {0, 1, 2, 3, 7, 8, 9, 10, 11, 12, 15, 16, 17, 27, B - 2};
        for (int i = 0; i < 6; ++i) lens.push_back(static_cast<int>(rnd() % static_cast<uint32_t>(B - 1)));
        for (int len : lens) {
            if (len < 0) continue;
            for (long long buf_bytes : {static_cast<long long>(len), static_cast<long long>(len) + 3, 8ll, 40ll + len}) {
                if (buf_bytes < len) continue;
                uint8_t *buf = static_cast<uint8_t *>(std::malloc(buf_bytes ? static_cast<size_t>(buf_bytes) : 1));
                for (long long i = 0; i < buf_bytes; ++i) buf[i] = static_cast<uint8_t>(rnd());
                for (long long src : {0ll, buf_bytes - len, (buf_bytes - len) / 2})
                    for (int hlen : {5, 14})
                        if (!run_case(hlen, buf, buf_bytes, src, len, false)) return 1;
                std::free(buf);
            }
        }
        // a recovery block: the buffer is exactly the block, or the block is its first or last
        for (int blocks : {1, 3}) {
            const long long bytes = static_cast<long long>(blocks) * B;
            uint8_t *buf = static_cast<uint8_t *>(std::malloc(static_cast<size_t>(bytes)));
            for (long long i = 0; i < bytes; ++i) buf[i] = static_cast<uint8_t>(rnd());
            for (int y = 0; y < blocks; ++y)
                if (!run_case(6, buf, bytes, static_cast<long long>(y) * B, B, true)) return 1;
            std::free(buf);
        }
    }
    // the largest block, and a pong-only datagram
    {
        const int B = 65544;
        uint8_t *buf = static_cast<uint8_t *>(std::malloc(B));
        for (int i = 0; i < B; ++i) buf[i] = static_cast<uint8_t>(rnd());
        if (!run_case(6, buf, B, 0, B, true)) return 1;
        if (!run_case(14, buf, 65535, 0, 65535, false)) return 1;
        std::free(buf);
    }
    for (int hlen : hlens)
        if (!run_case(hlen, nullptr, 0, 0, 0, false)) return 1;
    std::printf("tx_copy_check: %ld cases ok\n", cases);
    return 0;
}
