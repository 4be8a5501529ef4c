// Wire records of recovery blocks (include/shorthair_wire.h): GenerateRecoveryBlock's framing
// (Shorthair.cpp:598-608), "[k+y][k-1][m-1][block]", for a whole batch as one streaming kernel.
//
// The output wire[groups * m][S], S = 3 + B, is one flat run of bytes at any address. A lane owns one
// address-aligned 16-byte piece of it as two 8-byte words: every store is one aligned 16-byte piece,
// consecutive lanes write consecutive memory and no byte is written twice; only the piece at either end
// of the run, where it is ragged, is written byte by byte. Destination byte D lies in record p = D / S at
// r = D - p * S: r < 3 is a header byte, any other is recovery byte D - 3 (p + 1) -- the source is
// contiguous across records and only the shift grows, by 3 per record. A word touches at most two
// records (S >= 11), so it is one unaligned 8-byte load with up to three header bytes spliced in.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bytes.hpp"
#include "wire.hpp"

namespace sh {
namespace {

constexpr int WIRE_THREADS = 256;
constexpr int WIRE_BYTES = 16 * WIRE_THREADS;  // output bytes per workgroup
constexpr int WIRE_MUL_S = 32768;              // largest record size divided by multiplication

// The header of recovery block y of a group whose first[] entries are f0, f1 (unused when uniform), as
// the low 3 bytes of a word; ok = false for a group malformed by var_group's rule (geometry.hpp).
struct RecInfo {
    uint32_t hdr;
    bool ok;
};
template <bool VAR>
__device__ __forceinline__ RecInfo rec_info(const WireArgs &a, int y, int f0, int f1) {
    int kg = a.k;
    bool ok = true;
    if (VAR) {
        const long long kk = static_cast<long long>(f1) - f0;
        ok = f0 >= 0 && f1 <= a.total && kk >= 2 && kk <= a.k;
        kg = static_cast<int>(kk);
    }
    RecInfo r;
    r.ok = ok;
    r.hdr = ok ? static_cast<uint32_t>(kg + y) | (static_cast<uint32_t>(kg - 1) << 8) |
                     (static_cast<uint32_t>(a.m - 1) << 16)
               : 0;
    return r;
}

// One byte of the run by the rule: the ragged piece at either end.
template <bool VAR>
__device__ uint8_t wire_byte(const WireArgs &a, long long D) {
    const long long p = D / a.S;
    const int r = static_cast<int>(D - p * a.S);
    const int g = static_cast<int>(p / a.m), y = static_cast<int>(p - static_cast<long long>(g) * a.m);
    const RecInfo ri = rec_info<VAR>(a, y, VAR ? a.first[g] : 0, VAR ? a.first[g + 1] : 0);
    if (!ri.ok) return 0;
    return r < 3 ? static_cast<uint8_t>(ri.hdr >> (8 * r)) : a.rec[D - 3 * (p + 1)];
}

template <bool VAR>
__global__ __launch_bounds__(WIRE_THREADS) void wire_emit(WireArgs a) {
    // the workgroup's first byte as (record, offset), and that record as (group, row): one wave-uniform
    // 64-bit division and one 32-bit one
    const long long base = static_cast<long long>(blockIdx.x) * WIRE_BYTES - a.head;
    const long long wb = max(base, 0ll);
    const long long p0 = wb / a.S;
    const uint32_t r0 = static_cast<uint32_t>(wb - p0 * a.S);
    const uint32_t g0 = static_cast<uint32_t>(p0) / static_cast<uint32_t>(a.m);  // p0 < groups * m <= INT_MAX
    const uint32_t y0 = static_cast<uint32_t>(p0) - g0 * a.m;
    const long long D0 = base + 16 * static_cast<int>(threadIdx.x);  // this lane's piece: [D0, D0 + 16)
    if (D0 >= a.run) return;
    if (D0 < 0 || D0 + 16 > a.run) {
        for (long long D = max(D0, 0ll); D < min(D0 + 16, a.run); ++D) a.wire[D] = wire_byte<VAR>(a, D);
        return;
    }
    // both words in step -- positions, then every load, then the splices -- so that the loads of one
    // word do not wait for the other's. Word i starts at offset r[i] of record p[i] = block y[i] of group
    // g[i]; all 16 bytes lie in the run, so every record the piece touches exists.
    long long p[2];
    int r[2], g[2], y[2];
    {
        const uint32_t l = r0 + static_cast<uint32_t>(D0 - wb);  // < S + WIRE_BYTES
        const uint32_t q = a.mul_s ? __umulhi(l, a.mul_s) : l / static_cast<uint32_t>(a.S);
        const uint32_t t = y0 + q;  // < m + WIRE_BYTES / 11 + 2
        const uint32_t gq = a.m == 1 ? t : __umulhi(t, a.mul_m);
        p[0] = p0 + q;
        r[0] = static_cast<int>(l - q * a.S);
        g[0] = static_cast<int>(g0 + gq);
        y[0] = static_cast<int>(t - gq * a.m);
        const bool step = r[0] + 8 >= a.S;  // S > 8: at most one record further
        const bool wrap = step && y[0] + 1 == a.m;
        p[1] = p[0] + step;
        r[1] = r[0] + 8 - (step ? a.S : 0);
        g[1] = g[0] + wrap;
        y[1] = wrap ? 0 : y[0] + step;
    }
    // The header in a word, if any, starts at byte hp of it (-2..7; 8: none): record p's own when the
    // word starts inside it (r < 3), else the next record's. The source bytes of a word are contiguous
    // from s0 whichever records they belong to; the load window is pulled back from the buffer's end.
    int hp[2], shr[2];
    long long ws[2];
    for (int i = 0; i < 2; ++i) {
        hp[i] = r[i] < 3 ? -r[i] : min(a.S - r[i], 8);
        const long long s0 = p[i] * a.B + max(r[i] - 3, 0);
        ws[i] = min(s0, a.src - 8);
        shr[i] = 8 * static_cast<int>(s0 - ws[i]);
    }
    uint64_t x[2];
    int fa[2] = {0, 0}, fb[2] = {0, 0}, fc[2] = {0, 0};  // first[g], first[g + 1], first[g + 2]
    for (int i = 0; i < 2; ++i) x[i] = ld64(a.rec + ws[i]);
    if (VAR)
        for (int i = 0; i < 2; ++i) {
            fa[i] = a.first[g[i]];
            fb[i] = a.first[g[i] + 1];
            fc[i] = a.first[min(g[i] + 2, a.groups)];  // (the last group has no next: a span of 0, unused)
        }
    uint64_t v[2];
    for (int i = 0; i < 2; ++i) {
        const RecInfo own = rec_info<VAR>(a, y[i], fa[i], fb[i]);
        const RecInfo next = y[i] + 1 == a.m ? rec_info<VAR>(a, 0, fb[i], fc[i]) : rec_info<VAR>(a, y[i] + 1, fa[i], fb[i]);
        const RecInfo h = r[i] < 3 ? own : next;  // the record of the header and of the bytes behind it
        const uint64_t xs = x[i] >> shr[i];
        const int nlo = max(hp[i], 0);  // bytes of record p in front of the header
        const uint64_t lo = nlo >= 8 ? xs : xs & ((1ull << (8 * (nlo & 7))) - 1);
        const int t = hp[i] + 3;  // first byte behind the header
        const uint64_t hi = t < 8 ? (xs >> (8 * (nlo & 7))) << (8 * (t & 7)) : 0;
        const uint64_t hw = hp[i] < 0 ? static_cast<uint64_t>(h.hdr >> (8 * (-hp[i] & 3)))
                                      : (hp[i] < 8 ? static_cast<uint64_t>(h.hdr) << (8 * (hp[i] & 7)) : 0);
        v[i] = (own.ok ? lo : 0) | (h.ok ? hi | hw : 0);
    }
    u64x2 o;
    o.x = v[0];
    o.y = v[1];
    *reinterpret_cast<u64x2 *>(a.wire + D0) = o;
}

}  // namespace

hipError_t launch_wire_emit(WireArgs a, hipStream_t stream) {
    if (a.groups <= 0) return hipSuccess;
    a.S = 3 + a.B;
    const long long records = static_cast<long long>(a.groups) * a.m;
    a.run = records * a.S;
    a.src = records * a.B;
    a.head = static_cast<int>(reinterpret_cast<uintptr_t>(a.wire) & 15);
    a.mul_s = a.S <= WIRE_MUL_S ? static_cast<uint32_t>((1ull << 32) / a.S) + 1 : 0;
    a.mul_m = a.m >= 2 ? static_cast<uint32_t>((1ull << 32) / a.m) + 1 : 0;
    const long long wgs = (a.run + a.head + WIRE_BYTES - 1) / WIRE_BYTES;
    if (wgs > 0x7fffffffll) return hipErrorInvalidValue;
    if (a.first)
        hipLaunchKernelGGL(wire_emit<true>, dim3(static_cast<unsigned>(wgs)), dim3(WIRE_THREADS), 0, stream, a);
    else
        hipLaunchKernelGGL(wire_emit<false>, dim3(static_cast<unsigned>(wgs)), dim3(WIRE_THREADS), 0, stream, a);
    return hipGetLastError();
}

}  // namespace sh
