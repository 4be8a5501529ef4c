// Which kernel family runs encode and decode stage A: the one place the choice is made. Encode, the
// decode workspace carve (decode stage A and the reserve read its plan) and cauchy_256_batch_path ask.
#pragma once

namespace sh {

enum class StageARoute {
    Fixed,    // compile-time kernels (csrc/gen/fixed_k<K>_m<m>_*.hip) of a K >= k (fixed_kernel_k)
    Tile,     // runtime-coefficient tile kernels (csrc/tile_snip.hip)
    Generic,  // apply_generic (csrc/kernels.hip): any geometry, coefficient bytes
};

struct StageAPlan {
    StageARoute route;
    bool sliced;  // Tile only: one group's steps run as parallel slices (single-group latency path)
    int kp;       // decode position-table stride: round4 of the stage-A kernel's K
};

// The 2 GiB span of the compile-time and tile kernels. fixed::Src, fixed::RowSink and tile::TSrc
// address through one buffer descriptor per workgroup, based at the workgroup's first group and
// capped at 0x7FFFFFFF bytes, with 32-bit offsets
//   input   (gx - g_first) * k * B + col_off + a * sub + p * B      (decode: array index p < k)
//           (gx - g_first) * k * B + col_off + a * sub, + x * B      (encode: step x < k, scalar term)
//   output  (g - g_first) * m * B + col_off + b * sub, + y * B       (row y < m, scalar term)
// and every offset at or past 2^31 is OOR by design: it reads zeros, or stores nothing. Each 16-byte
// access of group g_first + i ends at or before (i + 1) * k * B (input) or (i + 1) * m * B (output),
// so a workgroup stays inside its descriptor iff n * max(k, m) * B <= 0x7FFFFFFF, n = the groups a
// tile can overlap = FixedArgs::groups_per_wg = (COLS - 1) / nq + 2. COLS <= 512 (64 * CW, CW <= 8
// for the compile-time kernels, <= 4 for the tile kernels); the bound takes 512 for every kernel and
// does not look at `groups` (cauchy_256_batch_path has none), so it is conservative: from nq >= 512
// (B >= 16,264) it reads 2 * max(k, m) * B <= 0x7FFFFFFF, and below that it cannot bind
// ((511 / nq + 2) * 255 * B < 2^24 there). The same bound keeps the scalar terms x * B, y * B below
// 2^31. Var-k batches: a tile's well-formed groups are consecutive blocks of the packed array, so
// their window ends within n * kmax * B of its start (k = kmax here).
// Shapes past the bound run apply_generic and stageb_snip, which address through 64-bit pointers.
// Their grids stay in range: grid.x = groups * ceil(nq / 64) (stageb_snip, apply_generic per group)
// or groups * nq / 256 <= total bytes / 2048, grid.z = groups <= 65,535 (a group of such a shape
// holds more than 8 MiB, so more groups than that would need over 512 GiB).
inline bool stagea_span_fits(int k, int m, int B) {
    if (B <= 0 || B % 8 != 0 || B / 8 < 16) return true;  // neither family runs the shape
    const int nq = (((B / 8 + 3) / 4) + 3) & ~3;          // fixed_geometry(B).nq
    const long long n = (512 - 1) / nq + 2;
    return n * (k > m ? k : m) * B <= 0x7FFFFFFFll;
}

// kfix: fixed_kernel_k(k, m, B), 0 = no compile-time kernel. tile: the tile kernels can run the
// shape. slices: latency_slices() of the steps (k; decode k + m) with slice scratch and one group,
// else 1. The tile kernels read position tables round4(k) wide, so below a wider compiled K a
// decode is not sliced and stays Fixed. Decode leaves all m residual rows iff route != Generic.
// fits: stagea_span_fits(k, m, B); a shape that does not fit is Generic whatever else holds.
inline StageAPlan stagea_route(int k, int kfix, bool tile, bool dec, int slices, bool fits = true) {
    if (!fits) {
        kfix = 0;
        tile = false;
    }
    StageAPlan p{};
    p.kp = ((k > kfix ? k : kfix) + 3) & ~3;
    p.sliced = tile && slices > 1 && (!dec || p.kp == ((k + 3) & ~3));
    p.route = kfix > 0 && !p.sliced ? StageARoute::Fixed : tile ? StageARoute::Tile : StageARoute::Generic;
    return p;
}

}  // namespace sh
