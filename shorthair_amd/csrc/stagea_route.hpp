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

// kfix: fixed_kernel_k(k, m, B), 0 = no compile-time kernel. tile: the tile kernels can run the
// shape. slices: latency_slices() of the steps (k; decode k + m) with slice scratch and one group,
// else 1. The tile kernels read position tables round4(k) wide, so below a wider compiled K a
// decode is not sliced and stays Fixed. Decode leaves all m residual rows iff route != Generic.
inline StageAPlan stagea_route(int k, int kfix, bool tile, bool dec, int slices) {
    StageAPlan p{};
    p.kp = ((k > kfix ? k : kfix) + 3) & ~3;
    p.sliced = tile && slices > 1 && (!dec || p.kp == ((k + 3) & ~3));
    p.route = kfix > 0 && !p.sliced ? StageARoute::Fixed : tile ? StageARoute::Tile : StageARoute::Generic;
    return p;
}

}  // namespace sh
