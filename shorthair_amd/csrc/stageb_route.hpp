// Which kernel runs decode stage B (csrc/stageb.hip): the one place the choice is made. The
// workspace carve, the host restatement of the decode setup and every launcher's guard call it.
#pragma once

#include "geometry.hpp"

namespace sh {

enum class StageBRoute {
    Snip,   // stageb_snip: any geometry, byte coefficients, the emax rows of a generic stage A
    Regs,   // stageb_regs: emax <= 8, setup-written snippet addresses (DecodeSetupArgs::targets)
    Small,  // stageb_small: nq <= 16 word columns (B <= 512), per-lane byte coefficients
    V2,     // stageb_v2: emax > 8, byte coefficients, one workgroup per (group, 64-column chunk)
};

// fixed_geo: fixed_geometry(B). emax = min(k, m) <= 128 (k + m <= 256). full_residual: stage A
// (compile-time or tile kernels) leaves all m residual rows; only then, and only with whole
// 4-column chunks of a sub-block of >= 16 bytes, can the three residual kernels run.
// Measured bounds: stageb_v2 beats stageb_regs from emax = 9 on ((64,16) e = 16:
// 0.229 vs 0.280 ms), stageb_regs beats a one-wave stageb_v2 below ((28,4,1400): 0.114 vs 0.132 ms).
inline StageBRoute stageb_route(const Geometry &fixed_geo, int emax, bool full_residual) {
    if (!full_residual || fixed_geo.nq % 4 != 0 || fixed_geo.sub < 16 || emax < 1) return StageBRoute::Snip;
    if (fixed_geo.nq <= 16) return StageBRoute::Small;
    return emax > 8 ? StageBRoute::V2 : StageBRoute::Regs;
}

}  // namespace sh
