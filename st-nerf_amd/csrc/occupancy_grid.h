// The point -> cell rule of the occupancy grids (include/stnerf.h: stnerf_occupancy), stated once for the kernels of
// csrc/occupancy.hip and csrc/sample_rows.hip.  Both files are compiled with -ffp-contract=off: the map is a subtraction and a
// product, two separate fp32 operations.
#pragma once
#include <math.h>

#include "common.h"

namespace stnerf {

// One grid by value (wave-uniform -> SGPRs).
struct OccGrid {
    const uint32_t* bits;
    int32_t rx, ry, rz;
    float lo[3], inv[3];
};

static inline OccGrid make_occ_grid(const stnerf_occupancy& t) {
    return OccGrid{t.bits, t.res[0], t.res[1], t.res[2], {t.lo[0], t.lo[1], t.lo[2]}, {t.inv_cell[0], t.inv_cell[1], t.inv_cell[2]}};
}

#if defined(__HIPCC__)
// c_a = min(max((int)floorf((p_a - lo_a) inv_a), 0), R_a - 1); the clamp is taken on the floor's float, which gives the same
// cell for every finite value and for +-inf and keeps the conversion in range.
__device__ __forceinline__ int cell_of(float p, float lo, float inv, int r) {
    const float d = p - lo;
    const float f = floorf(d * inv);
    return (int)fminf(fmaxf(f, 0.f), (float)(r - 1));
}

__device__ __forceinline__ bool point_occupied(const OccGrid& g, float x, float y, float z) {
    if (x != x || y != y || z != z) return true;   // a NaN coordinate counts as occupied
    const int cx = cell_of(x, g.lo[0], g.inv[0], g.rx);
    const int cy = cell_of(y, g.lo[1], g.inv[1], g.ry);
    const int cz = cell_of(z, g.lo[2], g.inv[2], g.rz);
    const int c = (cz * g.ry + cy) * g.rx + cx;    // < 2^24
    return (g.bits[c >> 5] >> (c & 31) & 1u) != 0;
}
#endif

}  // namespace stnerf
