// Occupancy grids (include/stnerf.h: stnerf_occupancy): a bit per cell of a performer's box, made from the
// networks' own densities at the cell corners (occupancy_build_kernel), and the cull that clears the hit bit of a (ray, layer)
// pair none of whose coarse sample points lies in an occupied cell (occupancy_cull_kernel).  A culled pair is in the state of
// a ray that grazes the box -- bit 0 clear, bit 1 clear, depths real -- which every later kernel already handles.  Also the host
// checks of a grid, for every entry that takes one.  The sample cull's row list is stnerf_occupancy_rows (csrc/sample_rows.hip).
// Compiled with -ffp-contract=off: the point -> cell map is a subtraction and a product, two separate fp32 operations.
#include <math.h>
#include <stdio.h>

#include <algorithm>

#include "common.h"
#include "occupancy_grid.h"   // OccGrid, cell_of, point_occupied: the point -> cell rule, shared with sample_rows.hip

using namespace stnerf;

namespace {

// One wave per ray of `layer` at a time: lanes take the pair's points k = lane, lane + 64, ... (12-byte points, contiguous), the
// wave stops at the first trip with a hit, then goes on to the ray a whole grid of waves further.  counts (or null): [l][2] =
// (pairs tested, pairs culled), summed in the wave's registers and added once per wave as one 64-bit add: an add per tested
// pair, all to one address, serialises in the memory and was 20 ms of a 1080p frame (profiles/occupancy_ab.md).
__global__ void __launch_bounds__(256) occupancy_cull_kernel(const float* __restrict__ xyz, int64_t n, int l, int layer, int n1, OccGrid g,
                                                             uint8_t* __restrict__ mask, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    unsigned long long seen = 0ull;                // tested | culled << 32, the same in every lane
    for (int64_t ray = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); ray < n; ray += waves) {
        const int64_t pair = ray * l + layer;
        const uint8_t m = mask[pair];
        if (!(m & 1)) continue;
        const float* p = xyz + pair * n1 * 3;
        bool hit = false;
        for (int k0 = 0; k0 < n1 && !hit; k0 += 64) {
            const int k = k0 + lane;
            bool occ = false;
            if (k < n1) occ = point_occupied(g, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
            hit = __ballot(occ) != 0ull;
        }
        if (!hit && lane == 0) mask[pair] = m & (uint8_t)~1u;
        seen += 1ull | (hit ? 0ull : 1ull << 32);
    }
    if (lane == 0 && counts && seen) atomicAdd(counts + layer, seen);
}

// dense: !(sigma <= threshold) in either array (a NaN is dense)
__device__ __forceinline__ bool vertex_dense(const float* __restrict__ sc, const float* __restrict__ sf, int64_t v, float thr) {
    return (sc && !(sc[v] <= thr)) || (sf && !(sf[v] <= thr));
}

// One lane per cell, a wave per 64 consecutive cells = two words of the table.  A cell of the grid grown by `dilate` is set when
// a cell within that Chebyshev distance has a dense corner: one of the vertices [x - dilate, x + 1 + dilate] per axis, cut to
// the grid.  Cells past the last one vote 0, so the unused high bits of the last word are 0.
__global__ void __launch_bounds__(256) occupancy_build_kernel(const float* __restrict__ sc, const float* __restrict__ sf, int rx, int ry, int rz,
                                                              float thr, int dilate, uint32_t* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int cells = rx * ry * rz, words = (cells + 31) >> 5;
    const int c = (int)(blockIdx.x * 256u + threadIdx.x);
    bool occ = false;
    if (c < cells) {
        const int x = c % rx, y = (c / rx) % ry, z = c / (rx * ry);
        const int x0 = max(x - dilate, 0), x1 = min(x + 1 + dilate, rx);
        const int y0 = max(y - dilate, 0), y1 = min(y + 1 + dilate, ry);
        const int z0 = max(z - dilate, 0), z1 = min(z + 1 + dilate, rz);
        for (int k = z0; k <= z1 && !occ; ++k)
            for (int j = y0; j <= y1 && !occ; ++j)
                for (int i = x0; i <= x1 && !occ; ++i)
                    occ = vertex_dense(sc, sf, ((int64_t)k * (ry + 1) + j) * (rx + 1) + i, thr);
    }
    const unsigned long long bal = __ballot(occ);
    const int w0 = (c - lane) >> 5;    // the wave's first cell is a multiple of 64
    if (lane == 0 && w0 < words) bits[w0] = (uint32_t)bal;
    if (lane == 32 && w0 + 1 < words) bits[w0 + 1] = (uint32_t)(bal >> 32);
}

// 8 workgroups of 4 waves on each of 256 CUs: every wave slot of the device, and at most 8192 adds to a counter per launch
constexpr int64_t CULL_MAX_BLOCKS = 2048;

bool res_ok(const int32_t* res) {
    for (int a = 0; a < 3; ++a)
        if (res[a] < 1 || res[a] > 256) return false;
    return true;
}

}  // namespace

namespace stnerf {
// The checks of one entry with bits, shared by every caller.  layer names the grid in the messages; 0 is the background's.
static int check_grid(const stnerf_occupancy& g, int layer, const char* what) {
    char grid[48] = "the background's grid", bits[48] = "the background grid's bits";
    if (layer) {
        snprintf(grid, sizeof(grid), "occupancy grid of layer %d", layer);
        snprintf(bits, sizeof(bits), "occupancy bits of layer %d", layer);
    }
    STNERF_REQUIRE(res_ok(g.res), "%s: %s has res (%d, %d, %d), each must be 1..256", what, grid, g.res[0], g.res[1], g.res[2]);
    STNERF_REQUIRE(((uintptr_t)g.bits & 3) == 0, "%s: %s must be 4-byte aligned", what, bits);
    for (int a = 0; a < 3; ++a) {
        STNERF_REQUIRE(isfinite(g.inv_cell[a]) && g.inv_cell[a] > 0.f, "%s: %s: inv_cell[%d] = %g is not finite and positive", what, grid, a,
                       (double)g.inv_cell[a]);
        STNERF_REQUIRE(isfinite(g.lo[a]), "%s: %s: lo[%d] is not finite", what, grid, a);
    }
    return STNERF_OK;
}

int check_occupancy_entry(const stnerf_occupancy* g, int layer, const char* what) {
    STNERF_REQUIRE(layer != 0, "%s: layer 0 cannot carry an occupancy grid (the background runs on every ray whatever its mask)", what);
    return check_grid(*g, layer, what);
}

int check_occupancy_table(const stnerf_occupancy* table, int l, const char* what) {
    STNERF_REQUIRE(table, "%s: null occupancy table", what);
    for (int i = 0; i < l; ++i) {
        if (!table[i].bits) continue;
        const int rc = check_occupancy_entry(&table[i], i, what);
        if (rc) return rc;
    }
    return STNERF_OK;
}

int check_background_grid(const stnerf_occupancy* g, const char* what) {
    STNERF_REQUIRE(g && g->bits, "%s: the background's grid has no bits", what);
    return check_grid(*g, 0, what);
}
}  // namespace stnerf

extern "C" int stnerf_occupancy_build(const float* sigma_c, const float* sigma_f, const int32_t res[3], float threshold, int dilate,
                                      uint32_t* bits, stnerf_stream_t stream) {
    STNERF_REQUIRE(res && bits && (sigma_c || sigma_f), "occupancy_build: null pointer (one of sigma_c / sigma_f is required)");
    STNERF_REQUIRE(res_ok(res), "occupancy_build: res (%d, %d, %d), each must be 1..256", res[0], res[1], res[2]);
    STNERF_REQUIRE(dilate >= 0 && dilate <= 4, "occupancy_build: dilate %d outside 0..4", dilate);
    STNERF_REQUIRE(threshold == threshold, "occupancy_build: the threshold is NaN");
    STNERF_REQUIRE(((uintptr_t)bits & 3) == 0, "occupancy_build: bits must be 4-byte aligned");
    const int cells = res[0] * res[1] * res[2];
    hipStream_t st = as_stream(stream);
    LaunchTimer timer(PROF_OCCUPANCY_BUILD, dilate, cells, 1, 0, st);
    hipLaunchKernelGGL(occupancy_build_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, sigma_c, sigma_f, res[0], res[1], res[2],
                       threshold, dilate, bits);
    STNERF_CHECK_LAUNCH("occupancy_build");
    return STNERF_OK;
}

extern "C" int stnerf_occupancy_cull(const float* xyz, int64_t n, int l, int n1, const stnerf_occupancy* table_host, uint8_t* mask,
                                     int32_t* counts_or_null, stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && mask, "occupancy_cull: null pointer");
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && n1 >= 1, "occupancy_cull: bad shape");
    STNERF_REQUIRE((n + 3) / 4 < (int64_t)1 << 31, "occupancy_cull: %lld rays exceed one launch", (long long)n);
    STNERF_REQUIRE(((uintptr_t)counts_or_null & 7) == 0, "occupancy_cull: counts must be 8-byte aligned");
    const int rc = check_occupancy_table(table_host, l, "occupancy_cull");
    if (rc) return rc;
    if (n == 0) return STNERF_OK;
    hipStream_t st = as_stream(stream);
    for (int i = 1; i < l; ++i) {
        const stnerf_occupancy& t = table_host[i];
        if (!t.bits) continue;
        const OccGrid g = make_occ_grid(t);
        set_launch_tag(i);
        {
            LaunchTimer timer(PROF_OCCUPANCY_CULL, 0, n, n1, 12 * (int64_t)n1 + 2, st);
            hipLaunchKernelGGL(occupancy_cull_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, CULL_MAX_BLOCKS)), dim3(256), 0, st, xyz, n, l, i, n1, g, mask,
                               reinterpret_cast<unsigned long long*>(counts_or_null));
        }
        set_launch_tag(-1);
        STNERF_CHECK_LAUNCH("occupancy_cull");
    }
    return STNERF_OK;
}
