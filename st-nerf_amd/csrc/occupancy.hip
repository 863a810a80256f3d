// Occupancy grids (include/stnerf.h: stnerf_occupancy): a bit per cell of a performer's box, made from the
// networks' own densities at the cell corners (occupancy_build_kernel), and the cull that clears the hit bit of a (ray, layer)
// pair none of whose coarse sample points lies in an occupied cell (occupancy_cull_kernel).  A culled pair is in the state of
// a ray that grazes the box -- bit 0 clear, bit 1 clear, depths real -- which every later kernel already handles.
// Compiled with -ffp-contract=off: the point -> cell map is a subtraction and a product, two separate fp32 operations.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "occupancy_grid.h"   // OccGrid, cell_of, point_occupied: the point -> cell rule, shared with termination.hip

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

// The sample cull's row list.  A wave takes runs of ROWS_RUN consecutive slots of the layer's ray list, run
// after run a whole grid of waves apart.  Pass 1 tests the run's samples -- lane j the samples k = j, j + 64, ... of a ray, one
// ballot per (ray, 64 samples), all of them kept in scalar registers -- and stores the zero float4 of every sample that is not
// listed; then ONE atomic add reserves the run's range of the list, and pass 2 writes the words (ray << 8 | k) from the ballots:
// the rows of a ray contiguous and ascending in k, the runs in the order the adds landed.  NC = ceil(ns / 64) <= 4.
// counts (or null): (samples tested, samples skipped), summed in the wave's registers and added once per wave.
constexpr int ROWS_RUN = 16;
template <int NC>
__global__ void __launch_bounds__(256) occupancy_rows_kernel(const int32_t* __restrict__ ray_list, const int32_t* __restrict__ ray_count, int64_t n,
                                                             const float* __restrict__ xyz, int64_t xyz_ray_stride, int ns, OccGrid g,
                                                             float* __restrict__ raw, int64_t raw_ray_stride, int32_t* __restrict__ row_list,
                                                             int64_t capacity, int32_t* __restrict__ row_count,
                                                             unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    int64_t cnt = n;
    if (ray_count) {
        const int64_t c = *ray_count;
        cnt = c < 0 ? 0 : (c < cnt ? c : cnt);
    }
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long tested = 0ull, skipped = 0ull;    // the same in every lane
    for (int64_t slot0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * ROWS_RUN; slot0 < cnt; slot0 += waves * ROWS_RUN) {
        const int64_t left = cnt - slot0;
        const int m = left < ROWS_RUN ? (int)left : ROWS_RUN;      // rays of this run (uniform)
        int32_t my_ray = 0;
        if (lane < m) my_ray = ray_list ? ray_list[slot0 + lane] : (int32_t)(slot0 + lane);
        unsigned long long bal[ROWS_RUN][NC];
        int listed = 0;
#pragma unroll
        for (int r = 0; r < ROWS_RUN; ++r) {
            const int64_t ray = __builtin_amdgcn_readlane(my_ray, r);
            const float* p = xyz + ray * xyz_ray_stride;
            float4* o = reinterpret_cast<float4*>(raw + ray * raw_ray_stride);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k = 64 * c + lane;
                const bool live = r < m && k < ns;
                bool occ = false;
                if (live) {
                    occ = point_occupied(g, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
                    if (!occ) o[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                bal[r][c] = __ballot(occ);
                listed += __popcll(bal[r][c]);
            }
        }
        tested += (unsigned long long)m * (unsigned long long)ns;
        skipped += (unsigned long long)m * (unsigned long long)ns - (unsigned long long)listed;
        int base = 0;
        if (lane == 0 && listed) base = atomicAdd(row_count, listed);
        int64_t at = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int r = 0; r < ROWS_RUN; ++r) {
            const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane(my_ray, r) << 8;
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const unsigned long long b = bal[r][c];
                const int64_t pos = at + __popcll(b & below);
                if ((b >> lane & 1ull) && pos < capacity) row_list[pos] = (int32_t)(hi | (uint32_t)(64 * c + lane));
                at += __popcll(b);
            }
        }
    }
    if (lane == 0 && counts && tested) {
        atomicAdd(counts, tested);
        if (skipped) atomicAdd(counts + 1, skipped);
    }
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
int check_occupancy_table(const stnerf_occupancy* table, int l, const char* what) {
    STNERF_REQUIRE(table, "%s: null occupancy table", what);
    STNERF_REQUIRE(!table[0].bits, "%s: layer 0 cannot carry an occupancy grid (the background runs on every ray whatever its mask)", what);
    for (int i = 1; i < l; ++i) {
        const stnerf_occupancy& g = table[i];
        if (!g.bits) continue;
        STNERF_REQUIRE(res_ok(g.res), "%s: occupancy grid of layer %d has res (%d, %d, %d), each must be 1..256", what, i, g.res[0], g.res[1],
                       g.res[2]);
        STNERF_REQUIRE(((uintptr_t)g.bits & 3) == 0, "%s: occupancy bits of layer %d must be 4-byte aligned", what, i);
        for (int a = 0; a < 3; ++a) {
            STNERF_REQUIRE(isfinite(g.inv_cell[a]) && g.inv_cell[a] > 0.f, "%s: occupancy grid of layer %d: inv_cell[%d] = %g is not finite and positive",
                           what, i, a, (double)g.inv_cell[a]);
            STNERF_REQUIRE(isfinite(g.lo[a]), "%s: occupancy grid of layer %d: lo[%d] is not finite", what, i, a);
        }
    }
    return STNERF_OK;
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
        OccGrid g{t.bits, t.res[0], t.res[1], t.res[2], {t.lo[0], t.lo[1], t.lo[2]}, {t.inv_cell[0], t.inv_cell[1], t.inv_cell[2]}};
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

// One layer's row list: see include/stnerf.h.  xyz / raw are the LAYER's slices (as in stnerf_stage_layer); `layer` names it for the
// layer-0 refusal, the profiler's tag and the counters' row.
extern "C" int stnerf_occupancy_rows(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz,
                                     int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host, float* raw, int64_t raw_ray_stride,
                                     int32_t* row_list, int64_t capacity, int32_t* row_count, int64_t* counts_or_null, stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && raw && row_list && row_count && grid_host, "occupancy_rows: null pointer");
    STNERF_REQUIRE(layer >= 1 && layer < STNERF_MAX_LAYERS,
                   "occupancy_rows: layer %d: layer 0 cannot carry an occupancy grid (the background is never listed), layers end at %d", layer,
                   STNERF_MAX_LAYERS - 1);
    STNERF_REQUIRE(ns >= 1 && ns <= 256, "occupancy_rows: ns = %d, a row packs the sample into 8 bits: 1..256", ns);
    STNERF_REQUIRE(n >= 0 && n <= ((int64_t)1 << 23), "occupancy_rows: n = %lld, a row packs the ray into 23 bits: at most 2^23", (long long)n);
    STNERF_REQUIRE(capacity >= n * ns, "occupancy_rows: capacity %lld below n x ns = %lld", (long long)capacity, (long long)(n * ns));
    STNERF_REQUIRE((raw_ray_stride & 3) == 0 && ((uintptr_t)raw & 15) == 0, "occupancy_rows: raw must be 16-byte aligned, its ray stride a multiple of 4 floats");
    STNERF_REQUIRE(((uintptr_t)counts_or_null & 7) == 0, "occupancy_rows: counts must be 8-byte aligned");
    STNERF_REQUIRE(grid_host->bits, "occupancy_rows: layer %d has no grid", layer);
    {
        stnerf_occupancy table[STNERF_MAX_LAYERS];
        memset(table, 0, sizeof(table));
        table[layer] = *grid_host;
        const int rc = check_occupancy_table(table, layer + 1, "occupancy_rows");
        if (rc) return rc;
    }
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(row_count, 0, sizeof(int32_t), st) != hipSuccess) {
        set_error("occupancy_rows: hipMemsetAsync failed");
        return STNERF_ELAUNCH;
    }
    if (n == 0) return STNERF_OK;
    const stnerf_occupancy& t = *grid_host;
    OccGrid g{t.bits, t.res[0], t.res[1], t.res[2], {t.lo[0], t.lo[1], t.lo[2]}, {t.inv_cell[0], t.inv_cell[1], t.inv_cell[2]}};
    const int64_t runs = (n + ROWS_RUN - 1) / ROWS_RUN;
    const dim3 grid((unsigned)std::min<int64_t>((runs + 3) / 4, CULL_MAX_BLOCKS));
    unsigned long long* counts = counts_or_null ? reinterpret_cast<unsigned long long*>(counts_or_null) + 2 * layer : nullptr;
    set_launch_tag(layer);
    {
        // per ray: the points read, a zero or a row word per sample (at most 16 bytes)
        LaunchTimer timer(PROF_OCCUPANCY_ROWS, 0, n, ns, 28 * (int64_t)ns + 4, st);
#define STNERF_ROWS_LAUNCH(NC)                                                                                                                  \
    hipLaunchKernelGGL(occupancy_rows_kernel<NC>, grid, dim3(256), 0, st, ray_list, ray_count, n, xyz, xyz_ray_stride, ns, g, raw, raw_ray_stride, \
                       row_list, capacity, row_count, counts)
        if (ns <= 64)
            STNERF_ROWS_LAUNCH(1);
        else if (ns <= 128)
            STNERF_ROWS_LAUNCH(2);
        else
            STNERF_ROWS_LAUNCH(4);
#undef STNERF_ROWS_LAUNCH
    }
    set_launch_tag(-1);
    STNERF_CHECK_LAUNCH("occupancy_rows");
    return STNERF_OK;
}
