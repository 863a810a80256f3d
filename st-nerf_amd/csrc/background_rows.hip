// The background's sample cull (include/stnerf.h: "Background sample cull", stnerf_background_rows): the row
// list of layer 0 in a network stage.  The layer-0 flavour of occupancy_rows_kernel (csrc/occupancy.hip) and
// visibility_rows_kernel (csrc/termination.hip): the background runs on EVERY ray, so the slot is the ray -- no ray list, no
// device-side ray count, the launch bounds known on the host -- the grid is mandatory, and the hidden-sample test of early ray
// termination is a template flag.
// Compiled with -ffp-contract=off: the grid's point -> cell map is a subtraction and a product, two separate fp32 operations.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "occupancy_grid.h"   // OccGrid, point_occupied: the point -> cell rule, shared with occupancy.hip and termination.hip

using namespace stnerf;

namespace {

// A wave takes runs of BG_RUN consecutive rays, run after run a whole grid of waves apart.  Pass 1 tests the run's samples -- lane
// j the samples k = j, j + 64, ... of a ray, one ballot per (ray, 64 samples), all of them kept in scalar registers -- and stores
// the zero float4 of every sample that is not listed; then ONE vector atomic add reserves the run's range of the list, and pass 2
// writes the words (ray << 8 | k) from the ballots: the rows of a ray contiguous and ascending in k, the runs in the order the
// adds landed.  Listed: the point in an occupied cell (or NaN) and, with STOP, !(t > t_stop[ray]).  NC = ceil(ns / 64) <= 4.
// The bit table is read through the vector L1 / L2 like any other array: at 256^3 cells it is 2 MB, which an XCD's 4 MB L2 holds
// beside the streamed points; neighbouring samples of a ray fall into the same or the next 128-byte line of it.
// counts (or null): (samples tested, samples not listed), summed in the wave's registers and added once per wave.
constexpr int BG_RUN = 16;
constexpr int64_t BG_MAX_BLOCKS = 2048;   // 8 workgroups of 4 waves on each of 256 CUs
template <int NC, bool STOP>
__global__ void __launch_bounds__(256) background_rows_kernel(int64_t n, const float* __restrict__ xyz, int64_t xyz_ray_stride, int ns, OccGrid g,
                                                              const float* __restrict__ t, int64_t t_ray_stride, const float* __restrict__ t_stop,
                                                              float* __restrict__ raw, int64_t raw_ray_stride, int32_t* __restrict__ row_list,
                                                              int64_t capacity, int32_t* __restrict__ row_count,
                                                              unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: the run's addresses stay scalar)
    const int64_t waves = (int64_t)gridDim.x * 4;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long tested = 0ull, skipped = 0ull;    // the same in every lane
    for (int64_t ray0 = ((int64_t)blockIdx.x * 4 + wave) * BG_RUN; ray0 < n; ray0 += waves * BG_RUN) {
        const int64_t left = n - ray0;
        const int m = left < BG_RUN ? (int)left : BG_RUN;      // rays of this run (uniform)
        float my_stop = 0.f;
        if constexpr (STOP)
            if (lane < m) my_stop = t_stop[ray0 + lane];
        unsigned long long bal[BG_RUN][NC];
        int listed = 0;
#pragma unroll
        for (int r = 0; r < BG_RUN; ++r) {
            const int64_t ray = ray0 + r;                      // (< n wherever it is dereferenced: r < m)
            const float* p = xyz + ray * xyz_ray_stride;
            float4* o = reinterpret_cast<float4*>(raw + ray * raw_ray_stride);
            float stop = 0.f;
            if constexpr (STOP) stop = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_stop), r));
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k = 64 * c + lane;
                const bool live = r < m && k < ns;
                bool on = false;
                if (live) {
                    on = true;
                    if constexpr (STOP) on = !(t[ray * t_ray_stride + k] > stop);   // (a NaN depth is not hidden)
                    if (on) on = point_occupied(g, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
                    if (!on) o[k] = make_float4(0.f, 0.f, 0.f, 0.f);
                }
                bal[r][c] = __ballot(on);
                listed += __popcll(bal[r][c]);
            }
        }
        tested += (unsigned long long)m * (unsigned long long)ns;
        skipped += (unsigned long long)m * (unsigned long long)ns - (unsigned long long)listed;
        int base = 0;
        if (lane == 0 && listed) base = atomicAdd(row_count, listed);
        int64_t at = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int r = 0; r < BG_RUN; ++r) {
            const uint32_t hi = (uint32_t)(ray0 + r) << 8;
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

}  // namespace

namespace stnerf {
// The host checks of the background's grid (a stnerf_occupancy entry with bits), made before any launch: check_occupancy_table's,
// for the one entry that table refuses.
int check_background_grid(const stnerf_occupancy* g, const char* what) {
    STNERF_REQUIRE(g && g->bits, "%s: the background's grid has no bits", what);
    for (int a = 0; a < 3; ++a) {
        STNERF_REQUIRE(g->res[a] >= 1 && g->res[a] <= 256, "%s: the background's grid has res (%d, %d, %d), each must be 1..256", what, g->res[0],
                       g->res[1], g->res[2]);
        STNERF_REQUIRE(isfinite(g->inv_cell[a]) && g->inv_cell[a] > 0.f, "%s: the background's grid: inv_cell[%d] = %g is not finite and positive", what,
                       a, (double)g->inv_cell[a]);
        STNERF_REQUIRE(isfinite(g->lo[a]), "%s: the background's grid: lo[%d] is not finite", what, a);
    }
    STNERF_REQUIRE(((uintptr_t)g->bits & 3) == 0, "%s: the background grid's bits must be 4-byte aligned", what);
    return STNERF_OK;
}
}  // namespace stnerf

// Layer 0's row list of one stage: see include/stnerf.h.  xyz / t / raw are LAYER 0's slices (as in stnerf_stage_layer).
extern "C" int stnerf_background_rows(int64_t n, const float* xyz, int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host,
                                      const float* t_or_null, int64_t t_ray_stride, const float* t_stop_or_null, float* raw,
                                      int64_t raw_ray_stride, int32_t* row_list, int64_t capacity, int32_t* row_count,
                                      int64_t* counts_or_null, stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && raw && row_list && row_count && grid_host, "background_rows: null pointer");
    STNERF_REQUIRE(ns >= 1 && ns <= 256, "background_rows: ns = %d, a row packs the sample into 8 bits: 1..256", ns);
    STNERF_REQUIRE(n >= 0 && n <= ((int64_t)1 << 23), "background_rows: n = %lld, a row packs the ray into 23 bits: at most 2^23", (long long)n);
    STNERF_REQUIRE(capacity >= n * ns, "background_rows: capacity %lld below n x ns = %lld", (long long)capacity, (long long)(n * ns));
    STNERF_REQUIRE((raw_ray_stride & 3) == 0 && ((uintptr_t)raw & 15) == 0, "background_rows: raw must be 16-byte aligned, its ray stride a multiple of 4 floats");
    STNERF_REQUIRE(((uintptr_t)counts_or_null & 7) == 0, "background_rows: counts must be 8-byte aligned");
    STNERF_REQUIRE(!t_stop_or_null || t_or_null, "background_rows: t_stop without the stage's depths t");
    const int grc = check_background_grid(grid_host, "background_rows");
    if (grc) return grc;
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(row_count, 0, sizeof(int32_t), st) != hipSuccess) {
        set_error("background_rows: hipMemsetAsync failed");
        return STNERF_ELAUNCH;
    }
    if (n == 0) return STNERF_OK;
    const OccGrid g = make_occ_grid(*grid_host);
    const int64_t runs = (n + BG_RUN - 1) / BG_RUN;
    const dim3 grid((unsigned)std::min<int64_t>((runs + 3) / 4, BG_MAX_BLOCKS));
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_or_null);
    const bool stop = t_stop_or_null != nullptr;
    set_launch_tag(0);
    {
        // per ray: the points (and with t_stop the depths) read, a zero or a row word per sample (at most 16 bytes)
        LaunchTimer timer(PROF_BACKGROUND_ROWS, stop ? 1 : 0, n, ns, (stop ? 32 : 28) * (int64_t)ns + (stop ? 4 : 0), st);
#define STNERF_BG_LAUNCH(NC, STOP)                                                                                                          \
    hipLaunchKernelGGL((background_rows_kernel<NC, STOP>), grid, dim3(256), 0, st, n, xyz, xyz_ray_stride, ns, g, t_or_null, t_ray_stride, \
                       t_stop_or_null, raw, raw_ray_stride, row_list, capacity, row_count, counts)
#define STNERF_BG_LAUNCH_NC(NC)          \
    do {                                 \
        if (stop)                        \
            STNERF_BG_LAUNCH(NC, true);  \
        else                             \
            STNERF_BG_LAUNCH(NC, false); \
    } while (0)
        if (ns <= 64)
            STNERF_BG_LAUNCH_NC(1);
        else if (ns <= 128)
            STNERF_BG_LAUNCH_NC(2);
        else
            STNERF_BG_LAUNCH_NC(4);
#undef STNERF_BG_LAUNCH_NC
#undef STNERF_BG_LAUNCH
    }
    set_launch_tag(-1);
    STNERF_CHECK_LAUNCH("background_rows");
    return STNERF_OK;
}
