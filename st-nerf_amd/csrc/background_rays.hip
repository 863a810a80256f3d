// The background's per-ray mask (include/stnerf.h: "Per-ray background mask", stnerf_background_ray_rows): the
// row list of layer 0 in a network stage when the caller says, ray by ray, whether the background is to be evaluated.  The sibling
// of background_rows_kernel (csrc/background_rows.hip) with one more test in front of its two -- the ray's flag byte -- and with the
// grid optional: a sample is listed when its ray's byte is nonzero AND (GRID) its point lies in an occupied cell or is NaN AND
// (STOP) !(t > t_stop[ray]).  A ray whose byte is zero loads no point, no depth and no grid word: it only stores its zeros.
// Compiled with -ffp-contract=off: the grid's point -> cell map is a subtraction and a product, two separate fp32 operations.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "occupancy_grid.h"   // OccGrid, point_occupied: the point -> cell rule, stated once

using namespace stnerf;

namespace {

// The organisation of background_rows_kernel: a wave takes runs of BR_RUN consecutive rays, run after run a whole grid of waves
// apart; pass 1 tests the run's samples -- lane j the samples k = j, j + 64, ... of a ray, one ballot per (ray, 64 samples), all of
// them in scalar registers -- and stores the zero float4 of every sample that is not listed; ONE vector atomic add reserves the
// run's range of the list; pass 2 writes the words (ray << 8 | k) from the ballots: the rows of a ray contiguous and ascending in k.
// New here: the run's BR_RUN flag bytes are loaded once (lane r the byte of ray r) and balloted into a wave-uniform mask, so the
// branch around a masked ray's loads is a scalar one.  NC = ceil(ns / 64) <= 4.
// counts (or null): (samples tested, samples not listed); a masked ray's samples are both tested and not listed.
constexpr int BR_RUN = 16;
constexpr int64_t BR_MAX_BLOCKS = 2048;   // 8 workgroups of 4 waves on each of 256 CUs
template <int NC, bool GRID, bool STOP>
__global__ void __launch_bounds__(256) background_ray_rows_kernel(int64_t n, const uint8_t* __restrict__ ray_flags, const float* __restrict__ xyz,
                                                                  int64_t xyz_ray_stride, int ns, OccGrid g, const float* __restrict__ t,
                                                                  int64_t t_ray_stride, const float* __restrict__ t_stop, float* __restrict__ raw,
                                                                  int64_t raw_ray_stride, int32_t* __restrict__ row_list, int64_t capacity,
                                                                  int32_t* __restrict__ row_count, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));   // (wave-uniform: the run's addresses stay scalar)
    const int64_t waves = (int64_t)gridDim.x * 4;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long tested = 0ull, skipped = 0ull;    // the same in every lane
    for (int64_t ray0 = ((int64_t)blockIdx.x * 4 + wave) * BR_RUN; ray0 < n; ray0 += waves * BR_RUN) {
        const int64_t left = n - ray0;
        const int m = left < BR_RUN ? (int)left : BR_RUN;      // rays of this run (uniform)
        bool flag = false;
        float my_stop = 0.f;
        if (lane < m) {
            flag = ray_flags[ray0 + lane] != 0;
            if constexpr (STOP) my_stop = t_stop[ray0 + lane];
        }
        const unsigned long long wanted = __ballot(flag);     // bit r: ray r of the run is evaluated (uniform; 0 for r >= m)
        unsigned long long bal[BR_RUN][NC];
        int listed = 0;
#pragma unroll
        for (int r = 0; r < BR_RUN; ++r) {
            const int64_t ray = ray0 + r;                      // (< n wherever it is dereferenced: r < m)
            const float* p = xyz + ray * xyz_ray_stride;
            float4* o = reinterpret_cast<float4*>(raw + ray * raw_ray_stride);
            const bool ray_on = (wanted >> r & 1ull) != 0;     // (uniform: a scalar branch)
            float stop = 0.f;
            if constexpr (STOP) stop = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_stop), r));
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k = 64 * c + lane;
                const bool live = r < m && k < ns;
                bool on = false;
                if (live) {
                    if (ray_on) {
                        on = true;
                        if constexpr (STOP) on = !(t[ray * t_ray_stride + k] > stop);   // (a NaN depth is not hidden)
                        if constexpr (GRID)
                            if (on) on = point_occupied(g, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
                    }
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
        for (int r = 0; r < BR_RUN; ++r) {
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

// Layer 0's row list of one stage under a per-ray mask: see include/stnerf.h.  xyz / t / raw are LAYER 0's slices.
extern "C" int stnerf_background_ray_rows(int64_t n, const float* xyz, int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host_or_null,
                                          const float* t_or_null, int64_t t_ray_stride, const float* t_stop_or_null, float* raw,
                                          int64_t raw_ray_stride, int32_t* row_list, int64_t capacity, int32_t* row_count,
                                          int64_t* counts_or_null, const uint8_t* ray_flags, stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && raw && row_list && row_count, "background_ray_rows: null pointer");
    STNERF_REQUIRE(ray_flags, "background_ray_rows: ray_flags is required (one byte per ray; stnerf_background_rows is the call without a mask)");
    STNERF_REQUIRE(ns >= 1 && ns <= 256, "background_ray_rows: ns = %d, a row packs the sample into 8 bits: 1..256", ns);
    STNERF_REQUIRE(n >= 0 && n <= ((int64_t)1 << 23), "background_ray_rows: n = %lld, a row packs the ray into 23 bits: at most 2^23", (long long)n);
    STNERF_REQUIRE(capacity >= n * ns, "background_ray_rows: capacity %lld below n x ns = %lld", (long long)capacity, (long long)(n * ns));
    STNERF_REQUIRE((raw_ray_stride & 3) == 0 && ((uintptr_t)raw & 15) == 0,
                   "background_ray_rows: raw must be 16-byte aligned, its ray stride a multiple of 4 floats");
    STNERF_REQUIRE(((uintptr_t)counts_or_null & 7) == 0, "background_ray_rows: counts must be 8-byte aligned");
    STNERF_REQUIRE(!t_stop_or_null || t_or_null, "background_ray_rows: t_stop without the stage's depths t");
    if (grid_host_or_null) {
        const int grc = check_background_grid(grid_host_or_null, "background_ray_rows");
        if (grc) return grc;
    }
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(row_count, 0, sizeof(int32_t), st) != hipSuccess) {
        set_error("background_ray_rows: hipMemsetAsync failed");
        return STNERF_ELAUNCH;
    }
    if (n == 0) return STNERF_OK;
    OccGrid g;
    memset(&g, 0, sizeof(g));
    if (grid_host_or_null) g = make_occ_grid(*grid_host_or_null);
    const int64_t runs = (n + BR_RUN - 1) / BR_RUN;
    const dim3 grid((unsigned)std::min<int64_t>((runs + 3) / 4, BR_MAX_BLOCKS));
    unsigned long long* counts = reinterpret_cast<unsigned long long*>(counts_or_null);
    const bool cells = grid_host_or_null != nullptr, stop = t_stop_or_null != nullptr;
    set_launch_tag(0);
    {
        // per ray: the flag byte, at most the points (and with t_stop the depths) read, a zero or a row word per sample (at most 16 bytes)
        LaunchTimer timer(PROF_BACKGROUND_ROWS, (stop ? 1 : 0) | 2, n, ns, ((cells ? 12 : 0) + (stop ? 4 : 0) + 16) * (int64_t)ns + (stop ? 5 : 1), st);
#define STNERF_BR_LAUNCH(NC, GRID, STOP)                                                                                                      \
    hipLaunchKernelGGL((background_ray_rows_kernel<NC, GRID, STOP>), grid, dim3(256), 0, st, n, ray_flags, xyz, xyz_ray_stride, ns, g, t_or_null, \
                       t_ray_stride, t_stop_or_null, raw, raw_ray_stride, row_list, capacity, row_count, counts)
#define STNERF_BR_LAUNCH_NC(NC)                  \
    do {                                         \
        if (cells && stop)                       \
            STNERF_BR_LAUNCH(NC, true, true);    \
        else if (cells)                          \
            STNERF_BR_LAUNCH(NC, true, false);   \
        else if (stop)                           \
            STNERF_BR_LAUNCH(NC, false, true);   \
        else                                     \
            STNERF_BR_LAUNCH(NC, false, false);  \
    } while (0)
        if (ns <= 64)
            STNERF_BR_LAUNCH_NC(1);
        else if (ns <= 128)
            STNERF_BR_LAUNCH_NC(2);
        else
            STNERF_BR_LAUNCH_NC(4);
#undef STNERF_BR_LAUNCH_NC
#undef STNERF_BR_LAUNCH
    }
    set_launch_tag(-1);
    STNERF_CHECK_LAUNCH("background_ray_rows");
    return STNERF_OK;
}
