// Early ray termination (include/stnerf.h: stnerf_ray_stop, stnerf_visibility_rows): the depth behind which
// the coarse pass shows a ray to be opaque (ray_stop_kernel), and the fine stage's row list without the samples behind it
// (visibility_rows_kernel: occupancy_rows_kernel's organisation with the depth test, the grid optional, layer 0 allowed).
// Compiled with -ffp-contract=off: the walk is one fp32 add and one fp32 subtraction per step, the grid's point -> cell map a
// subtraction and a product.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "occupancy_grid.h"

using namespace stnerf;

namespace {

// One lane per ray: an l-way merge of the layers' ascending depths with the cursors and the head depths in registers (LCAP of
// each, every index a compile-time constant: the loops over the layers are unrolled and the update of the winning layer is a
// compare per layer).  The lowest layer wins a tie (strict <, layers ascending), which is the stable sort by source index.
// The walk ends one merged sample after the stop: that sample's depth is t_stop.
template <int LCAP>
__global__ void __launch_bounds__(256) ray_stop_kernel(const float* __restrict__ t, const float* __restrict__ wm, int64_t n, int l, int n1,
                                                       float tau, float* __restrict__ t_stop) {
    const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ray >= n) return;
    const float* tr = t + ray * l * n1;
    const float* wr = wm + ray * l * n1;
    int cur[LCAP];
    float head[LCAP];
#pragma unroll
    for (int i = 0; i < LCAP; ++i) {
        cur[i] = 0;
        head[i] = i < l ? tr[(int64_t)i * n1] : 0.f;
    }
    float acc = 0.f, out = INFINITY;
    bool stopped = false;
    const int total = l * n1;
    for (int j = 0; j < total; ++j) {
        int best = -1;
        float bt = 0.f;
#pragma unroll
        for (int i = 0; i < LCAP; ++i)
            if (i < l && cur[i] < n1 && (best < 0 || head[i] < bt)) {
                best = i;
                bt = head[i];
            }
        if (stopped) {   // merged sample j* + 1
            out = bt;
            break;
        }
        float w = 0.f;
#pragma unroll
        for (int i = 0; i < LCAP; ++i)
            if (i == best) {
                w = wr[(int64_t)i * n1 + cur[i]];
                ++cur[i];
                if (cur[i] < n1) head[i] = tr[(int64_t)i * n1 + cur[i]];
            }
        acc = acc + w;
        stopped = !(1.0f - acc > tau);
    }
    t_stop[ray] = out;
}

// occupancy_rows_kernel (csrc/occupancy.hip) with the hidden-sample test: a wave takes runs of VIS_RUN consecutive slots of the
// layer's ray list; pass 1 tests the run's samples -- lane j the samples k = j, j + 64, ... of a ray, one ballot per (ray, 64
// samples), kept in scalar registers -- and stores the zero float4 of every sample that is not listed; ONE atomic add reserves
// the run's range of the list, and pass 2 writes the words (ray << 8 | k) from the ballots.  Listed: !(t > t_stop[ray]) and,
// with GRID, the point in an occupied cell (or NaN).  NC = ceil(ns / 64) <= 4.
constexpr int VIS_RUN = 16;
constexpr int64_t VIS_MAX_BLOCKS = 2048;   // 8 workgroups of 4 waves on each of 256 CUs
template <int NC, bool GRID>
__global__ void __launch_bounds__(256) visibility_rows_kernel(const int32_t* __restrict__ ray_list, const int32_t* __restrict__ ray_count, int64_t n,
                                                              const float* __restrict__ xyz, int64_t xyz_ray_stride, const float* __restrict__ t,
                                                              int64_t t_ray_stride, const float* __restrict__ t_stop, int ns, OccGrid g,
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
    for (int64_t slot0 = ((int64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * VIS_RUN; slot0 < cnt; slot0 += waves * VIS_RUN) {
        const int64_t left = cnt - slot0;
        const int m = left < VIS_RUN ? (int)left : VIS_RUN;      // rays of this run (uniform)
        int32_t my_ray = 0;
        float my_stop = 0.f;
        if (lane < m) {
            my_ray = ray_list ? ray_list[slot0 + lane] : (int32_t)(slot0 + lane);
            my_stop = t_stop[my_ray];
        }
        unsigned long long bal[VIS_RUN][NC];
        int listed = 0;
#pragma unroll
        for (int r = 0; r < VIS_RUN; ++r) {
            const int64_t ray = __builtin_amdgcn_readlane(my_ray, r);
            const float stop = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, my_stop), r));
            const float* p = xyz + ray * xyz_ray_stride;
            const float* tt = t + ray * t_ray_stride;
            float4* o = reinterpret_cast<float4*>(raw + ray * raw_ray_stride);
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const int k = 64 * c + lane;
                const bool live = r < m && k < ns;
                bool on = false;
                if (live) {
                    on = !(tt[k] > stop);                      // (a NaN depth is not hidden)
                    if constexpr (GRID)
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
        for (int r = 0; r < VIS_RUN; ++r) {
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

}  // namespace

extern "C" int stnerf_ray_stop(const float* t, const float* merged_weights, int64_t n, int l, int n1, float tau, float* t_stop,
                               stnerf_stream_t stream) {
    STNERF_REQUIRE(t && merged_weights && t_stop, "ray_stop: null pointer");
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && n1 >= 1, "ray_stop: bad shape");
    STNERF_REQUIRE((int64_t)l * n1 <= 0x7fffffffll && (n + 255) / 256 < (int64_t)1 << 31, "ray_stop: %lld rays of %d x %d samples exceed one launch",
                   (long long)n, l, n1);
    STNERF_REQUIRE(tau >= 0.f && tau < 1.f, "ray_stop: tau = %g outside [0, 1)", (double)tau);
    if (n == 0) return STNERF_OK;
    hipStream_t st = as_stream(stream);
    const dim3 grid((unsigned)((n + 255) / 256));
    {
        // per ray: the depths and the merged weights read (at most), the stop depth written
        LaunchTimer timer(PROF_RAY_STOP, 0, n, n1, 8 * (int64_t)l * n1 + 4, st);
#define STNERF_STOP_LAUNCH(LCAP) hipLaunchKernelGGL(ray_stop_kernel<LCAP>, grid, dim3(256), 0, st, t, merged_weights, n, l, n1, tau, t_stop)
        if (l <= 4)
            STNERF_STOP_LAUNCH(4);
        else if (l <= 8)
            STNERF_STOP_LAUNCH(8);
        else
            STNERF_STOP_LAUNCH(STNERF_MAX_LAYERS);
#undef STNERF_STOP_LAUNCH
    }
    STNERF_CHECK_LAUNCH("ray_stop");
    return STNERF_OK;
}

// One layer's row list under the hidden-sample rule: see include/stnerf.h.  xyz / t / raw are the LAYER's slices.
extern "C" int stnerf_visibility_rows(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz,
                                      int64_t xyz_ray_stride, const float* t, int64_t t_ray_stride, const float* t_stop, int ns,
                                      const stnerf_occupancy* grid_host, float* raw, int64_t raw_ray_stride, int32_t* row_list,
                                      int64_t capacity, int32_t* row_count, int64_t* counts_or_null, stnerf_stream_t stream) {
    STNERF_REQUIRE(t && t_stop && raw && row_list && row_count, "visibility_rows: null pointer");
    STNERF_REQUIRE(layer >= 0 && layer < STNERF_MAX_LAYERS, "visibility_rows: layer %d outside 0..%d", layer, STNERF_MAX_LAYERS - 1);
    STNERF_REQUIRE(ns >= 1 && ns <= 256, "visibility_rows: ns = %d, a row packs the sample into 8 bits: 1..256", ns);
    STNERF_REQUIRE(n >= 0 && n <= ((int64_t)1 << 23), "visibility_rows: n = %lld, a row packs the ray into 23 bits: at most 2^23", (long long)n);
    STNERF_REQUIRE(capacity >= n * ns, "visibility_rows: capacity %lld below n x ns = %lld", (long long)capacity, (long long)(n * ns));
    STNERF_REQUIRE((raw_ray_stride & 3) == 0 && ((uintptr_t)raw & 15) == 0, "visibility_rows: raw must be 16-byte aligned, its ray stride a multiple of 4 floats");
    STNERF_REQUIRE(((uintptr_t)counts_or_null & 7) == 0, "visibility_rows: counts must be 8-byte aligned");
    const bool gridded = grid_host && grid_host->bits;
    if (gridded) {
        STNERF_REQUIRE(xyz, "visibility_rows: a grid needs the layer's points (xyz is null)");
        stnerf_occupancy table[STNERF_MAX_LAYERS];
        memset(table, 0, sizeof(table));
        table[layer] = *grid_host;
        const int rc = check_occupancy_table(table, layer + 1, "visibility_rows");   // (refuses a grid on layer 0)
        if (rc) return rc;
    }
    hipStream_t st = as_stream(stream);
    if (hipMemsetAsync(row_count, 0, sizeof(int32_t), st) != hipSuccess) {
        set_error("visibility_rows: hipMemsetAsync failed");
        return STNERF_ELAUNCH;
    }
    if (n == 0) return STNERF_OK;
    OccGrid g;
    memset(&g, 0, sizeof(g));
    if (gridded) g = make_occ_grid(*grid_host);
    const int64_t runs = (n + VIS_RUN - 1) / VIS_RUN;
    const dim3 grid((unsigned)std::min<int64_t>((runs + 3) / 4, VIS_MAX_BLOCKS));
    unsigned long long* counts = counts_or_null ? reinterpret_cast<unsigned long long*>(counts_or_null) + 2 * layer : nullptr;
    set_launch_tag(layer);
    {
        // per ray: the depths (and with a grid the points) read, a zero or a row word per sample (at most 16 bytes)
        LaunchTimer timer(PROF_VISIBILITY_ROWS, gridded ? 1 : 0, n, ns, (gridded ? 32 : 20) * (int64_t)ns + 8, st);
#define STNERF_VIS_LAUNCH(NC, GRID)                                                                                                             \
    hipLaunchKernelGGL((visibility_rows_kernel<NC, GRID>), grid, dim3(256), 0, st, ray_list, ray_count, n, xyz, xyz_ray_stride, t, t_ray_stride, \
                       t_stop, ns, g, raw, raw_ray_stride, row_list, capacity, row_count, counts)
#define STNERF_VIS_LAUNCH_NC(NC) \
    do {                         \
        if (gridded)             \
            STNERF_VIS_LAUNCH(NC, true);  \
        else                     \
            STNERF_VIS_LAUNCH(NC, false); \
    } while (0)
        if (ns <= 64)
            STNERF_VIS_LAUNCH_NC(1);
        else if (ns <= 128)
            STNERF_VIS_LAUNCH_NC(2);
        else
            STNERF_VIS_LAUNCH_NC(4);
#undef STNERF_VIS_LAUNCH_NC
#undef STNERF_VIS_LAUNCH
    }
    set_launch_tag(-1);
    STNERF_CHECK_LAUNCH("visibility_rows");
    return STNERF_OK;
}
