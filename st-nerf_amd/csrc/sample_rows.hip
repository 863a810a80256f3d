// The row lists of a network stage (include/stnerf.h: "Row lists"): the one kernel behind
// stnerf_occupancy_rows, stnerf_visibility_rows, stnerf_background_rows and stnerf_background_ray_rows, and their four entries.
// A sample is listed when every test its entry asks for holds: (FLAGS) its ray's flag byte is nonzero, (STOP) !(t > t_stop[ray]),
// (GRID) its point lies in an occupied cell or is NaN.  The slots are those of a compacted ray list with its count on the device
// (LIST) or the rays 0..n-1 themselves.
// Compiled with -ffp-contract=off: the grid's point -> cell map is a subtraction and a product, two separate fp32 operations.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"
#include "occupancy_grid.h"   // OccGrid, point_occupied: the point -> cell rule, stated once

using namespace stnerf;

namespace {

// A wave takes runs of ROWS_RUN consecutive slots, run after run a whole grid of waves apart.  Pass 1 tests the run's samples --
// lane j the samples k = j, j + 64, ... of a ray, one ballot per (ray, 64 samples), all of them kept in scalar registers -- and
// stores the zero float4 of every sample that is not listed; then ONE vector atomic add reserves the run's range of the list, and
// pass 2 writes the words (ray << 8 | k) from the ballots: the rows of a ray contiguous and ascending in k, the runs in the order
// the adds landed.  NC = ceil(ns / 64) <= 4.
// LIST: lane r holds the run's ray r (ray_list[slot], or the slot where ray_list is null) and the count is min(n, *ray_count).
// Without it the slot is the ray, the bounds are known on the host, and the wave index is made wave-uniform so that the run's
// addresses stay scalar.
// FLAGS: the run's flag bytes are loaded once (lane r the byte of ray r) and balloted into a wave-uniform mask, so the branch
// around a masked ray's loads is a scalar one: such a ray loads no point, no depth and no grid word, it only stores its zeros.
// The bit table is read through the vector L1 / L2 like any other array: at 256^3 cells it is 2 MB, which an XCD's 4 MB L2 holds
// beside the streamed points; neighbouring samples of a ray fall into the same or the next 128-byte line of it.
// counts (or null): (samples tested, samples not listed), summed in the wave's registers and added once per wave as one 64-bit
// add per counter; a masked ray's samples are both tested and not listed.
constexpr int ROWS_RUN = 16;
constexpr int64_t ROWS_MAX_BLOCKS = 2048;   // 8 workgroups of 4 waves on each of 256 CUs
template <int NC, bool LIST, bool FLAGS, bool GRID, bool STOP>
__global__ void __launch_bounds__(256) sample_rows_kernel(const int32_t* __restrict__ ray_list, const int32_t* __restrict__ ray_count,
                                                          const uint8_t* __restrict__ ray_flags, int64_t n, const float* __restrict__ xyz,
                                                          int64_t xyz_ray_stride, const float* __restrict__ t, int64_t t_ray_stride,
                                                          const float* __restrict__ t_stop, int ns, OccGrid g, float* __restrict__ raw,
                                                          int64_t raw_ray_stride, int32_t* __restrict__ row_list, int64_t capacity,
                                                          int32_t* __restrict__ row_count, unsigned long long* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    int wave = (int)(threadIdx.x >> 6);
    if constexpr (!LIST) wave = __builtin_amdgcn_readfirstlane(wave);
    const int64_t waves = (int64_t)gridDim.x * 4;
    int64_t cnt = n;
    if constexpr (LIST)
        if (ray_count) {
            const int64_t c = *ray_count;
            cnt = c < 0 ? 0 : (c < cnt ? c : cnt);
        }
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long tested = 0ull, skipped = 0ull;    // the same in every lane
    for (int64_t slot0 = ((int64_t)blockIdx.x * 4 + wave) * ROWS_RUN; slot0 < cnt; slot0 += waves * ROWS_RUN) {
        const int64_t left = cnt - slot0;
        const int m = left < ROWS_RUN ? (int)left : ROWS_RUN;      // rays of this run (uniform)
        int32_t my_ray = 0;
        bool flag = false;
        float my_stop = 0.f;
        if (lane < m) {
            if constexpr (LIST) my_ray = ray_list ? ray_list[slot0 + lane] : (int32_t)(slot0 + lane);
            if constexpr (FLAGS) flag = ray_flags[LIST ? (int64_t)my_ray : slot0 + lane] != 0;
            if constexpr (STOP) my_stop = t_stop[LIST ? (int64_t)my_ray : slot0 + lane];
        }
        unsigned long long wanted = ~0ull;
        if constexpr (FLAGS) wanted = __ballot(flag);         // bit r: ray r of the run is evaluated (uniform; 0 for r >= m)
        unsigned long long bal[ROWS_RUN][NC];
        int listed = 0;
#pragma unroll
        for (int r = 0; r < ROWS_RUN; ++r) {
            int64_t ray = slot0 + r;                           // (< n wherever it is dereferenced: r < m)
            if constexpr (LIST) ray = __builtin_amdgcn_readlane(my_ray, r);
            const float* p = xyz + ray * xyz_ray_stride;
            const float* tt = t + ray * t_ray_stride;
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
                        if constexpr (STOP) on = !(tt[k] > stop);   // (a NaN depth is not hidden)
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
        for (int r = 0; r < ROWS_RUN; ++r) {
            uint32_t hi = (uint32_t)(slot0 + r) << 8;
            if constexpr (LIST) hi = (uint32_t)__builtin_amdgcn_readlane(my_ray, r) << 8;
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

// The combinations (LIST, FLAGS, GRID, STOP) the four entries use, and no other: occupancy_rows; visibility_rows without and with
// a grid; background_rows without and with t_stop; background_ray_rows' four.
#define STNERF_ROWS_COMBINATIONS(X, NC)                                                                       \
    X(NC, true, false, true, false)                                                                           \
    X(NC, true, false, false, true) X(NC, true, false, true, true)                                            \
    X(NC, false, false, true, false) X(NC, false, false, true, true)                                          \
    X(NC, false, true, false, false) X(NC, false, true, false, true) X(NC, false, true, true, false) X(NC, false, true, true, true)

}  // namespace

namespace stnerf {
int launch_sample_rows(const SampleRowsCall& c) {
    const char* what = c.what;
    STNERF_REQUIRE(c.ns >= 1 && c.ns <= 256, "%s: ns = %d, a row packs the sample into 8 bits: 1..256", what, c.ns);
    STNERF_REQUIRE(c.n >= 0 && c.n <= ((int64_t)1 << 23), "%s: n = %lld, a row packs the ray into 23 bits: at most 2^23", what, (long long)c.n);
    STNERF_REQUIRE(c.capacity >= c.n * c.ns, "%s: capacity %lld below n x ns = %lld", what, (long long)c.capacity, (long long)(c.n * c.ns));
    STNERF_REQUIRE((c.raw_ray_stride & 3) == 0 && ((uintptr_t)c.raw & 15) == 0, "%s: raw must be 16-byte aligned, its ray stride a multiple of 4 floats",
                   what);
    STNERF_REQUIRE(((uintptr_t)c.counts & 7) == 0, "%s: counts must be 8-byte aligned", what);
    const int nc = c.ns <= 64 ? 1 : c.ns <= 128 ? 2 : 4;
    const bool list = c.by_list, flags = c.ray_flags != nullptr, cells = c.grid != nullptr, stop = c.t_stop != nullptr;
    decltype(&sample_rows_kernel<1, true, false, true, false>) kernel = nullptr;
#define STNERF_ROWS_PICK(NC, LIST, FLAGS, GRID, STOP) \
    if (nc == NC && list == LIST && flags == FLAGS && cells == GRID && stop == STOP) kernel = sample_rows_kernel<NC, LIST, FLAGS, GRID, STOP>;
    STNERF_ROWS_COMBINATIONS(STNERF_ROWS_PICK, 1)
    STNERF_ROWS_COMBINATIONS(STNERF_ROWS_PICK, 2)
    STNERF_ROWS_COMBINATIONS(STNERF_ROWS_PICK, 4)
#undef STNERF_ROWS_PICK
    STNERF_REQUIRE(kernel, "%s: no row-list kernel is compiled for this combination of tests", what);
    hipStream_t st = as_stream(c.stream);
    if (hipMemsetAsync(c.row_count, 0, sizeof(int32_t), st) != hipSuccess) {
        set_error("%s: hipMemsetAsync failed", what);
        return STNERF_ELAUNCH;
    }
    if (c.n == 0) return STNERF_OK;
    OccGrid g;
    memset(&g, 0, sizeof(g));
    if (c.grid) g = make_occ_grid(*c.grid);
    const int64_t runs = (c.n + ROWS_RUN - 1) / ROWS_RUN;
    const dim3 grid((unsigned)std::min<int64_t>((runs + 3) / 4, ROWS_MAX_BLOCKS));
    set_launch_tag(c.tag);
    {
        LaunchTimer timer(c.prof_kernel, c.prof_kind, c.n, c.ns, c.bytes_per_ray, st);
        hipLaunchKernelGGL(kernel, grid, dim3(256), 0, st, c.ray_list, c.ray_count, c.ray_flags, c.n, c.xyz, c.xyz_ray_stride, c.t, c.t_ray_stride,
                           c.t_stop, c.ns, g, c.raw, c.raw_ray_stride, c.row_list, c.capacity, c.row_count,
                           reinterpret_cast<unsigned long long*>(c.counts));
    }
    set_launch_tag(-1);
    STNERF_CHECK_LAUNCH(what);
    return STNERF_OK;
}
}  // namespace stnerf

// One performer layer's row list under its grid.  xyz / raw are the LAYER's slices (as in stnerf_stage_layer); `layer` names it for
// the layer-0 refusal, the profiler's tag and the counters' row.
extern "C" int stnerf_occupancy_rows(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz,
                                     int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host, float* raw, int64_t raw_ray_stride,
                                     int32_t* row_list, int64_t capacity, int32_t* row_count, int64_t* counts_or_null, stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && raw && row_list && row_count && grid_host, "occupancy_rows: null pointer");
    STNERF_REQUIRE(layer >= 1 && layer < STNERF_MAX_LAYERS,
                   "occupancy_rows: layer %d: layer 0 cannot carry an occupancy grid (the background is never listed), layers end at %d", layer,
                   STNERF_MAX_LAYERS - 1);
    STNERF_REQUIRE(grid_host->bits, "occupancy_rows: layer %d has no grid", layer);
    const int rc = check_occupancy_entry(grid_host, layer, "occupancy_rows");
    if (rc) return rc;
    SampleRowsCall c{};
    c.what = "occupancy_rows";
    // per ray: the points read, a zero or a row word per sample (at most 16 bytes)
    c.prof_kernel = PROF_OCCUPANCY_ROWS, c.prof_kind = 0, c.bytes_per_ray = 28 * (int64_t)ns + 4, c.tag = layer;
    c.by_list = true, c.ray_list = ray_list, c.ray_count = ray_count;
    c.n = n, c.ns = ns, c.xyz = xyz, c.xyz_ray_stride = xyz_ray_stride, c.grid = grid_host;
    c.raw = raw, c.raw_ray_stride = raw_ray_stride, c.row_list = row_list, c.capacity = capacity, c.row_count = row_count;
    c.counts = counts_or_null ? counts_or_null + 2 * layer : nullptr, c.stream = stream;
    return launch_sample_rows(c);
}

// One layer's row list under the hidden-sample rule.  xyz / t / raw are the LAYER's slices.
extern "C" int stnerf_visibility_rows(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz,
                                      int64_t xyz_ray_stride, const float* t, int64_t t_ray_stride, const float* t_stop, int ns,
                                      const stnerf_occupancy* grid_host, float* raw, int64_t raw_ray_stride, int32_t* row_list,
                                      int64_t capacity, int32_t* row_count, int64_t* counts_or_null, stnerf_stream_t stream) {
    STNERF_REQUIRE(t && t_stop && raw && row_list && row_count, "visibility_rows: null pointer");
    STNERF_REQUIRE(layer >= 0 && layer < STNERF_MAX_LAYERS, "visibility_rows: layer %d outside 0..%d", layer, STNERF_MAX_LAYERS - 1);
    const bool gridded = grid_host && grid_host->bits;
    if (gridded) {
        STNERF_REQUIRE(xyz, "visibility_rows: a grid needs the layer's points (xyz is null)");
        const int rc = check_occupancy_entry(grid_host, layer, "visibility_rows");   // (refuses a grid on layer 0)
        if (rc) return rc;
    }
    SampleRowsCall c{};
    c.what = "visibility_rows";
    // per ray: the depths (and with a grid the points) read, a zero or a row word per sample (at most 16 bytes)
    c.prof_kernel = PROF_VISIBILITY_ROWS, c.prof_kind = gridded ? 1 : 0, c.bytes_per_ray = (gridded ? 32 : 20) * (int64_t)ns + 8, c.tag = layer;
    c.by_list = true, c.ray_list = ray_list, c.ray_count = ray_count;
    c.n = n, c.ns = ns, c.xyz = xyz, c.xyz_ray_stride = xyz_ray_stride, c.grid = gridded ? grid_host : nullptr;
    c.t = t, c.t_ray_stride = t_ray_stride, c.t_stop = t_stop;
    c.raw = raw, c.raw_ray_stride = raw_ray_stride, c.row_list = row_list, c.capacity = capacity, c.row_count = row_count;
    c.counts = counts_or_null ? counts_or_null + 2 * layer : nullptr, c.stream = stream;
    return launch_sample_rows(c);
}

namespace {
// Layer 0's row list of one stage, with or without a per-ray mask: xyz / t / raw are LAYER 0's slices, counts its own two words.
int background_rows(const char* what, int64_t n, const float* xyz, int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_or_null,
                    const float* t_or_null, int64_t t_ray_stride, const float* t_stop_or_null, float* raw, int64_t raw_ray_stride,
                    int32_t* row_list, int64_t capacity, int32_t* row_count, int64_t* counts_or_null, const uint8_t* flags_or_null,
                    stnerf_stream_t stream) {
    STNERF_REQUIRE(!t_stop_or_null || t_or_null, "%s: t_stop without the stage's depths t", what);
    if (grid_or_null) {
        const int grc = check_background_grid(grid_or_null, what);
        if (grc) return grc;
    }
    const bool cells = grid_or_null != nullptr, stop = t_stop_or_null != nullptr;
    SampleRowsCall c{};
    c.what = what;
    c.prof_kernel = PROF_BACKGROUND_ROWS, c.tag = 0;
    if (flags_or_null) {
        // per ray: the flag byte, at most the points (and with t_stop the depths) read, a zero or a row word per sample (at most 16 bytes)
        c.prof_kind = (stop ? 1 : 0) | 2, c.bytes_per_ray = ((cells ? 12 : 0) + (stop ? 4 : 0) + 16) * (int64_t)ns + (stop ? 5 : 1);
    } else {
        // per ray: the points (and with t_stop the depths) read, a zero or a row word per sample (at most 16 bytes)
        c.prof_kind = stop ? 1 : 0, c.bytes_per_ray = (stop ? 32 : 28) * (int64_t)ns + (stop ? 4 : 0);
    }
    c.ray_flags = flags_or_null;
    c.n = n, c.ns = ns, c.xyz = xyz, c.xyz_ray_stride = xyz_ray_stride, c.grid = grid_or_null;
    c.t = t_or_null, c.t_ray_stride = t_ray_stride, c.t_stop = t_stop_or_null;
    c.raw = raw, c.raw_ray_stride = raw_ray_stride, c.row_list = row_list, c.capacity = capacity, c.row_count = row_count;
    c.counts = counts_or_null, c.stream = stream;
    return launch_sample_rows(c);
}
}  // namespace

extern "C" int stnerf_background_rows(int64_t n, const float* xyz, int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host,
                                      const float* t_or_null, int64_t t_ray_stride, const float* t_stop_or_null, float* raw,
                                      int64_t raw_ray_stride, int32_t* row_list, int64_t capacity, int32_t* row_count,
                                      int64_t* counts_or_null, stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && raw && row_list && row_count && grid_host, "background_rows: null pointer");
    return background_rows("background_rows", n, xyz, xyz_ray_stride, ns, grid_host, t_or_null, t_ray_stride, t_stop_or_null, raw, raw_ray_stride,
                           row_list, capacity, row_count, counts_or_null, nullptr, stream);
}

extern "C" int stnerf_background_ray_rows(int64_t n, const float* xyz, int64_t xyz_ray_stride, int ns, const stnerf_occupancy* grid_host_or_null,
                                          const float* t_or_null, int64_t t_ray_stride, const float* t_stop_or_null, float* raw,
                                          int64_t raw_ray_stride, int32_t* row_list, int64_t capacity, int32_t* row_count,
                                          int64_t* counts_or_null, const uint8_t* ray_flags, stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && raw && row_list && row_count, "background_ray_rows: null pointer");
    STNERF_REQUIRE(ray_flags, "background_ray_rows: ray_flags is required (one byte per ray; stnerf_background_rows is the call without a mask)");
    return background_rows("background_ray_rows", n, xyz, xyz_ray_stride, ns, grid_host_or_null, t_or_null, t_ray_stride, t_stop_or_null, raw,
                           raw_ray_stride, row_list, capacity, row_count, counts_or_null, ray_flags, stream);
}
