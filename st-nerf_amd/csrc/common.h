// Shared host/device helpers for libstnerf_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stnerf.h"

namespace stnerf {

void set_error(const char* fmt, ...);

static inline hipStream_t as_stream(stnerf_stream_t s) { return reinterpret_cast<hipStream_t>(s); }

// Opt a kernel into `bytes` of dynamic LDS (hipFuncAttributeMaxDynamicSharedMemorySize; needed above 64 KiB).  The
// attribute belongs to the (device, function) pair: the cache is keyed by the calling thread's current device and is
// guarded by a mutex, so a process that renders on several GPUs (or from several host threads) opts in on each.
int reserve_dynamic_lds(const void* kernel, int bytes, const char* what);

// Optional launch profiler (stnerf_profile_begin / _end): while enabled, every kernel launch of the op-level
// entry points is bracketed by a HIP event pair recorded on the launch stream.
enum ProfKernel { PROF_SPACENET = 0, PROF_MOTIONNET = 1, PROF_COMPOSITE = 2, PROF_RESAMPLE = 3, PROF_SAMPLE_COARSE = 4, PROF_MLP_STAGE = 5,
                  PROF_COPY_LAYER_RAW = 6, PROF_OCCUPANCY_CULL = 7, PROF_OCCUPANCY_BUILD = 8, PROF_OCCUPANCY_ROWS = 9, PROF_RAY_STOP = 10,
                  PROF_VISIBILITY_ROWS = 11, PROF_BACKGROUND_ROWS = 12, PROF_COPY_LAYER_RAW_LISTED = 13, PROF_SCENE_OCCLUDER = 14,
                  PROF_OCCLUDER_STOP = 15, PROF_DEEP_COUNT = 16, PROF_DEEP_OFFSETS = 17, PROF_DEEP_FILL = 18, PROF_DEEP_COMPOSITE = 19,
                  PROF_PROPOSAL_DENSITY = 20 };
bool profiling_enabled();
void set_launch_tag(int tag);  // e.g. the layer a pipeline launch works on; -1 = none
struct LaunchTimer {            // RAII: records start on construction, stop + bookkeeping on destruction
    LaunchTimer(int kernel, int kind, int64_t n_rays, int ns, int64_t bytes_per_ray, hipStream_t stream);
    ~LaunchTimer();
    void* rec_;
    hipStream_t stream_;
};

// The host checks of a stnerf_occupancy table of l entries (csrc/occupancy.hip), made before any launch.
int check_occupancy_table(const stnerf_occupancy* table, int l, const char* what);
// The same checks of one entry with bits, named `layer` in the messages; refuses layer 0.
int check_occupancy_entry(const stnerf_occupancy* grid, int layer, const char* what);
// The same checks of the background's grid, the one entry the two above refuse; bits are required.
int check_background_grid(const stnerf_occupancy* grid, const char* what);
// The host checks of one density grid with sigma (csrc/proposal.hip), named `layer` in the messages.
int check_density_grid(const stnerf_density_grid* grid, int layer, const char* what);

// One call of the row-list kernel (csrc/sample_rows.hip), as the four rows entries make it after their own refusals.  The tests of
// "listed" are the pointers that are set: ray_flags, t_stop (with t), grid (with xyz; checked by the entry).
struct SampleRowsCall {
    const char* what;              // the entry's name: the prefix of every message
    int prof_kernel, prof_kind;    // the profiler's record (LaunchTimer), with the bytes per ray and the launch tag
    int64_t bytes_per_ray;
    int tag;
    bool by_list;                  // slots of ray_list (null: the slot is the ray), at most *ray_count (null: n) of them
    const int32_t *ray_list, *ray_count;
    const uint8_t* ray_flags;
    int64_t n;
    int ns;
    const float* xyz;
    int64_t xyz_ray_stride;
    const stnerf_occupancy* grid;
    const float* t;
    int64_t t_ray_stride;
    const float* t_stop;
    float* raw;
    int64_t raw_ray_stride;
    int32_t* row_list;
    int64_t capacity;
    int32_t* row_count;
    int64_t* counts;               // the two words this call adds to, or null
    stnerf_stream_t stream;
};
// The shared checks, the row_count memset, the n == 0 return, the choice of kernel and its launch.
int launch_sample_rows(const SampleRowsCall& call);

#define STNERF_REQUIRE(cond, ...)                \
    do {                                         \
        if (!(cond)) {                           \
            ::stnerf::set_error(__VA_ARGS__);    \
            return STNERF_EINVAL;                \
        }                                        \
    } while (0)

#define STNERF_CHECK_LAUNCH(what)                                                        \
    do {                                                                                 \
        hipError_t e_ = hipGetLastError();                                               \
        if (e_ != hipSuccess) {                                                          \
            ::stnerf::set_error("%s: %s", what, hipGetErrorString(e_));                  \
            return STNERF_ELAUNCH;                                                       \
        }                                                                                \
    } while (0)

// Ray window (include/stnerf.h): local ray i of a call -> global ray index of the view.
struct RayWindow {
    int64_t first, stripe, period;
};
__host__ __device__ inline int64_t global_ray(const RayWindow& w, int64_t i) {
    if (w.stripe <= 0) return w.first + i;
    const int64_t s = i / w.stripe;
    return w.first + s * w.period + (i - s * w.stripe);
}
#define STNERF_REQUIRE_WINDOW(what, stripe, period)                                                              \
    STNERF_REQUIRE((stripe) >= 0 && ((stripe) == 0 || (period) >= (stripe)), what ": bad ray window (stripe %lld, period %lld)", \
                   (long long)(stripe), (long long)(period))

// Scene constants passed by value to kernels (small, wave-uniform -> SGPRs).
struct EditArgs {
    stnerf_layer_edit e[STNERF_MAX_LAYERS];
    float pivot[3];
    int32_t any;  // 0: no edit at all
};

static inline void fill_edit_args(EditArgs& a, const stnerf_layer_edit* edits, const float* pivot, int l) {
    a.any = 0;
    for (int i = 0; i < STNERF_MAX_LAYERS; ++i) {
        a.e[i].shift[0] = a.e[i].shift[1] = a.e[i].shift[2] = 0.f;
        a.e[i].scale = 1.f;
        a.e[i].has_shift = a.e[i].has_scale = 0;
    }
    a.pivot[0] = a.pivot[1] = a.pivot[2] = 0.f;
    if (edits) {
        for (int i = 0; i < l; ++i) {
            a.e[i] = edits[i];
            if (edits[i].has_shift || edits[i].has_scale) a.any = 1;
        }
    }
    if (pivot) { a.pivot[0] = pivot[0]; a.pivot[1] = pivot[1]; a.pivot[2] = pivot[2]; }
}

// Per-layer rotations (include/stnerf.h: stnerf_layer_rotation), by value like EditArgs: m = R^T, c = centre; bit i of
// `on` = layer i is rotated.
struct RotArgs {
    float m[STNERF_MAX_LAYERS][9];
    float c[STNERF_MAX_LAYERS][3];
    uint32_t on;
};

static inline void fill_rot_args(RotArgs& a, const stnerf_layer_rotation* rot, int l) {
    a.on = 0;
    for (int i = 0; i < STNERF_MAX_LAYERS; ++i) {
        const bool set = rot && i < l && rot[i].enabled;
        for (int j = 0; j < 9; ++j) a.m[i][j] = set ? rot[i].m[j] : (j % 4 == 0 ? 1.f : 0.f);
        for (int j = 0; j < 3; ++j) a.c[i][j] = set ? rot[i].centre[j] : 0.f;
        if (set) a.on |= 1u << i;
    }
}

#if defined(__HIPCC__)
// d' = R^T d and o' = R^T (o - c) + c of include/stnerf.h, every operation on its own in the stated order (contraction is
// switched off here whatever the file's flags are).
__device__ __forceinline__ void rotate_dir(const float* m, const float d[3], float out[3]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a = m[3 * r] * d[0];
        const float b = m[3 * r + 1] * d[1];
        const float e = m[3 * r + 2] * d[2];
        const float ab = a + b;
        out[r] = ab + e;
    }
}
__device__ __forceinline__ void rotate_ray(const float* m, const float* c, float o[3], float d[3]) {
#pragma clang fp contract(off)
    const float q[3] = {o[0] - c[0], o[1] - c[1], o[2] - c[2]};
    float oq[3], dq[3];
    rotate_dir(m, q, oq);
    rotate_dir(m, d, dq);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        o[r] = oq[r] + c[r];
        d[r] = dq[r];
    }
}

// ---- Philox4x32-10 counter-based RNG (Salmon et al. 2011): stateless, so the draw of
// (ray, layer, sample) does not depend on how rays are chunked or sharded over GPUs.
__device__ __forceinline__ uint4 philox4x32_10(uint4 c, uint2 k) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c.x), lo0 = M0 * c.x;
        const uint32_t hi1 = __umulhi(M1, c.z), lo1 = M1 * c.z;
        c = make_uint4(hi1 ^ c.y ^ k.x, lo1, hi0 ^ c.w ^ k.y, lo0);
        k.x += W0;
        k.y += W1;
    }
    return c;
}

// Uniform in [0,1) on the 2^-24 grid (the grid torch.rand uses for fp32).
__device__ __forceinline__ float philox_uniform(uint64_t seed, uint64_t ray, uint32_t layer, uint32_t stream,
                                                uint32_t sample) {
    const uint4 c = make_uint4((uint32_t)ray, (uint32_t)(ray >> 32), layer | (stream << 16), sample >> 2);
    const uint4 r = philox4x32_10(c, make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    const uint32_t w = (sample & 3) == 0 ? r.x : (sample & 3) == 1 ? r.y : (sample & 3) == 2 ? r.z : r.w;
    return (float)(w >> 8) * 5.9604644775390625e-8f;  // 2^-24
}

// Inverse of the box edit, applied to a sample point.  modeling/layered_rfrender.py:293-303 / :467-475.
// Arithmetic kept as separate IEEE ops (this file set is compiled with -ffp-contract=off).
__device__ __forceinline__ void unedit_point(float& x, float& y, float& z, const stnerf_layer_edit& e,
                                             const float* pivot) {
    if (e.has_shift) {
        x = x - e.shift[0];
        y = y - e.shift[1];
        z = z - e.shift[2];
    }
    if (e.has_scale) {
        x = (x - pivot[0]) / e.scale + pivot[0];
        y = (y - pivot[1]) / e.scale + pivot[1];
        z = (z - pivot[2]) / e.scale + pivot[2];
    }
}
#endif

}  // namespace stnerf
