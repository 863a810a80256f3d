// Reprojection of a key view's rows into a nearby view (include/stnerf.h: stnerf_reproject_splat, stnerf_reproject_resolve,
// stnerf_reproject_holes): the background of a key view, with its depth, is a textured surface; warped into
// a neighbouring view it covers almost every pixel, and the pixels it cannot cover are a list the renderer can already render.
// Three exact helper kernels next to the render path, none of which touches a stage kernel: a forward splat with a 64-bit
// atomic depth test, a resolve that guards against cracks, and the ordered compaction of the holes (csrc/ordered_compact.h).
// Compiled with -ffp-contract=off: every product, quotient, sum and difference of the definitions is one fp32 operation.
#include <cmath>

#include "common.h"
#include "ordered_compact.h"
#include "pinhole_ray.h"

namespace stnerf {

constexpr unsigned long long kEmptyKey = ~0ull;

struct SplatArgs {
    float kinv[9];   // source K^-1
    float T[16];     // source pose
    float K[9];      // destination K
    float W[12];     // destination world-to-camera, 3x4
    float o[3];      // destination camera centre
};

// One lane per source row.  HBM- and atomics-bound: 4 B read and one 8 B atomic per row; no LDS.  iv * w_d + iu < h_d w_d by the
// two range checks, so the one atomic is inside keys.
__global__ void __launch_bounds__(256) reproject_splat_kernel(SplatArgs a, int w_s, const float* __restrict__ t_src, int64_t n,
                                                              uint32_t id_base, int h_d, int w_d, float z_min,
                                                              unsigned long long* __restrict__ keys) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    const float t = t_src[q];
    if (!(t > 0.f) || !(t < INFINITY)) return;  // absent: NaN, infinite, t <= 0
    float o[3], d[3];
    pinhole_pixel_ray(a.kinv, a.T, (int)q, w_s, 0.f, 0.f, o, d);  // (n <= h_s w_s <= INT32_MAX: the host checks)
    float p[3], c[3], pix[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) p[r] = t * d[r] + o[r];
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = ((a.W[4 * r] * p[0] + a.W[4 * r + 1] * p[1]) + a.W[4 * r + 2] * p[2]) + a.W[4 * r + 3];
    if (!(c[2] > z_min)) return;  // behind the destination camera (or NaN)
#pragma unroll
    for (int r = 0; r < 3; ++r) pix[r] = (a.K[3 * r] * c[0] + a.K[3 * r + 1] * c[1]) + a.K[3 * r + 2] * c[2];
    const float u = pix[0] / pix[2];
    const float v = pix[1] / pix[2];
    const float ru = rintf(u);
    const float rv = rintf(v);
    // not finite, or outside the image (the float test makes the conversion safe, the integer test is the rule)
    if (!(ru >= 0.f && ru < 2147483648.f && rv >= 0.f && rv < 2147483648.f)) return;
    const int iu = (int)ru;
    const int iv = (int)rv;
    if (iu >= w_d || iv >= h_d) return;
    const float e0 = p[0] - a.o[0];
    const float e1 = p[1] - a.o[1];
    const float e2 = p[2] - a.o[2];
    const float tp = sqrtf(fmaf(e2, e2, fmaf(e1, e1, e0 * e0)));
    const unsigned long long key = ((unsigned long long)__float_as_uint(tp) << 32) | (unsigned long long)(id_base + (uint32_t)q);
    atomicMin(keys + ((int64_t)iv * w_d + iu), key);
}

struct SourceTable {
    const float* values[STNERF_REPROJECT_MAX_SOURCES];
    int64_t stride[STNERF_REPROJECT_MAX_SOURCES];
    uint32_t end[STNERF_REPROJECT_MAX_SOURCES];  // ids of source s: [end[s-1], end[s])
    int32_t count;
};

// One lane per destination pixel.  HBM-bound: the 9 keys of a neighbourhood are shared with the lanes beside it, so about
// 8 B read plus 4 C B read and 4 C + 8 B written per pixel; no LDS.  A key names a row of its source: id < end[s] by the search.
__global__ void __launch_bounds__(256) reproject_resolve_kernel(const unsigned long long* __restrict__ keys, int h, int w, float guard,
                                                                SourceTable tab, int C, float* __restrict__ values_out,
                                                                float* __restrict__ t_out, int32_t* __restrict__ src_out) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (int64_t)h * w) return;
    const unsigned long long key = keys[j];
    bool hole = key == kEmptyKey;
    float tp = 0.f;
    uint32_t id = 0;
    int s = 0;
    if (!hole) {
        const int y = (int)((uint32_t)j / (uint32_t)w), x = (int)j - y * w;  // (j < h w <= INT32_MAX: a 32-bit quotient)
        unsigned long long least = key;
        for (int dy = -1; dy <= 1; ++dy) {
            const int yy = y + dy;
            if (yy < 0 || yy >= h) continue;
            for (int dx = -1; dx <= 1; ++dx) {
                const int xx = x + dx;
                if (xx < 0 || xx >= w) continue;
                const unsigned long long k = keys[(int64_t)yy * w + xx];  // (an empty key is the largest there is)
                least = k < least ? k : least;
            }
        }
        tp = __uint_as_float((uint32_t)(key >> 32));
        const float m = __uint_as_float((uint32_t)(least >> 32));
        hole = tp > m * guard;
        id = (uint32_t)key;
#pragma unroll
        for (int k = 0; k < STNERF_REPROJECT_MAX_SOURCES; ++k) s += (k < tab.count && id >= tab.end[k]) ? 1 : 0;  // (end ascends)
        hole = hole || s >= tab.count;
    }
    float* out = values_out + j * C;
    if (hole) {
        for (int c = 0; c < C; ++c) out[c] = 0.f;
        t_out[j] = __uint_as_float(0x7fc00000u);
        src_out[j] = -1;
        return;
    }
    const float* values = tab.values[0];  // (selected, not indexed: the table stays in scalar registers)
    int64_t stride = tab.stride[0];
    uint32_t base = 0u;
#pragma unroll
    for (int k = 1; k < STNERF_REPROJECT_MAX_SOURCES; ++k)
        if (s == k) {
            values = tab.values[k];
            stride = tab.stride[k];
            base = tab.end[k - 1];
        }
    const float* row = values + (int64_t)(id - base) * stride;
    for (int c = 0; c < C; ++c) out[c] = row[c];
    t_out[j] = tp;
    src_out[j] = (int32_t)id;
}

struct IsHole {
    const int32_t* src;
    __device__ __forceinline__ bool operator()(int64_t j) const { return src[j] < 0; }
};

}  // namespace stnerf

using namespace stnerf;

extern "C" int stnerf_reproject_splat(const float* Kinv_s_host, const float* T_s_host, int h_s, int w_s, const float* t_src, int64_t n,
                                      int64_t id_base, const float* K_d_host, const float* Wd_host, const float* o_d_host, int h_d,
                                      int w_d, float z_min, uint64_t* keys, stnerf_stream_t stream) {
    STNERF_REQUIRE(Kinv_s_host && T_s_host && t_src && K_d_host && Wd_host && o_d_host && keys, "reproject_splat: null pointer");
    STNERF_REQUIRE(h_s > 0 && w_s > 0 && (int64_t)h_s * w_s <= INT32_MAX, "reproject_splat: bad source view %dx%d", h_s, w_s);
    STNERF_REQUIRE(h_d > 0 && w_d > 0 && (int64_t)h_d * w_d <= INT32_MAX, "reproject_splat: bad destination view %dx%d", h_d, w_d);
    STNERF_REQUIRE(n >= 0 && n <= (int64_t)h_s * w_s, "reproject_splat: %lld rows for a %dx%d source", (long long)n, h_s, w_s);
    STNERF_REQUIRE(id_base >= 0 && id_base + n <= ((int64_t)1 << 31), "reproject_splat: ids %lld + %lld do not stay below 2^31",
                   (long long)id_base, (long long)n);
    STNERF_REQUIRE(std::isfinite(z_min) && z_min >= 0.f, "reproject_splat: z_min must be finite and >= 0");
    if (n == 0) return STNERF_OK;
    SplatArgs a;
    for (int i = 0; i < 9; ++i) a.kinv[i] = Kinv_s_host[i];
    for (int i = 0; i < 16; ++i) a.T[i] = T_s_host[i];
    for (int i = 0; i < 9; ++i) a.K[i] = K_d_host[i];
    for (int i = 0; i < 12; ++i) a.W[i] = Wd_host[i];
    for (int i = 0; i < 3; ++i) a.o[i] = o_d_host[i];
    const int bs = 256;
    hipLaunchKernelGGL(reproject_splat_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, as_stream(stream), a, w_s, t_src, n,
                       (uint32_t)id_base, h_d, w_d, z_min, reinterpret_cast<unsigned long long*>(keys));
    STNERF_CHECK_LAUNCH("reproject_splat");
    return STNERF_OK;
}

extern "C" int stnerf_reproject_resolve(const uint64_t* keys, int h_d, int w_d, float rel, const stnerf_reproject_source* sources_host,
                                        int n_sources, int C, float* values_out, float* t_out, int32_t* src_out,
                                        stnerf_stream_t stream) {
    STNERF_REQUIRE(keys && sources_host && values_out && t_out && src_out, "reproject_resolve: null pointer");
    STNERF_REQUIRE(h_d > 0 && w_d > 0 && (int64_t)h_d * w_d <= INT32_MAX, "reproject_resolve: bad view %dx%d", h_d, w_d);
    STNERF_REQUIRE(C >= 1 && C <= 64, "reproject_resolve: bad width C=%d (1 <= C <= 64)", C);
    STNERF_REQUIRE(rel >= 0.f, "reproject_resolve: rel must be >= 0");
    STNERF_REQUIRE(n_sources >= 1 && n_sources <= STNERF_REPROJECT_MAX_SOURCES, "reproject_resolve: %d sources (1..%d)", n_sources,
                   STNERF_REPROJECT_MAX_SOURCES);
    SourceTable tab;
    int64_t end = 0;
    for (int s = 0; s < STNERF_REPROJECT_MAX_SOURCES; ++s) {
        if (s < n_sources) {
            const stnerf_reproject_source& r = sources_host[s];
            STNERF_REQUIRE(r.n >= 0 && r.n <= INT32_MAX, "reproject_resolve: source %d has %lld rows", s, (long long)r.n);
            STNERF_REQUIRE(r.values || r.n == 0, "reproject_resolve: source %d: null pointer", s);
            STNERF_REQUIRE(r.row_stride >= C, "reproject_resolve: source %d: row stride %lld < C = %d", s, (long long)r.row_stride, C);
            end += r.n;
            STNERF_REQUIRE(end <= INT32_MAX, "reproject_resolve: %lld ids do not stay below 2^31", (long long)end);
        }
        tab.values[s] = s < n_sources ? sources_host[s].values : nullptr;
        tab.stride[s] = s < n_sources ? sources_host[s].row_stride : 0;
        tab.end[s] = (uint32_t)end;
    }
    tab.count = n_sources;
    const float guard = 1.0f + rel;
    const int bs = 256;
    const int64_t P = (int64_t)h_d * w_d;
    hipLaunchKernelGGL(reproject_resolve_kernel, dim3((unsigned)((P + bs - 1) / bs)), dim3(bs), 0, as_stream(stream),
                       reinterpret_cast<const unsigned long long*>(keys), h_d, w_d, guard, tab, C, values_out, t_out, src_out);
    STNERF_CHECK_LAUNCH("reproject_resolve");
    return STNERF_OK;
}

extern "C" int64_t stnerf_reproject_holes_workspace_bytes(int64_t n_pixels) {
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "reproject_holes_workspace_bytes: bad pixel count %lld", (long long)n_pixels);
    return select_workspace_bytes(n_pixels);
}

extern "C" int stnerf_reproject_holes(const int32_t* src, int64_t n_pixels, int32_t* holes_out, int32_t* n_out, void* workspace,
                                      int64_t workspace_bytes, stnerf_stream_t stream) {
    STNERF_REQUIRE(src && holes_out && n_out && workspace, "reproject_holes: null pointer");
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "reproject_holes: bad pixel count %lld", (long long)n_pixels);
    STNERF_REQUIRE(workspace_bytes >= select_workspace_bytes(n_pixels), "reproject_holes: workspace too small (%lld B, %lld needed)",
                   (long long)workspace_bytes, (long long)select_workspace_bytes(n_pixels));
    const IsHole pred{src};
    return ordered_compact(pred, n_pixels, reinterpret_cast<int32_t*>(workspace), holes_out, n_out, as_stream(stream),
                           "reproject_holes (count)", "reproject_holes (scan)", "reproject_holes (write)");
}
