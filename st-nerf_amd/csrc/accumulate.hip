// Progressive multi-sample frames (include/stnerf.h: stnerf_generate_rays_list, stnerf_accumulate, stnerf_accumulate_select;
// DESIGN.md section 7): a frame is the per-pixel mean of several passes, each with its own sub-pixel offset, shutter time and
// seed, and a pixel stops being sampled once its running mean is known well enough.  Three exact helper kernels around the
// render path, none of which touches a stage kernel: a ray generator over a pixel list, a Welford scatter-accumulator, and an
// ordered, deterministic compaction of the pixels that are still active.
// Compiled with -ffp-contract=off: every product, quotient and sum of the definitions is one fp32 operation.
#include "common.h"
#include "ordered_compact.h"
#include "pinhole_ray.h"

namespace stnerf {

// ------------------------------------------------------------------------------------- rays of a pixel list
struct RayListArgs {
    float kinv[9];
    float T[16];
    float frame_ids[STNERF_MAX_LAYERS + 1];
};

// generate_rays_kernel (csrc/sampler.hip) with the pixel taken from a list and moved by (du, dv); every other operation in
// that kernel's order (csrc/pinhole_ray.h).  One lane per row; a list entry outside [0, h w) leaves its row unwritten.
__global__ void generate_rays_list_kernel(RayListArgs a, int w, int64_t n_pixels, const int32_t* __restrict__ pixels, int64_t n,
                                          float du, float dv, int n_frame_cols, float* __restrict__ rays, int ray_stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t pix = pixels ? (int64_t)pixels[i] : i;
    if (pix < 0 || pix >= n_pixels) return;
    float o[3], d[3];
    pinhole_pixel_ray(a.kinv, a.T, (int)pix, w, du, dv, o, d);  // (h w <= INT32_MAX: the host checks)
    float* r = rays + i * ray_stride;
    r[0] = o[0];
    r[1] = o[1];
    r[2] = o[2];
    r[3] = d[0];
    r[4] = d[1];
    r[5] = d[2];
    for (int c = 0; c < n_frame_cols; ++c) r[6 + c] = a.frame_ids[c];
}

// ------------------------------------------------------------------------------------- Welford scatter-accumulator
// One lane per (row, column): consecutive lanes read consecutive floats of `values` and, without a list, of `mean`; with an
// ascending list the rows of `mean` are whole and in order.  HBM-bound: 3 C + 2 V floats and one count per row.  The count is
// only READ here -- by every lane of the row, which may sit in different waves and workgroups; accumulate_count_kernel, the
// next launch on the stream, writes it.  A pixel outside [0, P) is skipped (both kernels).
__global__ void __launch_bounds__(256) accumulate_kernel(const float* __restrict__ values, int64_t n, int C, int64_t value_stride,
                                                         const int32_t* __restrict__ pixels, int64_t P, int V,
                                                         float* __restrict__ mean, float* __restrict__ m2,
                                                         const int32_t* __restrict__ count) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * C) return;
    const int64_t i = e / C;
    const int col = (int)(e - i * C);
    const int64_t q = pixels ? (int64_t)pixels[i] : i;
    if (q < 0 || q >= P) return;
    const float x = values[i * value_stride + col];
    const int c = count[q] + 1;
    if (c == 1) {  // the value itself: one pass reproduces the plain frame's bits (x + 0 would turn -0 into +0)
        mean[q * C + col] = x;
        if (col < V) m2[q * V + col] = 0.f;
        return;
    }
    const float m = mean[q * C + col];
    const float d = x - m;
    const float step = d / (float)c;
    const float mn = m + step;
    mean[q * C + col] = mn;
    if (col < V) {
        const float back = x - mn;
        const float prod = d * back;
        m2[q * V + col] = m2[q * V + col] + prod;
    }
}

__global__ void __launch_bounds__(256) accumulate_count_kernel(int64_t n, const int32_t* __restrict__ pixels, int64_t P,
                                                               int32_t* __restrict__ count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t q = pixels ? (int64_t)pixels[i] : i;
    if (q < 0 || q >= P) return;
    count[q] = count[q] + 1;
}

// ------------------------------------------------------------------------------------- the pixels still active
// (the three launches of the ordered compaction: csrc/ordered_compact.h)

// The rule of include/stnerf.h, as written there.
__device__ __forceinline__ bool pixel_active(const float* __restrict__ m2, const int32_t* __restrict__ count, int64_t q, int V,
                                             int min_spp, int max_spp, float tol2) {
    const int c = count[q];
    if (c < min_spp) return true;
    if (c >= max_spp) return false;
    const float bound = tol2 * (float)(c * (c - 1));
    bool any = false;
    for (int v = 0; v < V; ++v) any = any || (m2[q * V + v] > bound);
    return any;
}

struct PixelActive {
    const float* m2;
    const int32_t* count;
    int V, min_spp, max_spp;
    float tol2;
    __device__ __forceinline__ bool operator()(int64_t q) const { return pixel_active(m2, count, q, V, min_spp, max_spp, tol2); }
};

}  // namespace stnerf

using namespace stnerf;

extern "C" int stnerf_generate_rays_list(const float* Kinv_host, const float* T_host, int h, int w, const int32_t* pixels, int64_t n,
                                         float du, float dv, const float* frame_ids_host, int n_frame_cols, float* rays,
                                         int ray_stride, stnerf_stream_t stream) {
    STNERF_REQUIRE(Kinv_host && T_host && rays, "generate_rays_list: null pointer");
    STNERF_REQUIRE(h > 0 && w > 0 && (int64_t)h * w <= INT32_MAX, "generate_rays_list: bad view %dx%d", h, w);
    STNERF_REQUIRE(n >= 0 && n <= (int64_t)h * w, "generate_rays_list: %lld rows for a %dx%d view (a list names a pixel at most once)",
                   (long long)n, h, w);
    STNERF_REQUIRE(du == du && dv == dv, "generate_rays_list: the offset is NaN");
    STNERF_REQUIRE(n_frame_cols >= 0 && n_frame_cols <= STNERF_MAX_LAYERS + 1 && ray_stride >= 6 + n_frame_cols,
                   "generate_rays_list: bad frame-id columns %d / stride %d", n_frame_cols, ray_stride);
    STNERF_REQUIRE(n_frame_cols == 0 || frame_ids_host, "generate_rays_list: frame_ids is null");
    if (n == 0) return STNERF_OK;
    RayListArgs a;
    for (int i = 0; i < 9; ++i) a.kinv[i] = Kinv_host[i];
    for (int i = 0; i < 16; ++i) a.T[i] = T_host[i];
    for (int i = 0; i < STNERF_MAX_LAYERS + 1; ++i) a.frame_ids[i] = i < n_frame_cols ? frame_ids_host[i] : 0.f;
    const int bs = 256;
    hipLaunchKernelGGL(generate_rays_list_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, as_stream(stream), a, w,
                       (int64_t)h * w, pixels, n, du, dv, n_frame_cols, rays, ray_stride);
    STNERF_CHECK_LAUNCH("generate_rays_list");
    return STNERF_OK;
}

extern "C" int stnerf_accumulate(const float* values, int64_t n, int C, int64_t value_stride, const int32_t* pixels, int64_t n_pixels,
                                 int V, float* mean, float* m2, int32_t* count, stnerf_stream_t stream) {
    STNERF_REQUIRE(values && mean && m2 && count, "accumulate: null pointer");
    STNERF_REQUIRE(C >= 1 && C <= 4096 && V >= 1 && V <= C, "accumulate: bad widths C=%d V=%d (1 <= V <= C <= 4096)", C, V);
    STNERF_REQUIRE(value_stride >= C, "accumulate: row stride %lld < C = %d", (long long)value_stride, C);
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "accumulate: bad pixel count %lld", (long long)n_pixels);
    STNERF_REQUIRE(n >= 0 && n <= n_pixels, "accumulate: %lld rows for %lld pixels (a list names a pixel at most once)", (long long)n,
                   (long long)n_pixels);
    if (n == 0) return STNERF_OK;
    const int bs = 256;
    const int64_t tot = n * C;
    STNERF_REQUIRE((tot + bs - 1) / bs <= INT32_MAX, "accumulate: %lld rows of %d floats are more than one launch holds", (long long)n, C);
    hipLaunchKernelGGL(accumulate_kernel, dim3((unsigned)((tot + bs - 1) / bs)), dim3(bs), 0, as_stream(stream), values, n, C,
                       value_stride, pixels, n_pixels, V, mean, m2, (const int32_t*)count);
    STNERF_CHECK_LAUNCH("accumulate");
    hipLaunchKernelGGL(accumulate_count_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, as_stream(stream), n, pixels, n_pixels,
                       count);
    STNERF_CHECK_LAUNCH("accumulate (count)");
    return STNERF_OK;
}

extern "C" int64_t stnerf_accumulate_select_workspace_bytes(int64_t n_pixels) {
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "accumulate_select_workspace_bytes: bad pixel count %lld", (long long)n_pixels);
    return select_workspace_bytes(n_pixels);
}

extern "C" int stnerf_accumulate_select(const float* m2, const int32_t* count, int64_t n_pixels, int V, int min_spp, int max_spp,
                                        float tol2, int32_t* pixels_out, int32_t* n_out, void* workspace, int64_t workspace_bytes,
                                        stnerf_stream_t stream) {
    STNERF_REQUIRE(m2 && count && pixels_out && n_out && workspace, "accumulate_select: null pointer");
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "accumulate_select: bad pixel count %lld", (long long)n_pixels);
    STNERF_REQUIRE(V >= 1 && V <= 4096, "accumulate_select: bad V=%d", V);
    STNERF_REQUIRE(min_spp >= 1 && min_spp <= max_spp && max_spp <= 32768, "accumulate_select: bad spp range [%d, %d] (1 <= min <= max <= 32768)",
                   min_spp, max_spp);
    STNERF_REQUIRE(tol2 >= 0.f, "accumulate_select: tol2 must be >= 0");
    STNERF_REQUIRE(workspace_bytes >= stnerf_accumulate_select_workspace_bytes(n_pixels), "accumulate_select: workspace too small (%lld B, %lld needed)",
                   (long long)workspace_bytes, (long long)stnerf_accumulate_select_workspace_bytes(n_pixels));
    const PixelActive pred{m2, count, V, min_spp, max_spp, tol2};
    return ordered_compact(pred, n_pixels, reinterpret_cast<int32_t*>(workspace), pixels_out, n_out, as_stream(stream),
                           "accumulate_select (count)", "accumulate_select (scan)", "accumulate_select (write)");
}
