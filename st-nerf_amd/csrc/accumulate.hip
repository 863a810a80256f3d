// Progressive multi-sample frames (include/stnerf.h: stnerf_generate_rays_list, stnerf_accumulate, stnerf_accumulate_select;
// DESIGN.md section 7): a frame is the per-pixel mean of several passes, each with its own sub-pixel offset, shutter time and
// seed, and a pixel stops being sampled once its running mean is known well enough.  Three exact helper kernels around the
// render path, none of which touches a stage kernel: a ray generator over a pixel list, a Welford scatter-accumulator, and an
// ordered, deterministic compaction of the pixels that are still active.
// Compiled with -ffp-contract=off: every product, quotient and sum of the definitions is one fp32 operation.
#include "common.h"

namespace stnerf {

// ------------------------------------------------------------------------------------- rays of a pixel list
struct RayListArgs {
    float kinv[9];
    float T[16];
    float frame_ids[STNERF_MAX_LAYERS + 1];
};

// generate_rays_kernel (csrc/sampler.hip) with the pixel taken from a list and moved by (du, dv); every other operation in
// that kernel's order.  One lane per row; a list entry outside [0, h w) leaves its row unwritten.
__global__ void generate_rays_list_kernel(RayListArgs a, int w, int64_t n_pixels, const int32_t* __restrict__ pixels, int64_t n,
                                          float du, float dv, int n_frame_cols, float* __restrict__ rays, int ray_stride) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t pix = pixels ? (int64_t)pixels[i] : i;
    if (pix < 0 || pix >= n_pixels) return;
    const int p32 = (int)pix;               // (h w <= INT32_MAX: the host checks)
    const float u = (float)(p32 % w) + du;  // column
    const float v = (float)(p32 / w) + dv;  // row
    float cx = a.kinv[0] * u + a.kinv[1] * v + a.kinv[2];
    float cy = a.kinv[3] * u + a.kinv[4] * v + a.kinv[5];
    float cz = a.kinv[6] * u + a.kinv[7] * v + a.kinv[8];
    const float nrm = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));  // torch.norm's order (utils/render_helpers.py:108)
    cx = cx / nrm;
    cy = cy / nrm;
    cz = cz / nrm;
    float* r = rays + i * ray_stride;
    r[0] = a.T[3];
    r[1] = a.T[7];
    r[2] = a.T[11];
    r[3] = a.T[0] * cx + a.T[1] * cy + a.T[2] * cz;
    r[4] = a.T[4] * cx + a.T[5] * cy + a.T[6] * cz;
    r[5] = a.T[8] * cx + a.T[9] * cy + a.T[10] * cz;
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
constexpr int kSelectBlock = 256;   // pixels per workgroup of launches 1 and 3
constexpr int kScanBlock = 1024;    // workgroup popcounts per pass of launch 2

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

// Launch 1: block_count[b] = active pixels of [256 b, 256 b + 256).
__global__ void __launch_bounds__(kSelectBlock) select_count_kernel(const float* __restrict__ m2, const int32_t* __restrict__ count,
                                                                    int64_t P, int V, int min_spp, int max_spp, float tol2,
                                                                    int32_t* __restrict__ block_count) {
    __shared__ int wave_total[kSelectBlock / 64];
    const int64_t q = (int64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    const bool act = q < P && pixel_active(m2, count, q, V, min_spp, max_spp, tol2);
    const unsigned long long ball = __ballot(act);
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = __popcll(ball);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int i = 0; i < kSelectBlock / 64; ++i) tot += wave_total[i];
        block_count[blockIdx.x] = tot;
    }
}

// Launch 2: ONE workgroup turns the nb popcounts into exclusive offsets, in place, 1024 per pass with a running carry, and
// writes the total.  It waits on no other workgroup: there is none.
__global__ void __launch_bounds__(kScanBlock) select_scan_kernel(int32_t* __restrict__ block_count, int64_t nb, int32_t* __restrict__ total) {
    __shared__ int wave_sum[kScanBlock / 64];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += kScanBlock) {
        const int64_t b = base + threadIdx.x;
        const int v = b < nb ? block_count[b] : 0;
        int inc = v;  // inclusive scan of the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int before = carry_s;
        for (int i = 0; i < wave; ++i) before += wave_sum[i];
        if (b < nb) block_count[b] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == kScanBlock - 1) carry_s = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

// Launch 3: the predicate again, the pixel's place = its workgroup's offset + the waves before it + the lanes before it.
__global__ void __launch_bounds__(kSelectBlock) select_write_kernel(const float* __restrict__ m2, const int32_t* __restrict__ count,
                                                                    int64_t P, int V, int min_spp, int max_spp, float tol2,
                                                                    const int32_t* __restrict__ block_offset,
                                                                    int32_t* __restrict__ pixels_out) {
    __shared__ int wave_total[kSelectBlock / 64];
    const int64_t q = (int64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    const bool act = q < P && pixel_active(m2, count, q, V, min_spp, max_spp, tol2);
    const unsigned long long ball = __ballot(act);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_total[wave] = __popcll(ball);
    __syncthreads();
    if (!act) return;
    int at = block_offset[blockIdx.x];
    for (int i = 0; i < wave; ++i) at += wave_total[i];
    at += __popcll(ball & ((1ull << lane) - 1ull));
    pixels_out[at] = (int32_t)q;     // at < the total <= P: as many places as active pixels
}

static inline int64_t select_blocks(int64_t P) { return (P + kSelectBlock - 1) / kSelectBlock; }

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
    return (select_blocks(n_pixels) * (int64_t)sizeof(int32_t) + 255) / 256 * 256;
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
    const int64_t nb = select_blocks(n_pixels);
    int32_t* blocks = reinterpret_cast<int32_t*>(workspace);
    hipLaunchKernelGGL(select_count_kernel, dim3((unsigned)nb), dim3(kSelectBlock), 0, as_stream(stream), m2, count, n_pixels, V, min_spp,
                       max_spp, tol2, blocks);
    STNERF_CHECK_LAUNCH("accumulate_select (count)");
    hipLaunchKernelGGL(select_scan_kernel, dim3(1), dim3(kScanBlock), 0, as_stream(stream), blocks, nb, n_out);
    STNERF_CHECK_LAUNCH("accumulate_select (scan)");
    hipLaunchKernelGGL(select_write_kernel, dim3((unsigned)nb), dim3(kSelectBlock), 0, as_stream(stream), m2, count, n_pixels, V, min_spp,
                       max_spp, tol2, (const int32_t*)blocks, pixels_out);
    STNERF_CHECK_LAUNCH("accumulate_select (write)");
    return STNERF_OK;
}
