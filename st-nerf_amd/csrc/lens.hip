// A lens model in ray generation (include/stnerf.h: stnerf_lens, stnerf_generate_rays_lens): the rays of a
// pixel list through a lens that distorts (Brown-Conrady, inverted by a fixed number of fixed-point rounds) and has an aperture
// (thin lens: the ray starts at a point of the lens and passes through the pinhole ray's point on the plane in focus).  Both are
// properties of the camera; no stage kernel reads a ray, so nothing downstream changes.  One exact helper kernel.
// Compiled with -ffp-contract=off: every product, quotient, sum and difference of the definition is one fp32 operation.
//
// Per row, in this order (kinv = K^-1 row-major, T the 4x4 pose row-major):
//     pix = pixels[i] (or i); a pix outside [0, h w) leaves the row unwritten
//     u = (float)(pix % w) + du;  v = (float)(pix / w) + dv
//     c[r] = (kinv[3r] u + kinv[3r+1] v) + kinv[3r+2]                     r = 0, 1, 2  -> (cx, cy, cz)
//   distort != 0:
//     xd = cx / cz;  yd = cy / cz;  x = xd;  y = yd;  then STNERF_LENS_ITERS (20) rounds of
//         xx = x x;  yy = y y;  xy = x y;  r2 = xx + yy
//         rad = ((k3 r2 + k2) r2 + k1) r2 + 1
//         tx  = p1 (xy + xy) + p2 (r2 + (xx + xx))
//         ty  = p1 (r2 + (yy + yy)) + p2 (xy + xy)
//         x   = (xd - tx) / rad;  y = (yd - ty) / rad
//     cx = x cz;  cy = y cz                                               (cz is unchanged)
//   o[r] = T[4r+3]
//   points != NULL:
//     j = phase, or with decorrelate ((hash(pix ^ key) % n_points) + phase) % n_points in uint32, where
//         hash: x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
//     (ax, ay) = points[j];  unless ax == 0 && ay == 0 (the lens centre: the pinhole operations and nothing else):
//         s = focus / cz;  cx = cx s - ax;  cy = cy s - ay;  cz = cz s     (the old cz in all three)
//         o[r] = (T[4r] ax + T[4r+1] ay) + T[4r+3]
//   nrm = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx cx)));  c = c / nrm
//   d[r] = (T[4r] cx + T[4r+1] cy) + T[4r+2] cz;  the frame-id columns follow
// Without distortion and without a lens point the operations are those of generate_rays_list_kernel (csrc/accumulate.hip).
#include <cmath>

#include "common.h"

namespace stnerf {

struct LensRayArgs {
    float kinv[9];
    float T[16];
    float frame_ids[STNERF_MAX_LAYERS + 1];
    float k1, k2, k3, p1, p2;
    float focus;
    int32_t distort;
    int32_t n_points;
    int32_t phase;
    int32_t decorrelate;
    uint32_t key;
};

__device__ __forceinline__ uint32_t lens_hash(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// One lane per row, as generate_rays_list_kernel.  HBM-bound on the row it writes; the 20 rounds are about 400 flops per row.
// points holds n_points rows of two floats and j < n_points, so the one read of the table is inside it.
__global__ void __launch_bounds__(256) generate_rays_lens_kernel(LensRayArgs a, int w, int64_t n_pixels, const int32_t* __restrict__ pixels,
                                                                 int64_t n, float du, float dv, const float* __restrict__ points,
                                                                 int n_frame_cols, float* __restrict__ rays, int ray_stride) {
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
    if (a.distort) {
        const float xd = cx / cz;
        const float yd = cy / cz;
        float x = xd, y = yd;
#pragma unroll 1
        for (int it = 0; it < STNERF_LENS_ITERS; ++it) {
            const float xx = x * x;
            const float yy = y * y;
            const float xy = x * y;
            const float r2 = xx + yy;
            const float rad = ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2 + 1.0f;
            const float tx = a.p1 * (xy + xy) + a.p2 * (r2 + (xx + xx));
            const float ty = a.p1 * (r2 + (yy + yy)) + a.p2 * (xy + xy);
            x = (xd - tx) / rad;
            y = (yd - ty) / rad;
        }
        cx = x * cz;
        cy = y * cz;
    }
    float o0 = a.T[3], o1 = a.T[7], o2 = a.T[11];
    if (points) {
        uint32_t j = (uint32_t)a.phase;
        if (a.decorrelate) j = ((lens_hash((uint32_t)p32 ^ a.key) % (uint32_t)a.n_points) + (uint32_t)a.phase) % (uint32_t)a.n_points;
        const float ax = points[2 * (int64_t)j];
        const float ay = points[2 * (int64_t)j + 1];
        if (!(ax == 0.f && ay == 0.f)) {
            const float s = a.focus / cz;
            const float dx = cx * s - ax;
            const float dy = cy * s - ay;
            const float dz = cz * s;
            cx = dx;
            cy = dy;
            cz = dz;
            o0 = (a.T[0] * ax + a.T[1] * ay) + a.T[3];
            o1 = (a.T[4] * ax + a.T[5] * ay) + a.T[7];
            o2 = (a.T[8] * ax + a.T[9] * ay) + a.T[11];
        }
    }
    const float nrm = sqrtf(fmaf(cz, cz, fmaf(cy, cy, cx * cx)));  // torch.norm's order (utils/render_helpers.py:108)
    cx = cx / nrm;
    cy = cy / nrm;
    cz = cz / nrm;
    float* r = rays + i * ray_stride;
    r[0] = o0;
    r[1] = o1;
    r[2] = o2;
    r[3] = a.T[0] * cx + a.T[1] * cy + a.T[2] * cz;
    r[4] = a.T[4] * cx + a.T[5] * cy + a.T[6] * cz;
    r[5] = a.T[8] * cx + a.T[9] * cy + a.T[10] * cz;
    for (int c = 0; c < n_frame_cols; ++c) r[6 + c] = a.frame_ids[c];
}

}  // namespace stnerf

using namespace stnerf;

extern "C" int stnerf_generate_rays_lens(const float* Kinv_host, const float* T_host, int h, int w, const int32_t* pixels, int64_t n,
                                         float du, float dv, const stnerf_lens* lens_host, const float* frame_ids_host, int n_frame_cols,
                                         float* rays, int ray_stride, stnerf_stream_t stream) {
    if (lens_host) STNERF_REQUIRE(lens_host->struct_size == (int32_t)sizeof(stnerf_lens), "generate_rays_lens: struct_size %d, expected %d",
                                  (int)lens_host->struct_size, (int)sizeof(stnerf_lens));
    // no lens: the bits of stnerf_generate_rays_list, by being that call (its argument checks included)
    if (!lens_host || (!lens_host->distort && !lens_host->points))
        return stnerf_generate_rays_list(Kinv_host, T_host, h, w, pixels, n, du, dv, frame_ids_host, n_frame_cols, rays, ray_stride, stream);
    const stnerf_lens& L = *lens_host;
    STNERF_REQUIRE(Kinv_host && T_host && rays, "generate_rays_lens: null pointer");
    STNERF_REQUIRE(h > 0 && w > 0 && (int64_t)h * w <= INT32_MAX, "generate_rays_lens: bad view %dx%d", h, w);
    STNERF_REQUIRE(n >= 0 && n <= (int64_t)h * w, "generate_rays_lens: %lld rows for a %dx%d view (a list names a pixel at most once)",
                   (long long)n, h, w);
    STNERF_REQUIRE(du == du && dv == dv, "generate_rays_lens: the offset is NaN");
    STNERF_REQUIRE(n_frame_cols >= 0 && n_frame_cols <= STNERF_MAX_LAYERS + 1 && ray_stride >= 6 + n_frame_cols,
                   "generate_rays_lens: bad frame-id columns %d / stride %d", n_frame_cols, ray_stride);
    STNERF_REQUIRE(n_frame_cols == 0 || frame_ids_host, "generate_rays_lens: frame_ids is null");
    if (L.distort)
        STNERF_REQUIRE(std::isfinite(L.k1) && std::isfinite(L.k2) && std::isfinite(L.k3) && std::isfinite(L.p1) && std::isfinite(L.p2),
                       "generate_rays_lens: a distortion coefficient is NaN or infinite");
    const float k = Kinv_host[8];
    STNERF_REQUIRE(Kinv_host[6] == 0.f && Kinv_host[7] == 0.f && k != 0.f && std::isfinite(k),
                   "generate_rays_lens: the third row of K^-1 must be (0, 0, k) with k != 0 (one camera-space z for the view), got (%g, %g, %g)",
                   (double)Kinv_host[6], (double)Kinv_host[7], (double)k);
    if (L.points) {
        STNERF_REQUIRE(L.n_points >= 1, "generate_rays_lens: %d lens points", (int)L.n_points);
        STNERF_REQUIRE(L.phase >= 0 && L.phase < L.n_points, "generate_rays_lens: phase %d outside [0, %d)", (int)L.phase, (int)L.n_points);
        STNERF_REQUIRE(std::isfinite(L.focus) && L.focus != 0.f && (L.focus > 0.f) == (k > 0.f),
                       "generate_rays_lens: focus %g must be finite, non-zero and of the sign of K^-1's k = %g", (double)L.focus, (double)k);
    }
    if (n == 0) return STNERF_OK;
    LensRayArgs a;
    for (int i = 0; i < 9; ++i) a.kinv[i] = Kinv_host[i];
    for (int i = 0; i < 16; ++i) a.T[i] = T_host[i];
    for (int i = 0; i < STNERF_MAX_LAYERS + 1; ++i) a.frame_ids[i] = i < n_frame_cols ? frame_ids_host[i] : 0.f;
    a.distort = L.distort ? 1 : 0;
    a.k1 = L.distort ? L.k1 : 0.f;
    a.k2 = L.distort ? L.k2 : 0.f;
    a.k3 = L.distort ? L.k3 : 0.f;
    a.p1 = L.distort ? L.p1 : 0.f;
    a.p2 = L.distort ? L.p2 : 0.f;
    a.focus = L.points ? L.focus : 0.f;
    a.n_points = L.points ? L.n_points : 1;
    a.phase = L.points ? L.phase : 0;
    a.decorrelate = L.points && L.decorrelate ? 1 : 0;
    a.key = L.key;
    const int bs = 256;
    hipLaunchKernelGGL(generate_rays_lens_kernel, dim3((unsigned)((n + bs - 1) / bs)), dim3(bs), 0, as_stream(stream), a, w,
                       (int64_t)h * w, pixels, n, du, dv, L.points, n_frame_cols, rays, ray_stride);
    STNERF_CHECK_LAUNCH("generate_rays_lens");
    return STNERF_OK;
}
