// Grid proposals (include/stnerf.h: stnerf_density_grid): a layer's coarse densities by a trilinear lookup in a
// grid of vertex densities, in place of its coarse SpaceNet and MotionNet.  The lookup rule is stated once, in the header; the device
// function below is that rule, an fp32 operation per line.  Also the host checks of a grid, for the entry and for the render call.
// Compiled with -ffp-contract=off: every product and sum of the rule is a separate fp32 operation.
#include <math.h>

#include <algorithm>

#include "common.h"

using namespace stnerf;

namespace {

// One grid by value (wave-uniform -> SGPRs).
struct DensityGrid {
    const float* sigma;
    int32_t rx, ry, rz;
    float lo[3], inv[3];
};

// the cell index, the fraction and its complement of one axis
__device__ __forceinline__ void axis_of(float p, float lo, float inv, int r, int& i, float& f, float& u) {
    const float d = p - lo;
    const float g = d * inv;
    const float gc = fminf(fmaxf(g, 0.f), (float)r);
    i = (int)fminf(floorf(gc), (float)(r - 1));
    f = gc - (float)i;
    u = 1.f - f;
}

__device__ __forceinline__ float lerp2(float v0, float u, float v1, float f) {
    const float a = v0 * u;
    const float b = v1 * f;
    return a + b;
}

__device__ __forceinline__ float lookup(const DensityGrid& g, float x, float y, float z) {
    int ix, iy, iz;
    float fx, fy, fz, ux, uy, uz;
    axis_of(x, g.lo[0], g.inv[0], g.rx, ix, fx, ux);
    axis_of(y, g.lo[1], g.inv[1], g.ry, iy, fy, uy);
    axis_of(z, g.lo[2], g.inv[2], g.rz, iz, fz, uz);
    const int sx = g.rx + 1, sxy = sx * (g.ry + 1);
    const float* v = g.sigma + ((int64_t)iz * sxy + (int64_t)iy * sx + ix);   // (ix, iy, iz) <= R - 1: all eight vertices exist
    const float v000 = v[0], v100 = v[1], v010 = v[sx], v110 = v[sx + 1];
    const float v001 = v[sxy], v101 = v[sxy + 1], v011 = v[sxy + sx], v111 = v[sxy + sx + 1];
    const float c00 = lerp2(v000, ux, v100, fx);
    const float c10 = lerp2(v010, ux, v110, fx);
    const float c01 = lerp2(v001, ux, v101, fx);
    const float c11 = lerp2(v011, ux, v111, fx);
    const float c0 = lerp2(c00, uy, c10, fy);
    const float c1 = lerp2(c01, uy, c11, fy);
    const float s = lerp2(c0, uz, c1, fz);
    // (fmaxf drops a NaN: the coordinate's is carried in here)
    return (x != x || y != y || z != z) ? __int_as_float(0x7fc00000) : s;
}

// One wave per listed ray at a time over a persistent grid: lanes take the ray's samples k = lane, lane + 64, ...
__global__ void __launch_bounds__(256) proposal_density_kernel(const int32_t* __restrict__ ray_list, const int32_t* __restrict__ ray_count, int64_t n,
                                                               const float* __restrict__ xyz, int64_t xyz_ray_stride, int ns, DensityGrid g,
                                                               float* __restrict__ raw, int64_t raw_ray_stride) {
    const int lane = threadIdx.x & 63;
    const int64_t waves = (int64_t)gridDim.x * 4;
    int64_t cnt = n;
    if (ray_list) {
        const int64_t c = *ray_count;
        cnt = c < 0 ? 0 : (c < n ? c : n);
    }
    for (int64_t slot = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); slot < cnt; slot += waves) {
        const int64_t ray = ray_list ? (int64_t)ray_list[slot] : slot;
        if (ray < 0 || ray >= n) continue;   // (a list entry outside the call's rays writes nothing)
        const float* p = xyz + ray * xyz_ray_stride;
        float4* out = reinterpret_cast<float4*>(raw + ray * raw_ray_stride);
        for (int k = lane; k < ns; k += 64) {
            const float s = lookup(g, p[3 * k], p[3 * k + 1], p[3 * k + 2]);
            out[k] = make_float4(0.f, 0.f, 0.f, s);
        }
    }
}

// as occupancy_cull's: every wave slot of the device
constexpr int64_t PROPOSAL_MAX_BLOCKS = 2048;

}  // namespace

namespace stnerf {
int check_density_grid(const stnerf_density_grid* g, int layer, const char* what) {
    STNERF_REQUIRE(g && g->sigma, "%s: density grid of layer %d has no sigma", what, layer);
    STNERF_REQUIRE(((uintptr_t)g->sigma & 3) == 0, "%s: density grid of layer %d: sigma must be 4-byte aligned", what, layer);
    STNERF_REQUIRE(g->res[0] >= 1 && g->res[1] >= 1 && g->res[2] >= 1, "%s: density grid of layer %d has res (%d, %d, %d), each must be >= 1", what, layer,
                   g->res[0], g->res[1], g->res[2]);
    // (each factor <= 2^31: the product of two fits 63 bits, and is tested before the third goes in)
    const int64_t xy = ((int64_t)g->res[0] + 1) * ((int64_t)g->res[1] + 1);
    STNERF_REQUIRE(xy < ((int64_t)1 << 31) && xy * ((int64_t)g->res[2] + 1) < ((int64_t)1 << 31),
                   "%s: density grid of layer %d has res (%d, %d, %d): 2^31 vertices or more", what, layer, g->res[0], g->res[1], g->res[2]);
    for (int a = 0; a < 3; ++a)
        STNERF_REQUIRE(isfinite(g->lo[a]) && isfinite(g->inv_cell[a]), "%s: density grid of layer %d: lo[%d] = %g / inv_cell[%d] = %g is not finite", what,
                       layer, a, (double)g->lo[a], a, (double)g->inv_cell[a]);
    return STNERF_OK;
}
}  // namespace stnerf

extern "C" int stnerf_proposal_density(const int32_t* ray_list, const int32_t* ray_count, int64_t n, int layer, const float* xyz,
                                       int64_t xyz_ray_stride, int ns, const stnerf_density_grid* grid_host, float* raw, int64_t raw_ray_stride,
                                       stnerf_stream_t stream) {
    STNERF_REQUIRE(xyz && raw && grid_host, "proposal_density: null pointer");
    STNERF_REQUIRE(!ray_list || ray_count, "proposal_density: a ray list needs its count (ray_list == NULL means every ray)");
    STNERF_REQUIRE(layer >= 0 && layer < STNERF_MAX_LAYERS, "proposal_density: layer %d outside 0..%d", layer, STNERF_MAX_LAYERS - 1);
    STNERF_REQUIRE(ns >= 1 && ns <= 256, "proposal_density: ns = %d outside 1..256", ns);
    STNERF_REQUIRE(n >= 0 && xyz_ray_stride >= 0 && raw_ray_stride >= 0, "proposal_density: bad shape");
    STNERF_REQUIRE((((uintptr_t)ray_list | (uintptr_t)ray_count | (uintptr_t)xyz) & 3) == 0, "proposal_density: ray_list, ray_count and xyz must be 4-byte aligned");
    STNERF_REQUIRE(((uintptr_t)raw & 15) == 0 && (raw_ray_stride & 3) == 0, "proposal_density: raw must be 16-byte aligned, its stride a multiple of 4 floats");
    const int rc = check_density_grid(grid_host, layer, "proposal_density");
    if (rc) return rc;
    if (n == 0) return STNERF_OK;
    const DensityGrid g{grid_host->sigma, grid_host->res[0], grid_host->res[1], grid_host->res[2],
                        {grid_host->lo[0], grid_host->lo[1], grid_host->lo[2]}, {grid_host->inv_cell[0], grid_host->inv_cell[1], grid_host->inv_cell[2]}};
    hipStream_t st = as_stream(stream);
    set_launch_tag(layer);
    {
        // per ray: ns points read, ns float4 written, and up to 8 vertices of 4 bytes gathered per sample
        LaunchTimer timer(PROF_PROPOSAL_DENSITY, 0, n, ns, (12 + 16 + 32) * (int64_t)ns, st);
        hipLaunchKernelGGL(proposal_density_kernel, dim3((unsigned)std::min<int64_t>((n + 3) / 4, PROPOSAL_MAX_BLOCKS)), dim3(256), 0, st, ray_list, ray_count, n,
                           xyz, xyz_ray_stride, ns, g, raw, raw_ray_stride);
    }
    set_launch_tag(-1);
    STNERF_CHECK_LAUNCH("proposal_density");
    return STNERF_OK;
}
