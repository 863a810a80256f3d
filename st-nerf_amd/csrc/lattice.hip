// Adaptive lattice frames (include/stnerf.h: stnerf_lattice_begin, stnerf_lattice_classify, stnerf_lattice_select,
// stnerf_lattice_scatter): a frame is rendered on a sparse lattice of pixels, the cells whose corners
// disagree are refined at half the stride, and the pixels of the cells whose corners agree are interpolated.  Exact helper
// kernels around the render path, none of which touches a stage kernel: the first queue, the flat test of a cell, the fill of
// the pixels every cell around them is flat, their status, the ordered compaction of the queued pixels, and the scatter of
// the rendered rows.  All HBM-bound; no LDS beyond the compaction's few words, no scratch, no atomics.
// Compiled with -ffp-contract=off: every product, difference and sum of the definitions is one fp32 operation.
#include "common.h"
#include "ordered_compact.h"

namespace stnerf {

constexpr uint8_t kUnknown = 0, kRendered = 1, kFilled = 2, kQueued = 3;

// The covered region of include/stnerf.h: x <= Wc and y <= Hc, or no pixel at all (cells == false).
struct Covered {
    int Wc, Hc;
    bool cells;
};
static inline Covered covered_region(int h, int w, int S) {
    Covered c;
    c.Wc = (w - 1) / S * S;
    c.Hc = (h - 1) / S * S;
    c.cells = c.Wc > 0 && c.Hc > 0;
    return c;
}

// ------------------------------------------------------------------------------------- the first queue
// One lane per pixel: the margin, the forced pixels and the points of the top lattice are queued, every other pixel unknown.
__global__ void __launch_bounds__(256) lattice_begin_kernel(int w, int64_t P, int S, int Wc, int Hc, int cells,
                                                            const uint8_t* __restrict__ force, uint8_t* __restrict__ status) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= P) return;
    const int y = (int)(q / w);
    const int x = (int)(q - (int64_t)y * w);
    const bool margin = !cells || x > Wc || y > Hc;
    const bool forced = force && force[q] != 0;
    const bool point = x % S == 0 && y % S == 0;
    status[q] = margin || forced || point ? kQueued : kUnknown;
}

// ------------------------------------------------------------------------------------- flat cells
// One lane per cell (cx, cy, s) of the covered region, cell i = (cy / s) * ncx + cx / s: flat[i] = 1 if and only if every tested
// column's four corner values are finite with max - min <= tol[c] (ONE subtraction), and every exact column's compare equal.
__global__ void __launch_bounds__(256) lattice_flat_kernel(const float* __restrict__ values, int w, int C, int T, int s, int ncx,
                                                           int64_t ncells, const float* __restrict__ tol, uint8_t* __restrict__ flat) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= ncells) return;
    const int64_t cyi = i / ncx;
    const int64_t cxi = i - cyi * ncx;
    const int64_t q00 = cyi * s * w + cxi * s;
    const float* v00 = values + q00 * C;
    const float* v10 = v00 + (int64_t)s * C;
    const float* v01 = v00 + (int64_t)s * w * C;
    const float* v11 = v01 + (int64_t)s * C;
    bool ok = true;
    for (int c = 0; c < C; ++c) {
        const float a = v00[c], b = v10[c], d = v01[c], e = v11[c];
        if (c < T) {
            const bool finite = isfinite(a) && isfinite(b) && isfinite(d) && isfinite(e);
            const float hi = fmaxf(fmaxf(a, b), fmaxf(d, e));
            const float lo = fminf(fminf(a, b), fminf(d, e));
            const float spread = hi - lo;
            ok = ok && finite && spread <= tol[c];
        } else {
            ok = ok && a == b && a == d && a == e;
        }
    }
    flat[i] = ok ? 1 : 0;
}

// The cells of stride s whose closure contains (x, y), clipped to the covered region: one for an interior pixel, two on an
// edge.  -> all of them flat; (cx, cy) = the first, lowest cy then lowest cx.
__device__ __forceinline__ bool cells_around_flat(int x, int y, int s, int Wc, int Hc, int ncx, const uint8_t* __restrict__ flat,
                                                  int& cx, int& cy) {
    const int x0 = x / s * s, y0 = y / s * s;
    const int xlo = x == x0 ? x0 - s : x0;
    const int ylo = y == y0 ? y0 - s : y0;
    bool all = true, none = true;
    for (int yc = ylo; yc <= y0; yc += s) {
        for (int xc = xlo; xc <= x0; xc += s) {
            if (xc < 0 || yc < 0 || xc + s > Wc || yc + s > Hc) continue;
            all = all && flat[(int64_t)(yc / s) * ncx + xc / s] != 0;
            if (none) {
                cx = xc;
                cy = yc;
                none = false;
            }
        }
    }
    return all && !none;
}

// ------------------------------------------------------------------------------------- the fill
// One lane per (covered pixel, column): consecutive lanes write consecutive floats.  Reads the status (which the next launch
// writes) and the values of lattice-s points, whose status is 1 or 2 and which no lane owns; writes only its own pixel's column.
__global__ void __launch_bounds__(256) lattice_fill_kernel(float* __restrict__ values, const uint8_t* __restrict__ status, int w, int C,
                                                           int T, int s, float inv_s, int Wc, int Hc, int ncx, int64_t n_lanes,
                                                           const uint8_t* __restrict__ flat) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n_lanes) return;
    const int64_t pc = e / C;
    const int col = (int)(e - pc * C);
    const int y = (int)(pc / (Wc + 1));
    const int x = (int)(pc - (int64_t)y * (Wc + 1));
    const int64_t q = (int64_t)y * w + x;
    if (status[q] != kUnknown) return;
    int cx = 0, cy = 0;
    if (!cells_around_flat(x, y, s, Wc, Hc, ncx, flat, cx, cy)) return;
    const int64_t q00 = (int64_t)cy * w + cx;
    const float v00 = values[q00 * C + col];
    if (col >= T) {  // an exact column copies v00
        values[q * C + col] = v00;
        return;
    }
    const float v10 = values[(q00 + s) * C + col];
    const float v01 = values[(q00 + (int64_t)s * w) * C + col];
    const float v11 = values[(q00 + (int64_t)s * w + s) * C + col];
    const float fx = (float)(x - cx) * inv_s;  // (x - cx) / s: exact, s is a power of two
    const float fy = (float)(y - cy) * inv_s;
    const float gx = 1.f - fx;
    const float gy = 1.f - fy;
    const float t0 = gx * v00;
    const float t1 = fx * v10;
    const float top = t0 + t1;
    const float b0 = gx * v01;
    const float b1 = fx * v11;
    const float bot = b0 + b1;
    const float r0 = gy * top;
    const float r1 = fy * bot;
    values[q * C + col] = r0 + r1;
}

// One lane per covered pixel, after the fill: an unknown pixel becomes filled (every cell around it flat), queued (a point of
// the next lattice, stride s / 2) or stays unknown.  Reads lattice-s flat bytes only; writes only its own status.
__global__ void __launch_bounds__(256) lattice_mark_kernel(uint8_t* __restrict__ status, int w, int s, int Wc, int Hc, int ncx,
                                                           int64_t n_covered, const uint8_t* __restrict__ flat) {
    const int64_t pc = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pc >= n_covered) return;
    const int y = (int)(pc / (Wc + 1));
    const int x = (int)(pc - (int64_t)y * (Wc + 1));
    const int64_t q = (int64_t)y * w + x;
    if (status[q] != kUnknown) return;
    int cx = 0, cy = 0;
    const int half = s / 2;
    if (cells_around_flat(x, y, s, Wc, Hc, ncx, flat, cx, cy))
        status[q] = kFilled;
    else if (x % half == 0 && y % half == 0)
        status[q] = kQueued;
}

// ------------------------------------------------------------------------------------- the rendered rows
// One lane per (row, column), as accumulate_kernel; column 0's lane marks the pixel rendered (no lane reads a status here).  A
// pixel outside [0, P) is skipped.
__global__ void __launch_bounds__(256) lattice_scatter_kernel(const float* __restrict__ rows, int64_t n, int C, int64_t row_stride,
                                                              const int32_t* __restrict__ pixels, int64_t P, float* __restrict__ values,
                                                              uint8_t* __restrict__ status) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= n * C) return;
    const int64_t i = e / C;
    const int col = (int)(e - i * C);
    const int64_t q = (int64_t)pixels[i];
    if (q < 0 || q >= P) return;
    values[q * C + col] = rows[i * row_stride + col];
    if (col == 0) status[q] = kRendered;
}

// ------------------------------------------------------------------------------------- the queued pixels
// (the three launches of the ordered compaction: csrc/ordered_compact.h)
struct PixelQueued {
    const uint8_t* status;
    __device__ __forceinline__ bool operator()(int64_t q) const { return status[q] == kQueued; }
};

static inline unsigned blocks_of(int64_t lanes) { return (unsigned)((lanes + 255) / 256); }

}  // namespace stnerf

using namespace stnerf;

#define STNERF_REQUIRE_VIEW(what, h, w) \
    STNERF_REQUIRE((h) > 0 && (w) > 0 && (int64_t)(h) * (w) <= INT32_MAX, what ": bad view %dx%d", (h), (w))
#define STNERF_REQUIRE_LEVELS(what, levels) STNERF_REQUIRE((levels) >= 0 && (levels) <= 4, what ": levels = %d outside 0..4", (levels))
#define STNERF_REQUIRE_WIDTHS(what, C, E) \
    STNERF_REQUIRE((C) >= 1 && (C) <= 4096 && (E) >= 0 && (E) <= (C), what ": bad widths C=%d E=%d (0 <= E <= C, 1 <= C <= 4096)", (C), (E))

extern "C" int stnerf_lattice_begin(int h, int w, int levels, const uint8_t* force, uint8_t* status, stnerf_stream_t stream) {
    STNERF_REQUIRE(status, "lattice_begin: null pointer");
    STNERF_REQUIRE_VIEW("lattice_begin", h, w);
    STNERF_REQUIRE_LEVELS("lattice_begin", levels);
    const int S = 1 << levels;
    const Covered cov = covered_region(h, w, S);
    const int64_t P = (int64_t)h * w;
    hipLaunchKernelGGL(lattice_begin_kernel, dim3(blocks_of(P)), dim3(256), 0, as_stream(stream), w, P, S, cov.Wc, cov.Hc,
                       (int)cov.cells, force, status);
    STNERF_CHECK_LAUNCH("lattice_begin");
    return STNERF_OK;
}

extern "C" int stnerf_lattice_classify(float* values, uint8_t* status, int h, int w, int C, int E, int levels, int s, const float* tol,
                                       uint8_t* flat, int64_t flat_bytes, stnerf_stream_t stream) {
    STNERF_REQUIRE(values && status && flat, "lattice_classify: null pointer");
    STNERF_REQUIRE_VIEW("lattice_classify", h, w);
    STNERF_REQUIRE_LEVELS("lattice_classify", levels);
    STNERF_REQUIRE_WIDTHS("lattice_classify", C, E);
    STNERF_REQUIRE(tol || C == E, "lattice_classify: tol is null");
    const int S = 1 << levels;
    STNERF_REQUIRE(s >= 2 && s <= S && (s & (s - 1)) == 0, "lattice_classify: stride %d is not a power of two in [2, %d]", s, S);
    const Covered cov = covered_region(h, w, S);
    if (!cov.cells) return STNERF_OK;  // every pixel is margin
    const int ncx = cov.Wc / s;
    const int64_t ncells = (int64_t)ncx * (cov.Hc / s);
    STNERF_REQUIRE(flat_bytes >= ncells, "lattice_classify: flat bytes too few (%lld B, %lld cells of stride %d)", (long long)flat_bytes,
                   (long long)ncells, s);
    const int64_t n_covered = (int64_t)(cov.Wc + 1) * (cov.Hc + 1);
    const int64_t n_lanes = n_covered * C;
    STNERF_REQUIRE((n_lanes + 255) / 256 <= INT32_MAX, "lattice_classify: %lld pixels of %d floats are more than one launch holds",
                   (long long)n_covered, C);
    const int T = C - E;
    hipLaunchKernelGGL(lattice_flat_kernel, dim3(blocks_of(ncells)), dim3(256), 0, as_stream(stream), (const float*)values, w, C, T, s,
                       ncx, ncells, tol, flat);
    STNERF_CHECK_LAUNCH("lattice_classify (flat)");
    hipLaunchKernelGGL(lattice_fill_kernel, dim3(blocks_of(n_lanes)), dim3(256), 0, as_stream(stream), values, (const uint8_t*)status,
                       w, C, T, s, 1.f / (float)s, cov.Wc, cov.Hc, ncx, n_lanes, (const uint8_t*)flat);
    STNERF_CHECK_LAUNCH("lattice_classify (fill)");
    hipLaunchKernelGGL(lattice_mark_kernel, dim3(blocks_of(n_covered)), dim3(256), 0, as_stream(stream), status, w, s, cov.Wc, cov.Hc,
                       ncx, n_covered, (const uint8_t*)flat);
    STNERF_CHECK_LAUNCH("lattice_classify (mark)");
    return STNERF_OK;
}

extern "C" int64_t stnerf_lattice_select_workspace_bytes(int64_t n_pixels) {
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "lattice_select_workspace_bytes: bad pixel count %lld", (long long)n_pixels);
    return select_workspace_bytes(n_pixels);
}

extern "C" int stnerf_lattice_select(const uint8_t* status, int64_t n_pixels, int32_t* pixels_out, int32_t* n_out, void* workspace,
                                     int64_t workspace_bytes, stnerf_stream_t stream) {
    STNERF_REQUIRE(status && pixels_out && n_out && workspace, "lattice_select: null pointer");
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "lattice_select: bad pixel count %lld", (long long)n_pixels);
    STNERF_REQUIRE(workspace_bytes >= stnerf_lattice_select_workspace_bytes(n_pixels), "lattice_select: workspace too small (%lld B, %lld needed)",
                   (long long)workspace_bytes, (long long)stnerf_lattice_select_workspace_bytes(n_pixels));
    const PixelQueued pred{status};
    return ordered_compact(pred, n_pixels, reinterpret_cast<int32_t*>(workspace), pixels_out, n_out, as_stream(stream),
                           "lattice_select (count)", "lattice_select (scan)", "lattice_select (write)");
}

extern "C" int stnerf_lattice_scatter(const float* rows, int64_t n, int C, int64_t row_stride, const int32_t* pixels, int64_t n_pixels,
                                      float* values, uint8_t* status, stnerf_stream_t stream) {
    STNERF_REQUIRE(values && status && (n == 0 || (rows && pixels)), "lattice_scatter: null pointer");
    STNERF_REQUIRE(C >= 1 && C <= 4096, "lattice_scatter: bad width C=%d (1 <= C <= 4096)", C);
    STNERF_REQUIRE(row_stride >= C, "lattice_scatter: row stride %lld < C = %d", (long long)row_stride, C);
    STNERF_REQUIRE(n_pixels >= 1 && n_pixels <= INT32_MAX, "lattice_scatter: bad pixel count %lld", (long long)n_pixels);
    STNERF_REQUIRE(n >= 0 && n <= n_pixels, "lattice_scatter: %lld rows for %lld pixels (a list names a pixel at most once)", (long long)n,
                   (long long)n_pixels);
    if (n == 0) return STNERF_OK;
    const int64_t tot = n * C;
    STNERF_REQUIRE((tot + 255) / 256 <= INT32_MAX, "lattice_scatter: %lld rows of %d floats are more than one launch holds", (long long)n, C);
    hipLaunchKernelGGL(lattice_scatter_kernel, dim3(blocks_of(tot)), dim3(256), 0, as_stream(stream), rows, n, C, row_stride, pixels,
                       n_pixels, values, status);
    STNERF_CHECK_LAUNCH("lattice_scatter");
    return STNERF_OK;
}
