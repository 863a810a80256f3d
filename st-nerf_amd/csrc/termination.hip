// Early ray termination (include/stnerf.h: stnerf_ray_stop): the depth behind which the coarse pass shows a
// ray to be opaque (ray_stop_kernel).  The fine stage's row list without the samples behind it is stnerf_visibility_rows
// (csrc/sample_rows.hip).
// Compiled with -ffp-contract=off: the walk is one fp32 add and one fp32 subtraction per step.
#include <math.h>

#include "common.h"

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
