// Depth-tested occluder compositing (include/stnerf.h: stnerf_scene_occluder, stnerf_occluder_stop; DESIGN.md sections 4.2 and 7):
// an external element {r, g, b, a, z} per ray -- a prop, a title card, a plate with a z-buffer -- put INTO the scene.  The final
// stage's merged weights are split at z per ray and per layer (scene_occluder_kernel: layer_scene_kernel's sums, twice), the mix
// follows on five lanes of the ray's wave; an opaque row is also a stop depth for early ray termination (occluder_stop_kernel).
// Compiled with -ffp-contract=off: every product and every sum of the definitions is one fp32 operation.
#include <math.h>

#include "common.h"
#include "composite_rules.h"
#include "wave_prims.h"

namespace stnerf {

// One occluder row: a' = a clamped to [0, 1] (a NaN counts as 0); present = a' > 0 and z finite.
__device__ __forceinline__ bool occluder_row(float a, float z, float& ap) {
    ap = a > 0.f ? a : 0.f;
    ap = ap < 1.f ? ap : 1.f;
    return ap > 0.f && fabsf(z) < INFINITY;
}

struct SceneOccluderArgs {
    const float* t;
    const float4* raw;
    const uint8_t* mask;
    const float* merged_weights;
    int64_t n;
    int l, S;
    stnerf_composite_params p;
    const float* scene_in;
    const float* mixed_in;
    const float* occluder;
    float* occluded_mixed;
    float* occluded_scene;
    float* occluder_share;
    float* front_out;
    float* behind_out;
};

// lane c < 5: channel c of five wave-uniform totals
__device__ __forceinline__ float pick5(const float (&v)[5], unsigned lane) {
    return lane == 0u ? v[0] : lane == 1u ? v[1] : lane == 2u ? v[2] : lane == 3u ? v[3] : v[4];
}

// One wave per ray over a persistent grid; HBM-bound, layer_scene_kernel's 4 + 4 + 16 B per sample on a present ray, 20 B per
// layer on an absent one.  The sums are layer_scene_kernel's with the weight replaced by +0 on the side a sample is not on, so
// that a z beyond (below) every depth reproduces scene_out bit for bit in front (behind).  The mix needs no table of the layers'
// totals: pass_i depends on layer i alone and is summed as it appears, Af likewise; only the occluder's share waits for the
// last layer.  Lanes 0..4 hold the channels {r, g, b, depth, acc}.
__global__ void __launch_bounds__(256) scene_occluder_kernel(SceneOccluderArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t first = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t LS = (int64_t)a.l * a.S;
    const int L5 = a.l * 5;
    const EvalBits ev = eval_bits<false>(a.p, a.l);
    const bool activated = a.p.rgb_activated != 0;
    for (int64_t ray = first; ray < a.n; ray += stride) {
        // the row, read once: lanes 0..4 keep their own channel, a and z become wave-uniform
        const float ov = lane < 5u ? a.occluder[ray * 5 + lane] : 0.f;
        const float oa = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ov), 3));
        const float oz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(ov), 4));
        float ap;
        if (!occluder_row(oa, oz, ap)) {   // (uniform) absent: the plain outputs, no sample is loaded
            for (int j = (int)lane; j < L5; j += 64) {
                const float v = a.scene_in[ray * L5 + j];
                if (a.occluded_scene) a.occluded_scene[ray * L5 + j] = v;
                if (a.front_out) a.front_out[ray * L5 + j] = v;
                if (a.behind_out) a.behind_out[ray * L5 + j] = 0.f;
            }
            if (lane < 5u) {
                a.occluded_mixed[ray * 5 + lane] = a.mixed_in[ray * 5 + lane];
                if (a.occluder_share) a.occluder_share[ray * 5 + lane] = 0.f;
            }
            continue;
        }
        const int mv = (a.mask && (int)lane < a.l) ? (int)a.mask[ray * a.l + lane] : 0;
        const unsigned have_m = have_layers(ev, a.mask != nullptr, (unsigned)__ballot((mv & 1) != 0));
        const float q = 1.f - ap;
        const float ox = lane < 3u ? ov : lane == 3u ? oz : 1.f;   // this lane's channel of {r, g, b, z, 1}
        float sum = 0.f, af = 0.f;   // (pass_0 + pass_1) + ... of this lane's channel; (front[0][4] + front[1][4]) + ...
        for (int layer = 0; layer < a.l; ++layer) {
            float F[5] = {0.f, 0.f, 0.f, 0.f, 0.f}, B[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            if (have_m >> layer & 1u) {   // (uniform; a layer without output: five exact zeros on both sides)
                const float* tl = a.t + ray * LS + (int64_t)layer * a.S;
                const float* wl = a.merged_weights + ray * LS + (int64_t)layer * a.S;
                const float4* rl = a.raw + ray * LS + (int64_t)layer * a.S;
                CompositeAcc FA, BA;
                // every load of the layer (three blocks at a time) is issued before the first one is consumed
                constexpr int SB = 3;
                for (int k0 = 0; k0 < a.S; k0 += 64 * SB) {
                    float tv[SB], wv[SB];
                    float4 rv[SB];
#pragma unroll
                    for (int b = 0; b < SB; ++b) {
                        const int k = k0 + b * 64 + (int)lane;
                        tv[b] = wv[b] = 0.f;
                        rv[b] = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (k < a.S) {
                            wv[b] = wl[k];
                            tv[b] = tl[k];
                            rv[b] = rl[k];
                        }
                    }
#pragma unroll
                    for (int b = 0; b < SB; ++b) {
                        if (k0 + b * 64 + (int)lane < a.S) {
                            const float4 c = edit_sample(rv[b], tv[b], false, -INFINITY, 1.f, false, 0.f, activated);
                            const bool behind = tv[b] >= oz;   // (a NaN depth is in front)
                            const float wf = behind ? 0.f : wv[b], wb = behind ? wv[b] : 0.f;
                            FA.cr += wf * c.x;
                            FA.cg += wf * c.y;
                            FA.cb += wf * c.z;
                            FA.cd += wf * tv[b];
                            FA.ca += wf;
                            BA.cr += wb * c.x;
                            BA.cg += wb * c.y;
                            BA.cb += wb * c.z;
                            BA.cd += wb * tv[b];
                            BA.ca += wb;
                        }
                    }
                }
                composite_total5(FA, F);
                composite_total5(BA, B);
            }
            const float f = pick5(F, lane), bh = pick5(B, lane);
            const float pass = f + q * bh;
            sum = layer == 0 ? pass : sum + pass;
            af = layer == 0 ? F[4] : af + F[4];
            if (lane < 5u) {
                const int64_t at = (ray * a.l + layer) * 5 + lane;
                if (a.occluded_scene) a.occluded_scene[at] = pass;
                if (a.front_out) a.front_out[at] = f;
                if (a.behind_out) a.behind_out[at] = bh;
            }
        }
        const float left = 1.f - af;
        const float T = left > 0.f ? left : 0.f;   // (a NaN leaves nothing)
        const float s = ap * T;
        const float share = s * ox;
        if (lane < 5u) {
            a.occluded_mixed[ray * 5 + lane] = sum + share;
            if (a.occluder_share) a.occluder_share[ray * 5 + lane] = share;
        }
    }
}

// One lane per ray: an opaque present row in front of the ray's stop depth becomes the stop depth.
__global__ void __launch_bounds__(256) occluder_stop_kernel(const float* __restrict__ occluder, int64_t n, float* __restrict__ t_stop) {
    const int64_t ray = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (ray >= n) return;
    const float z = occluder[ray * 5 + 4];
    float ap;
    if (occluder_row(occluder[ray * 5 + 3], z, ap) && ap >= 1.f && z < t_stop[ray]) t_stop[ray] = z;
}

}  // namespace stnerf

using namespace stnerf;

extern "C" int stnerf_scene_occluder(const float* t, const float* raw, const uint8_t* mask, const float* merged_weights, int64_t n, int l,
                                     int S, const stnerf_composite_params* params_host, const float* scene_in, const float* mixed_in,
                                     const float* occluder, float* occluded_mixed, float* occluded_scene, float* occluder_share,
                                     float* front_out, float* behind_out, stnerf_stream_t stream) {
    STNERF_REQUIRE(t && raw && merged_weights && params_host && scene_in && mixed_in && occluder, "scene_occluder: null pointer");
    STNERF_REQUIRE(occluded_mixed, "scene_occluder: occluded_mixed is required");
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && S >= 1, "scene_occluder: bad shape n=%lld l=%d S=%d", (long long)n, l, S);
    STNERF_REQUIRE((int64_t)l * S <= 65535, "scene_occluder: more than 65535 samples per ray");
    STNERF_REQUIRE(((uintptr_t)raw & 15) == 0, "scene_occluder: raw must be 16-byte aligned");
    if (n == 0) return STNERF_OK;
    hipStream_t st = as_stream(stream);
    SceneOccluderArgs a{t, reinterpret_cast<const float4*>(raw), mask, merged_weights, n, l, S, *params_host, scene_in, mixed_in,
                        occluder, occluded_mixed, occluded_scene, occluder_share, front_out, behind_out};
    int64_t blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    {
        // per present ray: the samples read as the scene pass reads them, the row, and 20 B per output it writes
        LaunchTimer timer(PROF_SCENE_OCCLUDER, 0, n, S,
                          24ll * l * S + l + 20 + 20ll * (2 + (occluded_scene ? l : 0) + (front_out ? l : 0) + (behind_out ? l : 0)), st);
        hipLaunchKernelGGL(scene_occluder_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a);
    }
    STNERF_CHECK_LAUNCH("scene_occluder");
    return STNERF_OK;
}

extern "C" int stnerf_occluder_stop(const float* occluder, int64_t n, float* t_stop, stnerf_stream_t stream) {
    STNERF_REQUIRE(occluder && t_stop, "occluder_stop: null pointer");
    STNERF_REQUIRE(n >= 0 && (n + 255) / 256 < (int64_t)1 << 31, "occluder_stop: %lld rays exceed one launch", (long long)n);
    if (n == 0) return STNERF_OK;
    hipStream_t st = as_stream(stream);
    {
        LaunchTimer timer(PROF_OCCLUDER_STOP, 0, n, 1, 16, st);
        hipLaunchKernelGGL(occluder_stop_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, occluder, n, t_stop);
    }
    STNERF_CHECK_LAUNCH("occluder_stop");
    return STNERF_OK;
}
