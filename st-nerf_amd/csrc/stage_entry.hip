// stnerf_mlp_stage: one network stage of the pipeline as ONE persistent launch (a device-side queue of 128-row work
// items over every listed layer; the MotionNet of a deformed layer runs in front of its SpaceNet on the same rows).
// Two arithmetics behind it, both in the sample-split organisation (a wave owns 32 samples, activations in registers):
//   csrc/mlp_wave.hip    exact f32 (v_mfma_f32_32x32x2_f32)                       -- the default
//   csrc/mlp_bf16x3.hip  split-bf16: three bf16 pieces per fp32 operand, six MFMAs -- STNERF_STAGE_BF16X3
//                        (the machinery: mlp_bf16x3_core.h)
// The op-level exact-f32 entries run the same arithmetic: stnerf_spacenet_fwd is the wave kernel on one layer without a queue,
// stnerf_motionnet_fwd its MotionNet (motion_wave) in train_motion_fwd_kernel (mlp_wave_core.h).
// Reference: modeling/layered_rfrender.py:340-418 (coarse), :495-576 (fine).
#include <string.h>

#include "mlp_wave_core.h"
#include "mlp_bf16x3.h"

using namespace stnerf;

namespace stnerf {
// The op-level outputs of one sample: its flow and / or its moved point (modeling/layered_rfrender.py:356,510); null = not written.
struct MotionOpTap : NoTap {
    float* flow_out;
    float* xyz_out;
    float p[3];
    __device__ __forceinline__ void flow(const float (&fl)[3], int lane) const {
        if (lane >= 32) return;
        if (flow_out) {
            flow_out[0] = fl[0];
            flow_out[1] = fl[1];
            flow_out[2] = fl[2];
        }
        if (xyz_out) {
            xyz_out[0] = p[0] + fl[0];
            xyz_out[1] = p[1] + fl[1];
            xyz_out[2] = p[2] + fl[2];
        }
    }
};
struct MotionOpArgs {
    const float* net;
    const int32_t* ray_list;   // the work list of include/stnerf.h
    const int32_t* ray_count;
    int64_t n_rays;
    int32_t ns;
    int32_t flags;             // STNERF_MOTION_* bits
    float* xyz;
    int64_t xyz_ray_stride;
    const float* times;
    int64_t times_ray_stride;
    float* flow;               // or nullptr
    int64_t flow_ray_stride;
    __device__ __forceinline__ int64_t row_count() const { return layer_rows(ray_count, n_rays, ns); }
    __device__ __forceinline__ MotionOpTap fetch(int64_t row, int64_t n, float (&p)[3], float& tv) const {
        const RowRef r = locate_row(ray_list, row, n, ns);
        MotionOpTap t{{}, nullptr, nullptr, {0.f, 0.f, 0.f}};
        tv = 0.f;
        if (r.valid) {
            float* src = xyz + r.ray * xyz_ray_stride + 3 * r.k;
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) t.p[c3] = src[c3];
            tv = times[r.ray * times_ray_stride];
            if (flow) t.flow_out = flow + r.ray * flow_ray_stride + 3 * r.k;
            if (flags & STNERF_MOTION_ADD_TO_XYZ) t.xyz_out = src;
        }
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) p[c3] = t.p[c3];
        return t;
    }
};
}  // namespace stnerf

// layers[i] describes slot i of the queue (heavier, deformed layers first); `queue` is a zeroed uint32 on the device.
extern "C" int stnerf_mlp_stage(const stnerf_stage_layer* layers, int n_layers, int64_t n_rays, int ns, const float* dirs,
                                int64_t dirs_ray_stride, int64_t times_ray_stride, int64_t xyz_ray_stride,
                                int64_t raw_ray_stride, int flags, uint32_t* queue, float* ray_bias, stnerf_stream_t stream) {
    return stnerf_mlp_stage_rows(layers, nullptr, n_layers, n_rays, ns, dirs, dirs_ray_stride, times_ray_stride, xyz_ray_stride, raw_ray_stride,
                                 flags, queue, ray_bias, stream);
}

// rows[i]: the row list of queue slot i (include/stnerf.h: stnerf_stage_rows) or a null entry; rows == nullptr, or no entry with
// a list: the launch stnerf_mlp_stage always made.  Otherwise the row-list flavour of the same kernel (mlp_wave_rows.hip,
// mlp_bf16x3_rows.hip), listed and unlisted slots side by side in one queue.
extern "C" int stnerf_mlp_stage_rows(const stnerf_stage_layer* layers, const stnerf_stage_rows* rows, int n_layers, int64_t n_rays, int ns,
                                     const float* dirs, int64_t dirs_ray_stride, int64_t times_ray_stride, int64_t xyz_ray_stride,
                                     int64_t raw_ray_stride, int flags, uint32_t* queue, float* ray_bias, stnerf_stream_t stream) {
    STNERF_REQUIRE(layers && dirs && queue && ray_bias, "mlp_stage: null pointer");
    STNERF_REQUIRE(((uintptr_t)ray_bias & 15) == 0, "mlp_stage: ray_bias must be 16-byte aligned");
    STNERF_REQUIRE(n_layers >= 1 && n_layers <= STNERF_MAX_LAYERS && n_rays >= 0 && ns >= 1, "mlp_stage: bad shape");
    STNERF_REQUIRE((raw_ray_stride & 3) == 0, "mlp_stage: raw ray stride must be a multiple of 4 floats");
    STNERF_REQUIRE((flags & ~(STNERF_STAGE_DEEP_RGB | STNERF_STAGE_SIGMOID_RGB | STNERF_STAGE_BF16X3)) == 0, "mlp_stage: unknown flags %d", flags);
    StageRowsArgs ra;
    memset(&ra, 0, sizeof(ra));
    bool listed = false;
    for (int i = 0; rows && i < n_layers; ++i) {
        if (!rows[i].row_list) continue;
        STNERF_REQUIRE(rows[i].row_count, "mlp_stage: layer %d: a row list without its row count", i);
        STNERF_REQUIRE(ns <= 256 && n_rays <= ((int64_t)1 << 23), "mlp_stage: a row list packs (ray << 8 | k): ns <= 256 and n_rays <= 2^23 (got %d, %lld)",
                       ns, (long long)n_rays);
        ra.row_list[i] = rows[i].row_list;
        ra.row_count[i] = rows[i].row_count;
        listed = true;
    }
    if (n_rays == 0) return STNERF_OK;
    const int deep_rgb = (flags & STNERF_STAGE_DEEP_RGB) != 0;
    const bool bf16x3 = (flags & STNERF_STAGE_BF16X3) != 0;
    StageArgs a;
    memset(&a, 0, sizeof(a));
    a.sigmoid_rgb = (flags & STNERF_STAGE_SIGMOID_RGB) != 0;
    // (the profiler's record of the stage covers the per-ray prologues too: their work is part of the networks' FLOPs)
    LaunchTimer timer(PROF_MLP_STAGE, deep_rgb | (bf16x3 ? 2 : 0) | (listed ? 4 : 0), n_rays, ns, 0, as_stream(stream));
    for (int i = 0; i < n_layers; ++i) {
        const stnerf_stage_layer& s = layers[i];
        STNERF_REQUIRE(s.space && s.xyz && s.raw, "mlp_stage: layer %d: null pointer", i);
        // (a bf16x3 blob is streamed by 16-byte LDS-DMA from 1 KB-aligned sections: the blob itself must be 1 KB aligned)
        const uintptr_t amask = bf16x3 ? 1023 : 15;
        STNERF_REQUIRE(((uintptr_t)s.space & amask) == 0 && ((uintptr_t)s.raw & 15) == 0 && (!s.motion || ((uintptr_t)s.motion & amask) == 0),
                       "mlp_stage: layer %d: packed weights must be %d-byte aligned, raw 16-byte aligned", i, (int)amask + 1);
        STNERF_REQUIRE(!(s.use_time || s.motion) || s.times, "mlp_stage: layer %d needs its frame-id column", i);
        a.layer[i] = StageLayer{static_cast<const float*>(s.space), static_cast<const float*>(s.motion), s.ray_list,
                                s.ray_count, s.xyz, s.raw, s.times, s.use_time, s.motion_flags,
                                ray_bias + (int64_t)i * n_rays * 128};
        // rgb_net.1's direction / time columns once per ray of this layer (mlp_raybias.hip; exact f32 for both arithmetics:
        // a bf16x3 blob starts with the network's exact-f32 blob)
        const int kind = s.use_time ? (deep_rgb ? STNERF_NET_SPACE_TIME_DEEP : STNERF_NET_SPACE_TIME)
                                    : (deep_rgb ? STNERF_NET_SPACE_DEEP : STNERF_NET_SPACE);
        if (const int rc = launch_ray_bias(kind, static_cast<const float*>(s.space), n_rays, s.ray_list, s.ray_count, dirs,
                                           dirs_ray_stride, s.times, times_ray_stride, ray_bias + (int64_t)i * n_rays * 128,
                                           as_stream(stream), s.rotation))
            return rc;
    }
    a.n_layers = n_layers;
    a.ns = ns;
    a.n_rays = n_rays;
    a.xyz_ray_stride = xyz_ray_stride;
    a.raw_ray_stride = raw_ray_stride;
    a.dirs_ray_stride = dirs_ray_stride;
    a.times_ray_stride = times_ray_stride;
    a.dirs = dirs;
    a.queue = queue;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (listed)
        return bf16x3 ? launch_bf16x3_stage_rows(a, ra, deep_rgb != 0, cus, as_stream(stream))
                      : launch_wave_stage_rows(a, ra, deep_rgb != 0, cus, as_stream(stream));
    return bf16x3 ? launch_bf16x3_stage(a, deep_rgb != 0, cus, as_stream(stream)) : launch_wave_stage(a, deep_rgb != 0, cus, as_stream(stream));
}

// One SpaceNet on the work list of include/stnerf.h: a one-layer exact-f32 stage, raw output, no queue (workgroup b takes the
// items b, b + grid, ...).
extern "C" int stnerf_spacenet_fwd(int kind, const void* packed, int64_t n_rays, int ns, const int32_t* ray_list,
                                   const int32_t* ray_count, const float* xyz, int64_t xyz_ray_stride,
                                   const float* dirs, int64_t dirs_ray_stride, const float* times,
                                   int64_t times_ray_stride, float* raw, int64_t raw_ray_stride, float* ray_bias,
                                   stnerf_stream_t stream) {
    return stnerf_spacenet_fwd_rot(kind, packed, n_rays, ns, ray_list, ray_count, xyz, xyz_ray_stride, dirs, dirs_ray_stride, times,
                                   times_ray_stride, raw, raw_ray_stride, ray_bias, nullptr, stream);
}

// (rotation_host: the layer's rotation or null -- it reaches the ray-bias launch only)
extern "C" int stnerf_spacenet_fwd_rot(int kind, const void* packed, int64_t n_rays, int ns, const int32_t* ray_list,
                                       const int32_t* ray_count, const float* xyz, int64_t xyz_ray_stride,
                                       const float* dirs, int64_t dirs_ray_stride, const float* times,
                                       int64_t times_ray_stride, float* raw, int64_t raw_ray_stride, float* ray_bias,
                                       const stnerf_layer_rotation* rotation_host, stnerf_stream_t stream) {
    STNERF_REQUIRE(STNERF_NET_IS_SPACE(kind), "spacenet_fwd: bad kind %d", kind);
    STNERF_REQUIRE(packed && xyz && dirs && raw && ray_bias, "spacenet_fwd: null pointer");
    STNERF_REQUIRE(((uintptr_t)ray_bias & 15) == 0, "spacenet_fwd: ray_bias must be 16-byte aligned");
    STNERF_REQUIRE(!STNERF_NET_USES_TIME(kind) || times, "spacenet_fwd: net takes time but times is null");
    STNERF_REQUIRE(n_rays >= 0 && ns >= 1, "spacenet_fwd: bad shape n_rays=%lld ns=%d", (long long)n_rays, ns);
    STNERF_REQUIRE((raw_ray_stride & 3) == 0 && ((uintptr_t)raw & 15) == 0, "spacenet_fwd: raw must be 16-byte aligned");
    STNERF_REQUIRE(((uintptr_t)packed & 15) == 0, "spacenet_fwd: packed weights must be 16-byte aligned");
    if (n_rays == 0) return STNERF_OK;
    // rgb_net.1's direction / time columns once per ray (mlp_raybias.hip) -> the rows added behind that layer's product
    if (const int rc = launch_ray_bias(kind, static_cast<const float*>(packed), n_rays, ray_list, ray_count, dirs, dirs_ray_stride,
                                       times, times_ray_stride, ray_bias, as_stream(stream), rotation_host))
        return rc;
    StageArgs a;
    memset(&a, 0, sizeof(a));
    a.layer[0] = StageLayer{static_cast<const float*>(packed), nullptr, ray_list, ray_count, xyz, raw, times,
                            STNERF_NET_USES_TIME(kind) ? 1 : 0, 0, ray_bias};
    a.n_layers = 1;
    a.ns = ns;
    a.n_rays = n_rays;
    a.xyz_ray_stride = xyz_ray_stride;
    a.raw_ray_stride = raw_ray_stride;
    a.dirs_ray_stride = dirs_ray_stride;
    a.times_ray_stride = times_ray_stride;
    a.dirs = dirs;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    LaunchTimer timer(PROF_SPACENET, kind, n_rays, ns, 0, as_stream(stream));
    return launch_wave_stage(a, STNERF_NET_IS_DEEP(kind), cus, as_stream(stream));
}

// One MotionNet on the work list of include/stnerf.h: the op-level instantiation of train_motion_fwd_kernel (mlp_wave_core.h).
extern "C" int stnerf_motionnet_fwd(const void* packed, int64_t n_rays, int ns, const int32_t* ray_list,
                                    const int32_t* ray_count, float* xyz, int64_t xyz_ray_stride, const float* times,
                                    int64_t times_ray_stride, float* flow, int64_t flow_ray_stride, int add_to_xyz,
                                    stnerf_stream_t stream) {
    STNERF_REQUIRE(packed && xyz && times, "motionnet_fwd: null pointer");
    STNERF_REQUIRE(flow || (add_to_xyz & STNERF_MOTION_ADD_TO_XYZ), "motionnet_fwd: nothing to write");
    STNERF_REQUIRE(n_rays >= 0 && ns >= 1, "motionnet_fwd: bad shape");
    STNERF_REQUIRE(((uintptr_t)packed & 15) == 0, "motionnet_fwd: packed weights must be 16-byte aligned");
    if (n_rays == 0) return STNERF_OK;
    const MotionOpArgs a{static_cast<const float*>(packed), ray_list, ray_count, n_rays, ns, add_to_xyz, xyz, xyz_ray_stride, times,
                         times_ray_stride, flow, flow_ray_stride};
    LaunchTimer timer(PROF_MOTIONNET, STNERF_NET_MOTION, n_rays, ns, 0, as_stream(stream));
    return launch_motion_fwd(a, n_rays * ns, "motionnet_fwd", as_stream(stream));
}
