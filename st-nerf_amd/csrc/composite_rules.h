// The compositor's rules that its forward (composite.hip) and its backward (render_bwd.hip) must state alike: the
// post-network density edits of a sample, and which layers of a ray have network output; and the weighted sums its forward
// shares with the occluder split of the merged weights (occluder.hip).
#pragma once
#include <math.h>

#include "common.h"
#include "wave_prims.h"

namespace stnerf {

// ---------------------------------------------------------------------------------------------
// The post-network density edits (a10) of ONE sample of a layer with network output, in the reference's order
// (modeling/layered_rfrender.py):
//   cut_neg   :414                        coarse stage, performers: sigma = 0 where t < 0
//   thr       :416-418, :538-547, :564-566  sigma = 0 below the layer's threshold; a layer without one carries thr = -inf
//                                         (x < -inf is false for every x, NaN included)
//   scale     :575-576                    sigma *= sigma_scale
//   cut_near  :422                        coarse stage, background: sigma = 0 where t < near
//   activated layers/render_layer.py:47   rgb = torch.sigmoid(rgb), unless the caller hands in activated colours
// The sigmoid is evaluated once per sample here and shared by the per-layer and the merged composite.  The fine stage's
// merged-only `t < near` cut (:605) is not an edit of the sample: the merged composites apply it to their own copy.
// dsigma (the backward, render_bwd.hip): receives d sigma' / d sigma -- 0 where sigma was overwritten, sigma_scale where it
// was multiplied.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 edit_sample(float4 v, float t, bool cut_neg, float thr, float scale, bool cut_near, float nearv,
                                              bool activated, float* dsigma = nullptr) {
    float f = 1.f;
    if (cut_neg && t < 0.f) v.w = f = 0.f;
    if (v.w < thr) v.w = f = 0.f;
    v.w = v.w * scale;
    f = f * scale;
    if (cut_near && t < nearv) v.w = f = 0.f;
    if (dsigma) *dsigma = f;
    if (!activated) {
        v.x = sigmoidf(v.x);
        v.y = sigmoidf(v.y);
        v.z = sigmoidf(v.z);
    }
    return v;
}

// The switches of edit_sample for one layer (wave-uniform wherever the layer is).
struct LayerEdit {
    bool cut_neg, cut_near;
    float thr, scale;
};
__device__ __forceinline__ LayerEdit layer_edit(const stnerf_composite_params& p, int layer) {
    return LayerEdit{!p.fine && p.cut_negative_t && layer > 0, !p.fine && layer == 0,
                     p.use_threshold[layer] != 0 ? p.threshold[layer] : -INFINITY, p.sigma_scale[layer]};
}

// The layers' thresholds and scales as a table in LDS, thr[16] | scale[16] (EDIT_TAB_BYTES), for code that picks a sample's
// layer per lane.  Every thread of the workgroup calls it; __syncthreads() before the first read.
constexpr int EDIT_TAB_BYTES = 128;
__device__ __forceinline__ void build_edit_table(float* tab, const stnerf_composite_params& p, int l) {
#pragma unroll
    for (int i = 0; i < STNERF_MAX_LAYERS; ++i)   // (unrolled: no dynamic index into the kernel's arguments)
        if (i < l && (int)threadIdx.x == i) {
            tab[i] = p.use_threshold[i] != 0 ? p.threshold[i] : -INFINITY;
            tab[16 + i] = p.sigma_scale[i];
        }
}

// ---------------------------------------------------------------------------------------------
// The weighted sums of a composite, shared by the compositor (composite.hip) and the occluder split of its merged weights
// (occluder.hip): each lane accumulates acc = acc + w x over its samples, the wave's totals come from in-place prefix scans.
// ---------------------------------------------------------------------------------------------
// Running state of one composite: the transmittance carried from block to block and the five weighted sums.
struct CompositeAcc {
    float carry = 1.f, cr = 0.f, cg = 0.f, cb = 0.f, cd = 0.f, ca = 0.f;
};

// the five sums over the wave, stored by lane 63 (which holds the totals of the in-place scans)
__device__ __forceinline__ void composite_store5(const CompositeAcc& A, float* dst, float* dst2, unsigned lane) {
    const float o0 = wave_scan_add(A.cr), o1 = wave_scan_add(A.cg), o2 = wave_scan_add(A.cb), o3 = wave_scan_add(A.cd),
                o4 = wave_scan_add(A.ca);
    if (lane == 63u) {
        if (dst) { dst[0] = o0; dst[1] = o1; dst[2] = o2; dst[3] = o3; dst[4] = o4; }
        if (dst2) { dst2[0] = o0; dst2[1] = o1; dst2[2] = o2; dst2[3] = o3; dst2[4] = o4; }
    }
}
// the same five totals as wave-uniform values, for a caller that goes on computing with them
__device__ __forceinline__ void composite_total5(const CompositeAcc& A, float (&o)[5]) {
    o[0] = wave_last(wave_scan_add(A.cr));
    o[1] = wave_last(wave_scan_add(A.cg));
    o[2] = wave_last(wave_scan_add(A.cb));
    o[3] = wave_last(wave_scan_add(A.cd));
    o[4] = wave_last(wave_scan_add(A.ca));
}

// Which layers have network output (stnerf_composite_params::evaluated): bit i of `masked` = on the rays layer i's hit mask
// marks (1), of `always` = on every ray whatever the mask says (2) -- the background: bkgd_spacenet runs on all rays and its
// output is composited even where ray_mask[0] is False (a ray through an edge of the background box: start == end, bin
// width 0; layered_rfrender.py:382-392,435-444, fixture fwd_grazing).  Neither: no output (a hidden layer).
// UNROLL: sixteen predicated steps without a dynamic index into the kernel's arguments (the merge kernel's form, fused
// with its build_edit_table); the rolled loop is ~ 400 instructions shorter in the kernels that do not need that.
struct EvalBits {
    unsigned masked = 0, always = 0;
};
template <bool UNROLL>
__device__ __forceinline__ EvalBits eval_bits(const stnerf_composite_params& p, int l) {
    EvalBits e;
    auto one = [&](int i) {
        if (p.evaluated[i] == 2) e.always |= 1u << i;
        else if (p.evaluated[i] != 0) e.masked |= 1u << i;
    };
    if (UNROLL) {
#pragma unroll
        for (int i = 0; i < STNERF_MAX_LAYERS; ++i)
            if (i < l) one(i);
    } else {
        for (int i = 0; i < l; ++i) one(i);
    }
    return e;
}
// bit i: the ray reads layer i's raw output (`hit`: the ray's hit-mask bits; `has_mask` false: the call has no mask)
__device__ __forceinline__ unsigned have_layers(EvalBits e, bool has_mask, unsigned hit) {
    return e.always | (e.masked & (has_mask ? hit : ~0u));
}

}  // namespace stnerf
