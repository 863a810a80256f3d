// stnerf_render_rays_opts: the whole chunk pipeline of LayeredRFRender.forward (modeling/layered_rfrender.py:141-734)
// behind ONE C-ABI call -- coarse sampler -> mask compaction -> [MotionNet] -> SpaceNets -> density edits +
// per-layer composite + depth merge + merged composite -> inverse-CDF resample -> [MotionNet] -> fine SpaceNets ->
// composite.  Host-side sequencing only: every stage is one of the kernels behind the op-level entry points,
// enqueued on the caller's stream into a caller-provided workspace (no allocation, no synchronisation).
// Every optional argument travels in one stnerf_render_options record (include/stnerf.h).  The call is three things, in this
// order in the file: check_call (the argument checks and the bit sets they derive), Workspace (the carve, beside the Plan and
// RowPlan the size query shares with it) and launch_sequence.  The named entries stnerf_render_rays[_cached | _rot | _scene |
// _opacity | _occupancy | _samples | _terminated | _background | _layers | _occluded] and the four named size queries are the
// fixed-argument forms: each fills a record and forwards it (the end of the file).
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"
#include "mlp_bf16x3.h"

using namespace stnerf;

namespace {

struct Carve {
    char* base;
    int64_t off, cap;
    template <class T>
    T* take(int64_t count) {
        off = (off + 255) & ~int64_t(255);
        T* p = reinterpret_cast<T*>(base + off);
        off += count * (int64_t)sizeof(T);
        return p;
    }
};

// sizes of the workspace regions for n rays (shared by the size query and the carve)
struct Plan {
    int64_t t_c, xyz_c, raw_c, w_c, slots, t_f, xyz_f, raw_f, list, count, flags, raybias;
    // Once the resampler has read t_c / w_c the whole coarse block [t_c | xyz_c | raw_c | w_c] is dead: the fine network outputs
    // (raw_f, the largest fine buffer) are written over it.  shared = the larger of the two.  64 + 64 samples: 9 n1 = 576 floats
    // of coarse block per (ray, layer) against 4 S = 512 of raw_f -- the workspace goes from 1728 to 1216 floats (- 30 %).
    static int64_t pad(int64_t floats) { return (floats + 63) & ~int64_t(63); }   // 256-byte granules, as Carve::take
    // The fine MotionNet's slot lists (MotionNet reuse, below) are written over raw_c / w_c, which are dead once the resampler
    // has run, and read before the fine stage writes raw_f: 64 + 64 samples need n2 = 64 of the 5 l n1 words there.
    int64_t tail() const { return pad(raw_c) + pad(w_c) > pad(slots) ? pad(raw_c) + pad(w_c) : pad(slots); }
    int64_t coarse_block() const { return pad(t_c) + pad(xyz_c) + tail(); }
    int64_t shared() const { return coarse_block() > pad(raw_f) ? coarse_block() : pad(raw_f); }
    int64_t bytes() const { return (shared() + t_f + xyz_f + raybias) * 4 + (list + count) * 4 + flags + 16 * 256; }
};
Plan make_plan(int64_t n, int l, int n1, int n2, int only_coarse) {
    Plan p;
    const int64_t S = n1 + n2;
    p.t_c = n * l * n1;
    p.xyz_c = n * l * n1 * 3;
    p.raw_c = n * l * n1 * 4;
    p.w_c = only_coarse ? 0 : n * l * n1;
    p.slots = only_coarse ? 0 : n * n2;   // int32, one layer at a time
    p.t_f = only_coarse ? 0 : n * l * S;
    p.xyz_f = only_coarse ? 0 : n * l * S * 3;
    p.raw_f = only_coarse ? 0 : n * l * S * 4;
    p.list = (int64_t)l * n;
    p.flags = n;                      // one byte per ray: the compositor's scratch
    // hit-ray counts + the work-queue heads of the two network stages + those of the MotionNet launches (coarse, fine per layer)
    p.count = STNERF_MAX_LAYERS + 2 + 2 * STNERF_MAX_LAYERS;
    p.raybias = (int64_t)l * n * 128;  // per (layer, ray): rgb_net.1's bias rows (mlp_raybias.hip), reused by both stages
    return p;
}

int sampled_layers(int l, const int32_t* samples) {
    int c = 0;
    for (int i = 0; samples && i < l; ++i) c += samples[i] ? 1 : 0;
    return c;
}
bool any_flag(int l, const int32_t* flags) {
    for (int i = 0; flags && i < l; ++i)
        if (flags[i]) return true;
    return false;
}

// The three culls' share of the workspace, shared by the size query and the carve as Plan is.  A layer walks
// ONE row list of n x (samples of the larger stage) words when it is sample-culled, when its fine stage is terminated (a flag and a
// fine stage: nothing under only_coarse) or when it is the background under its grid -- which shares the list termination gives
// layer 0.  The lists bring their counts; termination brings the stop depths, n floats that live from the coarse composite to the
// fine stage.  Nothing without a cull.
struct RowPlan {
    uint32_t listed = 0;    // bit i: layer i has a row list
    int n_lists = 0;        // (a sample flag on layer 0 beside a grid is counted twice, as the named queries always did: the call refuses it)
    bool stops = false;     // termination: t_stop
    int64_t row_cap = 0;    // words per list
    int64_t bytes(int64_t n) const {
        if (n_lists == 0) return 0;
        return n_lists * ((row_cap * 4 + 255) & ~int64_t(255)) + STNERF_MAX_LAYERS * 4 + 2 * 256 + (stops ? ((n * 4 + 255) & ~int64_t(255)) + 256 : 0);
    }
};
RowPlan make_row_plan(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples, const int32_t* terminate, bool bg) {
    RowPlan r;
    r.row_cap = n * (only_coarse ? n1 : n1 + n2);
    r.stops = !only_coarse && any_flag(l, terminate);
    for (int i = 0; i < l; ++i) {
        const bool own = (samples && samples[i]) || (r.stops && terminate[i]);
        if (own || (bg && i == 0)) r.listed |= 1u << i;
        r.n_lists += own ? 1 : 0;
    }
    if (bg && !(r.stops && terminate[0])) r.n_lists += 1;
    return r;
}

// the workspace of one call, carved as Plan and RowPlan size it
struct Workspace {
    float *t_c, *xyz_c, *raw_c, *w_c, *raw_f, *t_f, *xyz_f, *ray_bias, *t_stop = nullptr;
    int32_t *slots, *ray_list, *ray_count, *row_count = nullptr;
    int32_t* row_list[STNERF_MAX_LAYERS] = {nullptr};
    uint8_t* ray_flags;
    Workspace(void* base, int64_t bytes, const Plan& pl, const RowPlan& rows, int64_t n, int l) {
        Carve ws{static_cast<char*>(base), 0, bytes};
        float* shared = ws.take<float>(pl.shared());
        Carve cb{reinterpret_cast<char*>(shared), 0, pl.shared() * 4};   // the coarse block inside the shared region
        t_c = cb.take<float>(pl.t_c);
        xyz_c = cb.take<float>(pl.xyz_c);
        raw_c = cb.take<float>(pl.raw_c);
        w_c = cb.take<float>(pl.w_c);
        slots = reinterpret_cast<int32_t*>(raw_c);   // over raw_c / w_c: written after the resampler, read before the fine stage
        raw_f = shared;            // over the coarse block: first written by the fine stage, after the resampler read t_c / w_c
        t_f = ws.take<float>(pl.t_f);
        xyz_f = ws.take<float>(pl.xyz_f);
        ray_list = ws.take<int32_t>(pl.list);
        ray_count = ws.take<int32_t>(pl.count);
        ray_flags = ws.take<uint8_t>(pl.flags);
        ray_bias = ws.take<float>(pl.raybias);
        if (rows.listed) {
            for (int i = 0; i < l; ++i)
                if (rows.listed >> i & 1) row_list[i] = ws.take<int32_t>(rows.row_cap);
            row_count = ws.take<int32_t>(STNERF_MAX_LAYERS);
            if (rows.stops) t_stop = ws.take<float>(n);
        }
    }
};

const stnerf_render_options kNoOptions = {(int32_t)sizeof(stnerf_render_options)};

// The record is stnerf_render_options or, with the deep fields behind it, stnerf_render_options_deep or, with the proposal table behind
// those, stnerf_render_options_proposal: struct_size says which.
int check_options_size(const stnerf_render_options* opts, const char* what) {
    STNERF_REQUIRE(!opts || opts->struct_size == (int32_t)sizeof(stnerf_render_options) || opts->struct_size == (int32_t)sizeof(stnerf_render_options_deep) ||
                       opts->struct_size == (int32_t)sizeof(stnerf_render_options_proposal),
                   "%s: stnerf_render_options.struct_size = %d is not a size this library knows (%d, %d with the deep fields, or %d with the proposal table): set it to sizeof",
                   what, opts ? (int)opts->struct_size : 0, (int)sizeof(stnerf_render_options), (int)sizeof(stnerf_render_options_deep),
                   (int)sizeof(stnerf_render_options_proposal));
    return STNERF_OK;
}

// the deep fields of a record that has them; nullptr: no deep output
const stnerf_render_options_deep* deep_options(const stnerf_render_options* opts) {
    if (!opts || (opts->struct_size != (int32_t)sizeof(stnerf_render_options_deep) && opts->struct_size != (int32_t)sizeof(stnerf_render_options_proposal)))
        return nullptr;
    const stnerf_render_options_deep* d = reinterpret_cast<const stnerf_render_options_deep*>(opts);
    return d->deep_samples ? d : nullptr;
}

// the proposal table of a record that has one with a grid among its first l entries; nullptr: no grid proposal
const stnerf_density_grid* proposal_options(const stnerf_render_options* opts, int l) {
    if (!opts || opts->struct_size != (int32_t)sizeof(stnerf_render_options_proposal)) return nullptr;
    const stnerf_density_grid* t = reinterpret_cast<const stnerf_render_options_proposal*>(opts)->proposal;
    for (int i = 0; t && i < l && i < STNERF_MAX_LAYERS; ++i)
        if (t[i].sigma) return t;
    return nullptr;
}

// Deep output (include/stnerf.h): count -> offsets -> fill on the final stage's buffers, behind its scene pass.
int launch_deep(const stnerf_render_options_deep& d, const float* t, const float* raw, const uint8_t* mask, const float* merged_weights, int64_t n, int l,
                int S, const stnerf_composite_params* cp, stnerf_stream_t stream) {
    const int64_t scan = stnerf_deep_workspace_bytes(n);
    int32_t* counts = reinterpret_cast<int32_t*>(static_cast<char*>(d.deep_workspace) + scan);
    int rc = stnerf_deep_count(t, mask, merged_weights, n, l, S, cp, d.deep_w_min, d.deep_merge_dz, counts, stream);
    if (rc) return rc;
    rc = stnerf_deep_offsets(counts, n, (int64_t)l * S, d.deep_offsets, d.deep_workspace, scan, stream);
    if (rc) return rc;
    return stnerf_deep_fill(t, raw, mask, merged_weights, n, l, S, cp, d.deep_w_min, d.deep_merge_dz, d.deep_offsets, d.deep_samples, d.deep_capacity,
                            d.deep_total, stream);
}

}  // namespace

extern "C" int64_t stnerf_render_workspace_bytes_opts(int64_t n, int l, int n1, int n2, int only_coarse, const stnerf_render_options* opts) {
    const int src = check_options_size(opts, "render_workspace_bytes");
    if (src) return src;
    if (n < 0 || l < 1 || l > STNERF_MAX_LAYERS || n1 < 3 || n2 < 0) {
        set_error("render_workspace_bytes: bad shape");
        return STNERF_EINVAL;
    }
    const stnerf_render_options& o = opts ? *opts : kNoOptions;
    return make_plan(n, l, n1, n2, only_coarse).bytes() +
           make_row_plan(n, l, n1, n2, only_coarse, o.samples, o.terminate, (o.bkgd_grid && o.bkgd_grid->bits) || o.bkgd_rays).bytes(n);
}

// The mask the caller gets back is the reference's ray_mask (0 / 1): the sampler's "missed" hint (bit 1) served the compositor and
// the resampler inside the call and is cleared on the way out (a C caller testing `mask != 0` must not see it).
static __global__ void clear_mask_hints_kernel(uint8_t* mask, int64_t count) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) mask[i] &= 1;
}
static int clear_mask_hints(uint8_t* mask, int64_t count, hipStream_t stream) {
    hipLaunchKernelGGL(clear_mask_hints_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, stream, mask, count);
    STNERF_CHECK_LAUNCH("render_rays (mask)");
    return STNERF_OK;
}

// ---- MotionNet reuse (split-bf16 stages).  The fine pass deforms all n1 + n2 sorted depths of a performer ray (:495-510); n1 of
// them ARE the coarse depths, which the coarse pass has deformed with the same network, frame id and flags (:340-356).  With the
// same box edit in both passes a depth gives the same point (t d + o, then the un-edit: the same expression in the sampler and
// the resampler), so the same flow.  Such a layer runs its MotionNet in launches of its own (mlp_bf16x3_motion_kernel): over the
// coarse points in place, then -- after the resampler -- only over the fine samples whose depth is not one of the coarse ones;
// the others take the moved coarse point.  Both stage launches then skip its MotionNet.  The points are the fused kernel's bits.

// One wave per hit ray of `layer`: fine sample m whose depth is bitwise one of the coarse depths takes that coarse sample's moved
// point; the others, ascending, are the ray's slot list (n2 entries, -1 padded: at least n1 of the S samples are coarse depths).
static __global__ void __launch_bounds__(256) motion_reuse_fill_kernel(const float* __restrict__ t_c, const float* __restrict__ xyz_c,
                                                                       const float* __restrict__ t_f, float* __restrict__ xyz_f,
                                                                       const int32_t* __restrict__ ray_list, const int32_t* __restrict__ ray_count,
                                                                       int64_t n, int l, int layer, int n1, int n2, int32_t* __restrict__ slots) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t cnt = *ray_count < n ? (int64_t)*ray_count : n;
    if (w >= cnt) return;
    const int64_t ray = ray_list[w];
    const int S = n1 + n2;
    const int64_t pair = ray * l + layer;
    const uint32_t* tc = reinterpret_cast<const uint32_t*>(t_c) + pair * n1;
    const uint32_t* tf = reinterpret_cast<const uint32_t*>(t_f) + pair * S;
    int32_t* sl = slots + ray * n2;
    int filled = 0;
    for (int m0 = 0; m0 < S; m0 += 64) {
        const int m = m0 + lane;
        int match = -1;
        if (m < S) {
            const uint32_t v = tf[m];
            for (int k = 0; k < n1 && match < 0; ++k) match = tc[k] == v ? k : -1;
        }
        const bool open = m < S && match < 0;
        const uint64_t bal = __ballot(open);
        if (open) {
            const int pos = filled + __popcll(bal & ((1ull << lane) - 1ull));
            if (pos < n2) sl[pos] = m;
        } else if (m < S) {
            const float* src = xyz_c + (pair * n1 + match) * 3;
            float* dst = xyz_f + (pair * S + m) * 3;
            dst[0] = src[0];
            dst[1] = src[1];
            dst[2] = src[2];
        }
        filled += __popcll(bal);
    }
    for (int j = filled + lane; j < n2; j += 64) sl[j] = -1;
}

// MotionNet of performer `layer` over rows (hit ray, j < ns) in place; slots: the fine pass's lists (nullptr: row j = sample j)
static int motion_rows(const stnerf_nets* nets, const stnerf_render_params* p, const float* rays, int64_t n, int layer, int ns, int S,
                       float* xyz, const int32_t* ray_list, const int32_t* ray_count, const int32_t* slots, int slot_stride,
                       uint32_t* queue, hipStream_t st) {
    STNERF_REQUIRE(((uintptr_t)nets->motion[layer] & 1023) == 0, "render_rays: packed MotionNet of layer %d must be 1024-byte aligned", layer);
    MotionBxArgs a;
    memset(&a, 0, sizeof(a));
    a.net = static_cast<const float*>(nets->motion[layer]);
    a.ray_list = ray_list + (int64_t)layer * n;
    a.ray_count = ray_count + layer;
    a.n_rays = n;
    a.ns = ns;
    a.flags = 0;
    a.xyz = xyz + (int64_t)layer * S * 3;
    a.xyz_ray_stride = (int64_t)p->l * S * 3;
    a.times = rays + (p->retiming ? 6 + layer : 6);
    a.times_ray_stride = p->ray_stride;
    a.slots = slots;
    a.slot_ray_stride = slot_stride;
    a.queue = queue;
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    set_launch_tag(layer);
    int rc;
    {
        LaunchTimer timer(PROF_MOTIONNET, STNERF_NET_MOTION, n, ns, 0, st);
        rc = launch_bf16x3_motion(a, cus, st);
    }
    set_launch_tag(-1);
    return rc;
}

// ---- the background cache (include/stnerf.h: stnerf_bkgd_cache).  One layer's slice of raw[n][l][ns][4] <-> dense[n][ns][4]: a lane
// moves one 16-byte sample, four independent samples in flight per lane and trip; the dense side is coalesced, the strided side
// runs of ns x 16 bytes.  64-bit flat index (a 1080p view at 64 + 64 samples has 2.7e8 samples, 4.2 GB, per layer).
template <bool TO_DENSE>
static __global__ void __launch_bounds__(256) copy_layer_raw_kernel(float4* __restrict__ raw, float4* __restrict__ dense, int64_t total,
                                                                    int l, int layer, int ns) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i0 < total; i0 += 4 * stride) {
        float4 v[4];
        int64_t at[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = i0 + j * stride;
            const int64_t ray = i / ns;
            at[j] = (ray * l + layer) * ns + (i - ray * ns);
            if (i < total) v[j] = TO_DENSE ? raw[at[j]] : dense[i];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int64_t i = i0 + j * stride;
            if (i < total) (TO_DENSE ? dense[i] : raw[at[j]]) = v[j];
        }
    }
}

extern "C" int stnerf_copy_layer_raw(float* raw, int64_t n, int l, int layer, int ns, float* dense, int to_dense,
                                     stnerf_stream_t stream) {
    STNERF_REQUIRE(raw && dense, "copy_layer_raw: null pointer");
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && layer >= 0 && layer < l && ns >= 1, "copy_layer_raw: bad shape");
    STNERF_REQUIRE((((uintptr_t)raw | (uintptr_t)dense) & 15) == 0, "copy_layer_raw: raw and dense must be 16-byte aligned");
    const int64_t total = n * ns;
    if (total == 0) return STNERF_OK;
    // memory-bound: at most 8 workgroups per CU's worth of blocks, the rest by the grid-stride loop
    const int64_t blocks = (total + 1023) / 1024;
    const dim3 grid((unsigned)(blocks < 2048 ? blocks : 2048));
    hipStream_t st = as_stream(stream);
    LaunchTimer timer(PROF_COPY_LAYER_RAW, to_dense ? 1 : 0, n, ns, 32 * (int64_t)ns, st);
    if (to_dense)
        hipLaunchKernelGGL(copy_layer_raw_kernel<true>, grid, dim3(256), 0, st, reinterpret_cast<float4*>(raw),
                           reinterpret_cast<float4*>(dense), total, l, layer, ns);
    else
        hipLaunchKernelGGL(copy_layer_raw_kernel<false>, grid, dim3(256), 0, st, reinterpret_cast<float4*>(raw),
                           reinterpret_cast<float4*>(dense), total, l, layer, ns);
    STNERF_CHECK_LAUNCH("copy_layer_raw");
    return STNERF_OK;
}

// ---- the render call.  The 15 arguments every render entry starts with, and the same handed on:
#define RENDER_PARAMS                                                                                                                   \
    const float *rays, int64_t n, const float *boxes, int64_t box_ray_stride, const stnerf_nets *nets, const stnerf_render_params *p,    \
        const float *jitter, const float *u, void *workspace, int64_t workspace_bytes, float *mixed_fine, float *mixed_coarse,          \
        float *layer_fine, float *layer_coarse, uint8_t *mask
#define RENDER_ARGS rays, n, boxes, box_ray_stride, nets, p, jitter, u, workspace, workspace_bytes, mixed_fine, mixed_coarse, layer_fine, layer_coarse, mask

namespace {

// what the checks derive from a call's arguments
struct Call {
    int n_sampled;            // sample-culled layers
    bool flagged;             // a terminate flag is set
    bool bg;                  // the background's grid has bits
    bool bg_rows;             // layer 0 walks a row list of its own launch: under its grid, under the per-ray mask, or both
    int cache_mode;           // the background cache's
    uint32_t lcap, lreuse;    // bit i: performer i's slices go to / come from its layer cache entry (a hidden layer's entry is ignored)
    uint32_t term;            // bit i: layer i's fine stage is terminated
    uint32_t prop;            // bit i: layer i's coarse densities come from its density grid (a grid proposal)
    RowPlan rows;
};

// Every argument check of the render call, on the host and before anything is launched.
int check_call(RENDER_PARAMS, const stnerf_render_options& o, const stnerf_render_options_deep* deep, const stnerf_density_grid* proposal, Call* call) {
    STNERF_REQUIRE(rays && boxes && nets && p && workspace && mask, "render_rays: null pointer");
    if (deep) {
        STNERF_REQUIRE(o.scene_out, "render_rays: deep output needs scene_out (the merged weights exist only with the scene passes)");
        STNERF_REQUIRE(deep->deep_offsets && deep->deep_total && deep->deep_workspace, "render_rays: deep output needs deep_offsets, deep_total and deep_workspace");
        STNERF_REQUIRE(deep->deep_w_min >= 0.f && deep->deep_merge_dz >= 0.f, "render_rays: deep_w_min = %g / deep_merge_dz = %g is negative or NaN",
                       (double)deep->deep_w_min, (double)deep->deep_merge_dz);
        STNERF_REQUIRE(deep->deep_capacity >= 0 && ((uintptr_t)deep->deep_samples & 15) == 0 && ((uintptr_t)deep->deep_workspace & 7) == 0,
                       "render_rays: deep_capacity = %lld, deep_samples 16-byte and deep_workspace 8-byte aligned", (long long)deep->deep_capacity);
        const int Sd = p->only_coarse ? p->n1 : p->n1 + p->n2;
        STNERF_REQUIRE(Sd <= 256 && n <= (int64_t)INT32_MAX / ((int64_t)(p->l > 0 ? p->l : 1) * (Sd > 0 ? Sd : 1)),
                       "render_rays: deep output packs first_k in eight bits and one call's records in 31: samples per layer <= 256, n l S < 2^31");
    }
    STNERF_REQUIRE(!o.occluder || (o.scene_out && o.occluded_mixed),
                   "render_rays: an occluder needs scene_out and occluded_mixed (the merged weights exist only with the scene passes)");
    STNERF_REQUIRE(o.occluder || (!o.occluder_stops && !o.occluded_mixed && !o.occluded_scene && !o.occluder_share),
                   "render_rays: occluder_stops / occluded outputs without an occluder");
    STNERF_REQUIRE(mixed_coarse && layer_coarse, "render_rays: coarse outputs are required");
    STNERF_REQUIRE(p->only_coarse || (mixed_fine && layer_fine), "render_rays: fine outputs are required");
    const int l = p->l, n1 = p->n1, n2 = p->n2, S = n1 + n2, rs = p->ray_stride;
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && n1 >= 3 && n2 >= 0, "render_rays: bad shape");
    STNERF_REQUIRE(rs >= (p->retiming ? 6 + l : 7), "render_rays: ray stride %d too small for the frame-id columns", rs);
    STNERF_REQUIRE(p->precision == 0 || p->precision == 2 || p->precision == 3, "render_rays: unknown precision %d", p->precision);
    STNERF_REQUIRE(nets->bkgd && (p->only_coarse || nets->bkgd_fine), "render_rays: background network missing");
    STNERF_REQUIRE(!p->bkgd_use_deform_time || nets->motion[0], "render_rays: bkgd_time_deform_net missing");
    STNERF_REQUIRE(!p->bkgd_use_space_time || p->use_space_time,
                   "render_rays: BKGD_USE_SPACE_TIME needs USE_SPACE_TIME (the reference passes the background its "
                   "frame id only then, layered_rfrender.py:382-390)");
    for (int i = 1; i < l; ++i) {
        if (!p->shown[i]) continue;
        STNERF_REQUIRE(nets->space[i] && (p->only_coarse || nets->space_fine[i]), "render_rays: SpaceNet of layer %d missing", i);
        STNERF_REQUIRE(!p->use_deform_time || nets->motion[i], "render_rays: MotionNet of layer %d missing", i);
    }
    if (o.layer_alpha)
        for (int i = 0; i < l; ++i)
            STNERF_REQUIRE(isfinite(o.layer_alpha[i]) && o.layer_alpha[i] >= 0.f,
                           "render_rays: layer_alpha[%d] = %g is not a finite, non-negative factor", i, (double)o.layer_alpha[i]);
    call->n_sampled = sampled_layers(l, o.samples);
    if (call->n_sampled) {
        STNERF_REQUIRE(p->precision != 2, "render_rays: the sample cull is not built for precision 2 (one launch per network)");
        STNERF_REQUIRE(!o.samples[0], "render_rays: layer 0 cannot be sample-culled (the background is never listed)");
        for (int i = 1; i < l; ++i)
            STNERF_REQUIRE(!o.samples[i] || (o.occ && o.occ[i].bits), "render_rays: layer %d is to be sample-culled but has no occupancy grid", i);
        STNERF_REQUIRE(S <= 256 && n <= ((int64_t)1 << 23), "render_rays: the sample cull packs (ray << 8 | k): n1 + n2 <= 256, n <= 2^23 per call");
        STNERF_REQUIRE(((uintptr_t)o.sample_counts & 7) == 0, "render_rays: sample counts must be 8-byte aligned");
    }
    const bool flagged = call->flagged = any_flag(l, o.terminate);
    STNERF_REQUIRE(!o.occluder_stops || flagged,
                   "render_rays: occluder_stops needs early ray termination on at least one layer (it lowers the stop depth the row lists test)");
    if (flagged) {
        STNERF_REQUIRE(o.tau >= 0.f && o.tau < 1.f, "render_rays: termination with tau = %g outside [0, 1)", (double)o.tau);
        STNERF_REQUIRE(p->precision != 2, "render_rays: termination is not built for precision 2 (one launch per network)");
        STNERF_REQUIRE(S <= 256 && n <= ((int64_t)1 << 23), "render_rays: termination packs (ray << 8 | k): n1 + n2 <= 256, n <= 2^23 per call");
        STNERF_REQUIRE(((uintptr_t)o.visibility_counts & 7) == 0, "render_rays: visibility counts must be 8-byte aligned");
        if (!p->only_coarse) {   // (only_coarse ignores both opacities and terminates nothing)
            STNERF_REQUIRE(o.layer_alpha || l <= 2 || p->alpha == 1.f,
                           "render_rays: termination with alpha = %g: the coarse composite ignores it, so its stop depth would be wrong", (double)p->alpha);
            for (int i = 0; o.layer_alpha && i < l; ++i)
                STNERF_REQUIRE(o.layer_alpha[i] == 1.f, "render_rays: termination with layer_alpha[%d] = %g: the coarse composite ignores it, so its stop depth would be wrong",
                               i, (double)o.layer_alpha[i]);
        }
    }
    const bool bg = call->bg = o.bkgd_grid && o.bkgd_grid->bits;
    if (bg) {
        const int brc = check_background_grid(o.bkgd_grid, "render_rays");
        if (brc) return brc;
        STNERF_REQUIRE(p->precision != 2, "render_rays: the background grid is not built for precision 2 (one launch per network)");
        STNERF_REQUIRE(S <= 256 && n <= ((int64_t)1 << 23), "render_rays: the background grid packs (ray << 8 | k): n1 + n2 <= 256, n <= 2^23 per call");
        STNERF_REQUIRE(((uintptr_t)o.bkgd_counts & 7) == 0, "render_rays: background counts must be 8-byte aligned");
    }
    if (o.bkgd_rays) {
        STNERF_REQUIRE(p->precision != 2, "render_rays: the per-ray background mask is not built for precision 2 (one launch per network)");
        STNERF_REQUIRE(S <= 256 && n <= ((int64_t)1 << 23),
                       "render_rays: the per-ray background mask packs (ray << 8 | k): n1 + n2 <= 256, n <= 2^23 per call");
        STNERF_REQUIRE(!o.cache || o.cache->mode == STNERF_BKGD_CACHE_OFF,
                       "render_rays: the per-ray background mask with a background cache in CAPTURE or REUSE: the cached raw would hold the zeros of one mask");
        STNERF_REQUIRE(((uintptr_t)o.bkgd_counts & 7) == 0, "render_rays: background counts must be 8-byte aligned");
    }
    const bool bg_rows = call->bg_rows = bg || o.bkgd_rays != nullptr;
    call->rows = make_row_plan(n, l, n1, n2, p->only_coarse, o.samples, o.terminate, bg_rows);
    const int64_t need = make_plan(n, l, n1, n2, p->only_coarse).bytes() + call->rows.bytes(n);
    STNERF_REQUIRE(workspace_bytes >= need, "render_rays: workspace of %lld B, need %lld", (long long)workspace_bytes,
                   (long long)need);
    const int cache_mode = call->cache_mode = o.cache ? o.cache->mode : STNERF_BKGD_CACHE_OFF;
    STNERF_REQUIRE(cache_mode == STNERF_BKGD_CACHE_OFF || cache_mode == STNERF_BKGD_CACHE_CAPTURE || cache_mode == STNERF_BKGD_CACHE_REUSE,
                   "render_rays: unknown background cache mode %d", cache_mode);
    if (cache_mode != STNERF_BKGD_CACHE_OFF) {
        STNERF_REQUIRE(o.cache->raw_coarse, "render_rays: background cache without raw_coarse");
        STNERF_REQUIRE(p->only_coarse || o.cache->raw_fine, "render_rays: background cache without raw_fine (required unless only_coarse)");
        STNERF_REQUIRE(((uintptr_t)o.cache->raw_coarse & 15) == 0 && (p->only_coarse || ((uintptr_t)o.cache->raw_fine & 15) == 0),
                       "render_rays: background cache buffers must be 16-byte aligned");
    }
    uint32_t lcap = 0, lreuse = 0;
    if (o.layers) {
        STNERF_REQUIRE(o.layers[0].mode == STNERF_LAYER_CACHE_OFF, "render_rays: layer cache entry 0 must be OFF (the background has its own cache)");
        STNERF_REQUIRE(((uintptr_t)o.mismatch & 7) == 0, "render_rays: the layer cache's mismatch counter must be 8-byte aligned");
        for (int i = 1; i < l; ++i) {
            const stnerf_layer_cache& e = o.layers[i];
            STNERF_REQUIRE(e.mode == STNERF_LAYER_CACHE_OFF || e.mode == STNERF_LAYER_CACHE_CAPTURE || e.mode == STNERF_LAYER_CACHE_REUSE,
                           "render_rays: unknown layer cache mode %d of layer %d", e.mode, i);
            if (e.mode == STNERF_LAYER_CACHE_OFF || !p->shown[i]) continue;
            STNERF_REQUIRE(e.raw_coarse && e.rays && e.count, "render_rays: layer cache entry %d without raw_coarse / rays / count", i);
            STNERF_REQUIRE(p->only_coarse || e.raw_fine, "render_rays: layer cache entry %d without raw_fine (required unless only_coarse)", i);
            STNERF_REQUIRE(((uintptr_t)e.raw_coarse & 15) == 0 && (p->only_coarse || ((uintptr_t)e.raw_fine & 15) == 0),
                           "render_rays: layer cache buffers of layer %d must be 16-byte aligned", i);
            STNERF_REQUIRE(e.capacity >= 0, "render_rays: layer cache entry %d with a negative capacity", i);
            (e.mode == STNERF_LAYER_CACHE_REUSE ? lreuse : lcap) |= 1u << i;
        }
    }
    call->lcap = lcap;
    call->lreuse = lreuse;
    // Not the background's while its raw outputs go to or come from the cache (they would depend on the performers), not a
    // performer's while they go to or come from the layer cache, not a hidden performer's (it is in no stage).
    call->term = 0;
    if (flagged && !p->only_coarse)
        for (int i = 0; i < l; ++i)
            if (o.terminate[i] && (i == 0 ? cache_mode == STNERF_BKGD_CACHE_OFF : p->shown[i] != 0 && !((lcap | lreuse) >> i & 1))) call->term |= 1u << i;
    if (o.occ) {
        const int orc = check_occupancy_table(o.occ, l, "render_rays");
        if (orc) return orc;
        STNERF_REQUIRE(((uintptr_t)o.counts & 7) == 0, "render_rays: occupancy counts must be 8-byte aligned");
    }
    call->prop = 0;
    if (proposal) {
        STNERF_REQUIRE(p->precision != 2, "render_rays: grid proposals are not built for precision 2 (the per-net schedule does not store activated colours)");
        STNERF_REQUIRE(n1 <= 256, "render_rays: grid proposals take n1 <= 256 coarse samples");
        for (int i = 0; i < l; ++i) {
            if (!proposal[i].sigma) continue;
            const int prc = check_density_grid(&proposal[i], i, "render_rays");
            if (prc) return prc;
            if (i == 0) {
                STNERF_REQUIRE(cache_mode == STNERF_BKGD_CACHE_OFF,
                               "render_rays: a grid proposal on layer 0 with the background cache in CAPTURE or REUSE (the cached coarse raw would be the grid's)");
                STNERF_REQUIRE(!bg_rows, "render_rays: a grid proposal on layer 0 with a background grid or a per-ray background mask (the coarse rows launch that "
                                         "stores their zeros is gone: out of scope)");
            } else {
                STNERF_REQUIRE(p->shown[i], "render_rays: a grid proposal on layer %d, which is hidden", i);
                STNERF_REQUIRE(!((lcap | lreuse) >> i & 1), "render_rays: a grid proposal on layer %d, whose layer cache entry is in CAPTURE or REUSE", i);
            }
            call->prop |= 1u << i;
        }
    }
    return STNERF_OK;
}

// The launches of one checked call with n > 0 rays, in stream order.  How each option acts:
// rot: the table reaches the sampler, the resampler and the ray-bias launches of both passes; everything else -- the stage
// kernels, the compositor, the workspace -- is what it is without one.
// scene_out: the in-scene layer passes of the final stage.  Their merged weights (n l ns floats) are written over that stage's
// points (xyz_c with only_coarse, else xyz_f: three times as large), which nobody reads once the stage's networks have run: the
// background cache's copies move `raw` only, the MotionNet reuse reads xyz_c BEFORE the fine stage and the fine compositor reads
// t_f / raw_f, neither of which overlaps xyz_f.
// layer_alpha: one density factor per layer for the FINE composite, or null = the reference's `if i == 2: density *= alpha`
// (p->alpha on layer 2).  A table replaces p->alpha; only_coarse ignores both.  Entries of `nets` may alias (include/stnerf.h):
// nothing below compares or groups network pointers.
// occ: the cull runs between the coarse sampler and the ray compaction and writes nothing but bit 0 of the mask: a culled (ray,
// performer) pair never reaches a network stage, and the compositor and the resampler treat it as they treat a ray that grazes
// the box.
// samples: a flagged layer's stages walk a row list (stnerf_occupancy_rows -> stnerf_mlp_stage_rows): the rows kernel runs right
// before each stage, on the points that stage is given, and stores the zeros of the samples it does not list.  In the fine pass
// that is after the resampler and after every MotionNet-reuse launch of the other layers: the zeros go into raw_f, which lies
// over t_c / xyz_c, and those launches read them.  A flagged layer is never in `reuse`: its MotionNet runs fused, on listed rows.
// terminate: with a flag set -- and a fine stage to apply it to -- the coarse composite also writes its merged weights, into
// xyz_f's region, which nobody writes before the resampler; stnerf_ray_stop turns them into t_stop (a region of its own: it must
// survive to the fine stage), and a flagged layer's fine row list comes from stnerf_visibility_rows, at the place and time
// stnerf_occupancy_rows makes a sample-culled layer's.  The coarse stage is untouched.  Layer 0 is listed with ray_list == NULL
// (every ray): the row-list stage kernels address points, outputs and the ray-bias row by the word's ray, and the ray-bias launch
// of a layer without a list fills every ray's row.
// bkgd_grid: with bits, layer 0 is sample-culled in every stage it is evaluated in: stnerf_background_rows runs over EVERY ray (no
// mask bit is consulted: evaluated[0] == 2) on the points the stage is given -- xyz_c after the compaction, xyz_f after the
// resampler and every MotionNet-reuse launch, since the zeros land in raw_f over t_c / xyz_c -- and the stage walks layer 0's row
// list.  Where layer 0's fine stage is terminated too the same launch takes t_f / t_stop, in place of stnerf_visibility_rows, and
// the two share the list.  A background cache REUSE frame makes no rows launch (layer 0 is in no stage); a CAPTURE frame is culled
// by the grid and still not terminated, so the cached raw is a function of view and grid only.
// bkgd_rays: the same rows launch with one more test in front, the ray's byte (stnerf_background_ray_rows), run wherever the grid's
// runs and also without a grid; a masked ray's layer-0 samples get their zeros in both stages and are on no list.  The background
// cache is refused in CAPTURE and REUSE (check_call): the cached raw would hold the zeros of one mask.
// layers: a performer's raw outputs are a function of the view and of its own inputs, as the background's are, so a layer in REUSE
// is in no network stage: no stage item, no stand-alone MotionNet or MotionNet-reuse fill (its `reuse` bit is cleared), no ray-bias
// and no rows launch -- its slices are copied in by stnerf_copy_layer_raw_listed where the background's are, for the rays the slice
// was captured on.  A layer in CAPTURE renders as usual and is copied out after each stage; the coarse copy keeps the frame's ray
// list, the fine one walks the kept list.  Neither is terminated (its `term` bit is cleared: the raw outputs would depend on the
// other layers).  Everything else runs for every layer in every mode.
// occluder: the final stage's scene pass is followed by stnerf_scene_occluder on the same buffers -- t, raw and the merged weights,
// which lie over that stage's points and stay live until the call returns.  occluder_stops: an opaque row's depth is folded into
// t_stop right after stnerf_ray_stop, so the flagged layers' row lists leave out the fine samples behind it.
// proposal: a flagged layer is in no COARSE network stage, as a layer in REUSE is in none: no stage item, no rows launch, no ray-bias,
// no stand-alone MotionNet (its `reuse` bit is cleared: there are no moved coarse points, the fine MotionNet runs fused on all n1 + n2
// rows).  Its slice of raw_c is filled by stnerf_proposal_density right after the coarse stage and the caches' copies, on the
// layer's hit rays (layer 0: every ray) and on the points the coarse stage would have been given.  From the coarse composite on the
// call is what it is without the option; a sample-culled flagged layer is culled in the fine stage only.
// An option that is absent (a null table, no flag set, no bits, every mode OFF) adds no launch and changes none.
int launch_sequence(RENDER_PARAMS, const stnerf_render_options& o, const stnerf_render_options_deep* deep, const stnerf_density_grid* proposal, const Call& c,
                    const Plan& pl, const Workspace& w, stnerf_stream_t stream) {
    const int l = p->l, n1 = p->n1, n2 = p->n2, S = n1 + n2, rs = p->ray_stride;
    const bool cached = c.cache_mode == STNERF_BKGD_CACHE_REUSE;   // layer 0's network outputs come from the cache
    const uint32_t lcap = c.lcap, lreuse = c.lreuse, term = c.term, prop = c.prop;
    const int64_t row_cap = c.rows.row_cap;
    hipStream_t st = as_stream(stream);
    int rc;

    // ---- coarse samples + hit masks (+ un-edit), then the per-layer lists of hit rays
    rc = stnerf_sample_coarse_rot(rays, n, rs, boxes, box_ray_stride, l, n1, jitter, p->seed, p->ray_index_base,
                                  p->ray_index_stripe, p->ray_index_period,
                                  p->has_edits ? p->edits_coarse : nullptr, p->pivot, o.rot, w.t_c, w.xyz_c, mask, stream);
    if (rc) return rc;
    if (o.occ) {   // (before the compaction: a culled pair is on no list)
        rc = stnerf_occupancy_cull(w.xyz_c, n, l, n1, o.occ, mask, o.counts, stream);
        if (rc) return rc;
    }
    if (hipMemsetAsync(w.ray_count, 0, sizeof(int32_t) * pl.count, st) != hipSuccess) {
        set_error("render_rays: hipMemsetAsync failed");
        return STNERF_ELAUNCH;
    }
    rc = stnerf_compact_rays(mask, n, l, w.ray_list, w.ray_count, stream);
    if (rc) return rc;

    // ---- the performer layers whose MotionNet runs on its own (MotionNet reuse, above): split-bf16 stages, both passes, the same
    // box edit in both (STNERF_MOTION_REUSE=0: every layer fused, for A/B runs and tests)
    uint32_t reuse = 0;
    if (p->precision == 3 && !p->only_coarse && p->use_deform_time) {
        const char* sw = getenv("STNERF_MOTION_REUSE");
        if (!(sw && sw[0] == '0'))
            for (int i = 1; i < l; ++i)
                if (p->shown[i] && !w.row_list[i] && !((lreuse | prop) >> i & 1) && (!p->has_edits || memcmp(&p->edits_coarse[i], &p->edits_fine[i], sizeof(stnerf_layer_edit)) == 0))
                    reuse |= 1u << i;
    }
    uint32_t* motion_queue = reinterpret_cast<uint32_t*>(w.ray_count + STNERF_MAX_LAYERS + 2);   // [layer][coarse, fine]

    // ---- one network stage: deform + evaluate every shown layer on its hit rays (:340-418 / :495-576)
    auto stage = [&](float* xyz, float* raw, int ns, bool fine, uint32_t moved) -> int {
        const int64_t xs = (int64_t)l * ns * 3, ws_ = (int64_t)l * ns * 4;
        if (p->precision == 0 || p->precision == 3) {
            // exact f32 / bf16x3: ONE persistent launch over every shown layer (csrc/stage_entry.hip); deformed performers
            // first, the background last
            stnerf_stage_layer sl[STNERF_MAX_LAYERS];
            stnerf_stage_rows sr[STNERF_MAX_LAYERS];
            memset(sr, 0, sizeof(sr));
            int ns_l = 0;
            bool any_list = false;
            for (int pass = 0; pass < 2; ++pass) {
                for (int i = cached ? 1 : 0; i < l; ++i) {
                    if (i > 0 && (!p->shown[i] || (lreuse >> i & 1))) continue;   // (hidden, or from the layer cache)
                    if (!fine && (prop >> i & 1)) continue;                          // (a grid proposal: in no coarse stage)
                    const bool deform = i == 0 ? p->bkgd_use_deform_time != 0 : p->use_deform_time != 0;
                    if ((pass == 0) != deform) continue;
                    const bool timed = (i > 0 ? 1 : p->bkgd_use_space_time) && p->use_space_time;
                    stnerf_stage_layer& e = sl[ns_l++];
                    e.space = i == 0 ? (fine ? nets->bkgd_fine : nets->bkgd) : (fine ? nets->space_fine[i] : nets->space[i]);
                    e.motion = deform && !(moved >> i & 1) ? nets->motion[i] : nullptr;   // (moved: points deformed already)
                    e.ray_list = i == 0 ? nullptr : w.ray_list + (int64_t)i * n;
                    e.ray_count = i == 0 ? nullptr : w.ray_count + i;
                    e.xyz = xyz + (int64_t)i * ns * 3;
                    e.raw = raw + (int64_t)i * ns * 4;
                    e.times = (timed || deform) ? rays + (p->retiming ? 6 + i : 6) : nullptr;
                    e.use_time = timed ? 1 : 0;
                    e.motion_flags = i == 0 ? STNERF_MOTION_PLAIN_TIME : 0;
                    e.rotation = o.rot ? o.rot + i : nullptr;
                    const bool culled = o.samples && o.samples[i];
                    if (i == 0 && c.bg_rows) {   // the background's grid: every ray; with termination the same launch drops the hidden samples
                        const bool stop = fine && (term & 1);
                        const int r1 = o.bkgd_rays   // the per-ray mask: the same launch with the ray's byte in front, the grid optional
                                           ? stnerf_background_ray_rows(n, e.xyz, xs, ns, c.bg ? o.bkgd_grid : nullptr, stop ? w.t_f : nullptr, (int64_t)l * ns,
                                                                        stop ? w.t_stop : nullptr, e.raw, ws_, w.row_list[0], row_cap, w.row_count, o.bkgd_counts,
                                                                        o.bkgd_rays, stream)
                                           : stnerf_background_rows(n, e.xyz, xs, ns, o.bkgd_grid, stop ? w.t_f : nullptr, (int64_t)l * ns, stop ? w.t_stop : nullptr,
                                                                    e.raw, ws_, w.row_list[0], row_cap, w.row_count, o.bkgd_counts, stream);
                        if (r1) return r1;
                    } else if (fine && (term >> i & 1)) {   // termination: the rows that are not hidden (and, sample-culled too, in an occupied cell)
                        const int r1 = stnerf_visibility_rows(e.ray_list, e.ray_count, n, i, e.xyz, xs, w.t_f + (int64_t)i * ns, (int64_t)l * ns, w.t_stop, ns,
                                                              culled ? o.occ + i : nullptr, e.raw, ws_, w.row_list[i], row_cap, w.row_count + i,
                                                              o.visibility_counts, stream);
                        if (r1) return r1;
                    } else if (culled) {   // the sample cull: this layer's rows of this stage, and the zeros of the others
                        const int r1 = stnerf_occupancy_rows(e.ray_list, e.ray_count, n, i, e.xyz, xs, ns, o.occ + i, e.raw, ws_, w.row_list[i], row_cap,
                                                             w.row_count + i, o.sample_counts, stream);
                        if (r1) return r1;
                    } else {
                        continue;
                    }
                    sr[ns_l - 1].row_list = w.row_list[i];
                    sr[ns_l - 1].row_count = w.row_count + i;
                    any_list = true;
                }
            }
            if (ns_l == 0) return STNERF_OK;   // (every evaluated layer comes from a cache: nothing to evaluate)
            set_launch_tag(fine ? 1 : 0);
            const int r2 = stnerf_mlp_stage_rows(sl, any_list ? sr : nullptr, ns_l, n, ns, rays + 3, rs, rs, xs, ws_,
                                                 (p->deep_rgb ? STNERF_STAGE_DEEP_RGB : 0) | STNERF_STAGE_SIGMOID_RGB | (p->precision == 3 ? STNERF_STAGE_BF16X3 : 0),
                                                 reinterpret_cast<uint32_t*>(w.ray_count + STNERF_MAX_LAYERS + (fine ? 1 : 0)), w.ray_bias, stream);
            set_launch_tag(-1);
            return r2;
        }
        // precision 2: one launch per network through the op-level entries -- the same exact-f32 wave arithmetic, scheduled
        // network by network (the deformed points go back to xyz in between)
        for (int i = cached ? 1 : 0; i < l; ++i) {
            if (i == 0 ? !p->bkgd_use_deform_time : !p->use_deform_time) continue;
            if (i > 0 && (!p->shown[i] || (lreuse >> i & 1))) continue;  // a hidden layer's points are never consumed, a cached layer's neither
            set_launch_tag(i);
            // performers: time_deform_nets[i-1] on the hit rays, fractional frame ids lerp the encodings (:340-356);
            // background: bkgd_time_deform_net on every ray, MotionNet(input_time=False) (:358-367)
            const float* times = rays + (p->retiming ? 6 + i : 6);
            const int32_t* lst = i == 0 ? nullptr : w.ray_list + (int64_t)i * n;
            const int32_t* cnt = i == 0 ? nullptr : w.ray_count + i;
            const int flags = STNERF_MOTION_ADD_TO_XYZ | (i == 0 ? STNERF_MOTION_PLAIN_TIME : 0);
            const int r2 = stnerf_motionnet_fwd(nets->motion[i], n, ns, lst, cnt, xyz + (int64_t)i * ns * 3, xs, times,
                                                      rs, nullptr, 0, flags, stream);
            if (r2) return r2;
        }
        for (int i = cached ? 1 : 0; i < l; ++i) {
            if (i > 0 && (!p->shown[i] || (lreuse >> i & 1))) continue;
            set_launch_tag(i);
            const void* net = i == 0 ? (fine ? nets->bkgd_fine : nets->bkgd) : (fine ? nets->space_fine[i] : nets->space[i]);
            const bool timed = (i > 0 ? 1 : p->bkgd_use_space_time) && p->use_space_time;
            const int kind = timed ? (p->deep_rgb ? STNERF_NET_SPACE_TIME_DEEP : STNERF_NET_SPACE_TIME)
                                   : (p->deep_rgb ? STNERF_NET_SPACE_DEEP : STNERF_NET_SPACE);
            const float* times = timed ? rays + (p->retiming ? 6 + i : 6) : nullptr;
            const int32_t* lst = i == 0 ? nullptr : w.ray_list + (int64_t)i * n;
            const int32_t* cnt = i == 0 ? nullptr : w.ray_count + i;
            const int r2 = stnerf_spacenet_fwd_rot(kind, net, n, ns, lst, cnt, xyz + (int64_t)i * ns * 3, xs, rays + 3, rs, times, rs,
                                                   raw + (int64_t)i * ns * 4, ws_, w.ray_bias + (int64_t)i * n * 128, o.rot ? o.rot + i : nullptr,
                                                   stream);
            if (r2) return r2;
        }
        set_launch_tag(-1);
        return STNERF_OK;
    };
    for (int i = 1; i < l; ++i) {
        if (!(reuse >> i & 1)) continue;
        rc = motion_rows(nets, p, rays, n, i, n1, n1, w.xyz_c, w.ray_list, w.ray_count, nullptr, 0, motion_queue + 2 * i, st);
        if (rc) return rc;
    }
    // The stage followed by the caches' copies: layer 0's slice (the background cache) and the cached performers' (the layer cache,
    // compact: the hit rays only) out of `raw` after a capture frame's stage, into it in place of the stage's items in a reuse frame.
    auto stage_and_cache = [&](float* xyz, float* raw, int ns, bool fine, float* kept) -> int {
        const int r2 = stage(xyz, raw, ns, fine, reuse);
        if (r2) return r2;
        if (c.cache_mode != STNERF_BKGD_CACHE_OFF) {
            set_launch_tag(0);
            const int r3 = stnerf_copy_layer_raw(raw, n, l, 0, ns, kept, c.cache_mode == STNERF_BKGD_CACHE_CAPTURE, stream);
            set_launch_tag(-1);
            if (r3) return r3;
        }
        for (int i = 1; i < l; ++i) {
            if (!((lcap | lreuse) >> i & 1)) continue;
            const stnerf_layer_cache& e = o.layers[i];
            const bool capture = lcap >> i & 1;
            // (the fine capture walks the list the coarse one kept: list and count alias the entry's and stay as they are)
            const int32_t* lst = capture && fine ? e.rays : w.ray_list + (int64_t)i * n;
            const int32_t* cnt = capture && fine ? e.count : w.ray_count + i;
            set_launch_tag(i);
            const int r3 = stnerf_copy_layer_raw_listed(raw, n, l, i, ns, lst, cnt, fine ? e.raw_fine : e.raw_coarse, e.rays, e.count, e.capacity,
                                                        capture ? 1 : 0, capture ? nullptr : o.mismatch, stream);
            set_launch_tag(-1);
            if (r3) return r3;
        }
        return STNERF_OK;
    };
    // (raw_f lies over the whole coarse block: the coarse slice is copied here, before the compositor reads raw_c)
    rc = stage_and_cache(w.xyz_c, w.raw_c, n1, false, o.cache ? o.cache->raw_coarse : nullptr);
    if (rc) return rc;
    for (int i = 0; i < l; ++i) {   // grid proposals: the flagged layers' coarse densities
        if (!(prop >> i & 1)) continue;
        rc = stnerf_proposal_density(i == 0 ? nullptr : w.ray_list + (int64_t)i * n, i == 0 ? nullptr : w.ray_count + i, n, i, w.xyz_c + (int64_t)i * n1 * 3,
                                     (int64_t)l * n1 * 3, n1, proposal + i, w.raw_c + (int64_t)i * n1 * 4, (int64_t)l * n1 * 4, stream);
        if (rc) return rc;
    }

    // ---- coarse: density edits, per-layer + merged composite (:414-448)
    stnerf_composite_params cp;
    memset(&cp, 0, sizeof(cp));
    cp.border = p->border;
    cp.near = p->near;
    cp.fine = 0;
    cp.cut_negative_t = 1;
    cp.rgb_activated = p->precision == 0 || p->precision == 3;  // the persistent stage kernels store sigmoid(rgb)
    for (int i = 0; i < STNERF_MAX_LAYERS; ++i) {
        cp.sigma_scale[i] = 1.f;
        cp.evaluated[i] = i < l ? (i == 0 ? 2 : p->shown[i]) : 1;  // background: every ray, mask or not (:382-392)
        cp.use_threshold[i] = (p->retiming && i >= 1) ? 1 : 0;  // :416-418 (performers, retiming only)
        cp.threshold[i] = p->density_threshold;
    }
    const bool scene_coarse = o.scene_out && p->only_coarse;   // (xyz_c is dead: the coarse networks have run)
    // (termination: the merged weights go where the fine points will be -- scene_coarse is only_coarse, which terminates nothing)
    rc = stnerf_composite_scene(w.t_c, w.raw_c, mask, n, l, n1, &cp, layer_coarse, mixed_coarse, p->only_coarse ? nullptr : w.w_c,
                                nullptr, w.ray_flags, scene_coarse ? w.xyz_c : (term ? w.xyz_f : nullptr), scene_coarse ? o.scene_out : nullptr, stream);
    if (rc) return rc;
    if (p->only_coarse) {
        if (o.occluder) {   // (the coarse stage is the final one: its merged weights lie in xyz_c)
            rc = stnerf_scene_occluder(w.t_c, w.raw_c, mask, w.xyz_c, n, l, n1, &cp, o.scene_out, mixed_coarse, o.occluder, o.occluded_mixed, o.occluded_scene,
                                       o.occluder_share, nullptr, nullptr, stream);
            if (rc) return rc;
        }
        if (deep) {
            rc = launch_deep(*deep, w.t_c, w.raw_c, mask, w.xyz_c, n, l, n1, &cp, stream);
            if (rc) return rc;
        }
        return clear_mask_hints(mask, n * l, as_stream(stream));
    }
    if (term) {   // (before the resampler overwrites the weights with the fine points)
        rc = stnerf_ray_stop(w.t_c, w.xyz_f, n, l, n1, o.tau, w.t_stop, stream);
        if (rc) return rc;
        if (o.occluder_stops) {   // an opaque occluder in front of the stop depth is the stop depth
            rc = stnerf_occluder_stop(o.occluder, n, w.t_stop, stream);
            if (rc) return rc;
        }
    }

    // ---- resample + fine points (:459-475), fine networks, fine composite (:538-606)
    rc = stnerf_resample_rot(w.t_c, w.w_c, n, l, n1, n2, u, p->seed, p->ray_index_base, p->ray_index_stripe, p->ray_index_period,
                             rays, rs,
                             p->has_edits ? p->edits_fine : nullptr, p->pivot, o.rot, mask, w.t_f, w.xyz_f, nullptr, nullptr, nullptr, stream);
    if (rc) return rc;
    for (int i = 1; i < l; ++i) {   // (xyz_c and t_c lie under raw_f: read here, before the fine stage)
        if (!(reuse >> i & 1)) continue;
        hipLaunchKernelGGL(motion_reuse_fill_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, st, w.t_c, w.xyz_c, w.t_f, w.xyz_f,
                           w.ray_list + (int64_t)i * n, w.ray_count + i, n, l, i, n1, n2, w.slots);
        STNERF_CHECK_LAUNCH("render_rays (MotionNet reuse)");
        if (n2 == 0) continue;
        rc = motion_rows(nets, p, rays, n, i, n2, S, w.xyz_f, w.ray_list, w.ray_count, w.slots, n2, motion_queue + 2 * i + 1, st);
        if (rc) return rc;
    }
    // (the cached fine slice lands on t_c / xyz_c: after the MotionNet reuse launches above have read them)
    rc = stage_and_cache(w.xyz_f, w.raw_f, S, true, o.cache ? o.cache->raw_fine : nullptr);
    if (rc) return rc;
    cp.fine = 1;
    cp.cut_negative_t = 0;
    for (int i = 0; i < STNERF_MAX_LAYERS; ++i) {
        cp.use_threshold[i] = p->retiming ? 1 : 0;                       // :538-547 (bkgd), :564-566 (performers)
        cp.threshold[i] = i == 0 ? p->bkgd_density_threshold : p->density_threshold;
    }
    if (o.layer_alpha)
        for (int i = 0; i < l; ++i) cp.sigma_scale[i] = o.layer_alpha[i];
    else if (l > 2)
        cp.sigma_scale[2] = p->alpha;                                    // :575-576
    rc = stnerf_composite_scene(w.t_f, w.raw_f, mask, n, l, S, &cp, layer_fine, mixed_fine, nullptr, nullptr, w.ray_flags,
                                o.scene_out ? w.xyz_f : nullptr, o.scene_out, stream);
    if (rc) return rc;
    if (o.occluder) {   // (xyz_f holds the fine merged weights)
        rc = stnerf_scene_occluder(w.t_f, w.raw_f, mask, w.xyz_f, n, l, S, &cp, o.scene_out, mixed_fine, o.occluder, o.occluded_mixed, o.occluded_scene,
                                   o.occluder_share, nullptr, nullptr, stream);
        if (rc) return rc;
    }
    if (deep) {
        rc = launch_deep(*deep, w.t_f, w.raw_f, mask, w.xyz_f, n, l, S, &cp, stream);
        if (rc) return rc;
    }
    return clear_mask_hints(mask, n * l, as_stream(stream));
}

}  // namespace

extern "C" int stnerf_render_rays_opts(RENDER_PARAMS, const stnerf_render_options* opts, stnerf_stream_t stream) {
    const int src = check_options_size(opts, "render_rays");
    if (src) return src;
    const stnerf_render_options& o = opts ? *opts : kNoOptions;
    const stnerf_render_options_deep* deep = deep_options(opts);
    const stnerf_density_grid* proposal = p ? proposal_options(opts, p->l) : nullptr;
    Call call;
    const int rc = check_call(RENDER_ARGS, o, deep, proposal, &call);
    if (rc) return rc;
    if (n == 0) return STNERF_OK;
    const Plan pl = make_plan(n, p->l, p->n1, p->n2, p->only_coarse);
    const Workspace w(workspace, workspace_bytes, pl, call.rows, n, p->l);
    return launch_sequence(RENDER_ARGS, o, deep, proposal, call, pl, w, stream);
}

// ---- the fixed-argument forms (include/stnerf.h): each names the options up to the one it introduced, in the record's order, and
// leaves the rest zero
#define RENDER_ENTRY(name, params, ...)                                                \
    extern "C" int name(RENDER_PARAMS, params stnerf_stream_t stream) {                \
        const stnerf_render_options o = {(int32_t)sizeof(stnerf_render_options), __VA_ARGS__}; \
        return stnerf_render_rays_opts(RENDER_ARGS, &o, stream);                       \
    }
#define P(...) __VA_ARGS__,
extern "C" int stnerf_render_rays(RENDER_PARAMS, stnerf_stream_t stream) { return stnerf_render_rays_opts(RENDER_ARGS, nullptr, stream); }
RENDER_ENTRY(stnerf_render_rays_cached, P(const stnerf_bkgd_cache* cache), cache)
RENDER_ENTRY(stnerf_render_rays_rot, P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot), cache, rot)
RENDER_ENTRY(stnerf_render_rays_scene, P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out), cache, rot, scene_out)
RENDER_ENTRY(stnerf_render_rays_opacity, P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out, const float* layer_alpha),
             cache, rot, scene_out, layer_alpha)
RENDER_ENTRY(stnerf_render_rays_occupancy,
             P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out, const float* layer_alpha,
               const stnerf_occupancy* occ, int32_t* counts),
             cache, rot, scene_out, layer_alpha, occ, counts)
RENDER_ENTRY(stnerf_render_rays_samples,
             P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out, const float* layer_alpha,
               const stnerf_occupancy* occ, int32_t* counts, const int32_t* samples, int64_t* sample_counts),
             cache, rot, scene_out, layer_alpha, occ, counts, samples, sample_counts)
RENDER_ENTRY(stnerf_render_rays_terminated,
             P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out, const float* layer_alpha,
               const stnerf_occupancy* occ, int32_t* counts, const int32_t* samples, int64_t* sample_counts, float tau,
               const int32_t* terminate, int64_t* visibility_counts),
             cache, rot, scene_out, layer_alpha, occ, counts, samples, sample_counts, tau, terminate, visibility_counts)
RENDER_ENTRY(stnerf_render_rays_background,
             P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out, const float* layer_alpha,
               const stnerf_occupancy* occ, int32_t* counts, const int32_t* samples, int64_t* sample_counts, float tau,
               const int32_t* terminate, int64_t* visibility_counts, const stnerf_occupancy* bkgd_grid, int64_t* bkgd_counts),
             cache, rot, scene_out, layer_alpha, occ, counts, samples, sample_counts, tau, terminate, visibility_counts, bkgd_grid, bkgd_counts)
RENDER_ENTRY(stnerf_render_rays_layers,
             P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out, const float* layer_alpha,
               const stnerf_occupancy* occ, int32_t* counts, const int32_t* samples, int64_t* sample_counts, float tau,
               const int32_t* terminate, int64_t* visibility_counts, const stnerf_occupancy* bkgd_grid, int64_t* bkgd_counts,
               const stnerf_layer_cache* layers, int64_t* mismatch),
             cache, rot, scene_out, layer_alpha, occ, counts, samples, sample_counts, tau, terminate, visibility_counts, bkgd_grid, bkgd_counts,
             layers, mismatch)
RENDER_ENTRY(stnerf_render_rays_occluded,
             P(const stnerf_bkgd_cache* cache, const stnerf_layer_rotation* rot, float* scene_out, const float* layer_alpha,
               const stnerf_occupancy* occ, int32_t* counts, const int32_t* samples, int64_t* sample_counts, float tau,
               const int32_t* terminate, int64_t* visibility_counts, const stnerf_occupancy* bkgd_grid, int64_t* bkgd_counts,
               const stnerf_layer_cache* layers, int64_t* mismatch, const float* occluder, int32_t occluder_stops, float* occluded_mixed,
               float* occluded_scene, float* occluder_share),
             cache, rot, scene_out, layer_alpha, occ, counts, samples, sample_counts, tau, terminate, visibility_counts, bkgd_grid, bkgd_counts,
             layers, mismatch, occluder, occluder_stops, occluded_mixed, occluded_scene, occluder_share)
#undef P
#undef RENDER_ENTRY

// the named size queries: `background` != 0 stands for a grid with bits
static int64_t workspace_bytes_of(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples, const int32_t* terminate, int background) {
    static const uint32_t some_bits = 0;
    const stnerf_occupancy grid = {&some_bits};
    stnerf_render_options o = kNoOptions;
    o.samples = samples;
    o.terminate = terminate;
    o.bkgd_grid = background ? &grid : nullptr;
    return stnerf_render_workspace_bytes_opts(n, l, n1, n2, only_coarse, &o);
}
extern "C" int64_t stnerf_render_workspace_bytes(int64_t n, int l, int n1, int n2, int only_coarse) {
    return workspace_bytes_of(n, l, n1, n2, only_coarse, nullptr, nullptr, 0);
}
extern "C" int64_t stnerf_render_workspace_bytes_samples(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples) {
    return workspace_bytes_of(n, l, n1, n2, only_coarse, samples, nullptr, 0);
}
extern "C" int64_t stnerf_render_workspace_bytes_terminated(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples,
                                                            const int32_t* terminate) {
    return workspace_bytes_of(n, l, n1, n2, only_coarse, samples, terminate, 0);
}
extern "C" int64_t stnerf_render_workspace_bytes_background(int64_t n, int l, int n1, int n2, int only_coarse, const int32_t* samples,
                                                            const int32_t* terminate, int background) {
    return workspace_bytes_of(n, l, n1, n2, only_coarse, samples, terminate, background);
}
