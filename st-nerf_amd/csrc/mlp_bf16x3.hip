// The split-bf16 ("bf16x3") kernels of the render path, on the machinery of mlp_bf16x3_core.h (the design is described there): the
// persistent stage kernel (mlp_bf16x3_stage_kernel<DEEP, NoTapArgs>; with the training tap: <false, StoreTapArgs>) and the stage
// kernel's MotionNet alone (mlp_bf16x3_motion_kernel).  The backward chain: train_bf16x3.hip; the packers: pack_bf16x3.hip.
//
// Reference: modeling/spacenet.py:16-160, modeling/motion_net.py:7-71, modeling/layered_rfrender.py:340-418,495-576.
#include "mlp_bf16x3_core.h"

namespace stnerf {

#ifdef STNERF_BX_PROF
static __device__ unsigned long long g_bxphase[16];   // per-phase clocks of both kernels of this file (BXP: mlp_bf16x3_core.h)
#endif

// does this wave issue every store of a boundary?  (some row of its 32 inside the launch, mask planes wanted)
__device__ __forceinline__ bool tap_wave_stores(const BxStoreTap& tap, const StoreTapArgs& t) {
    return (uint32_t)(tap.wave * WV_ROWS) < tap.nrows && t.bits != nullptr;
}
__device__ __forceinline__ BxNoTap make_bx_tap(const NoTapArgs&, uint32_t, int64_t, int) { return BxNoTap(); }
__device__ __forceinline__ BxStoreTap make_bx_tap(const StoreTapArgs& t, uint32_t item, int64_t rows, int wave) {
    // (training launches one network: items of queue slot 0 are rows 128 item ..)
    const int64_t left = rows - (int64_t)item * WV_ITEM;
    return BxStoreTap{&t, item * (uint32_t)WV_ITEM, (uint32_t)(left < WV_ITEM ? left : WV_ITEM), wave};
}

// The tap variant (training: ONE SpaceNet on every ray, no MotionNet, no ray list) gives the tap's stores the registers they need
// by not carrying per-row values through the item: the next item's (ray, sample) is located where it is fetched, not at the
// top of the item; this item's output offset is recomputed from its ray at the end; the MotionNet path is compiled out.
template <bool DEEP, class TapArgs>
__global__ __launch_bounds__(WV_THREADS, 1) void mlp_bf16x3_stage_kernel(StageArgs a, TapArgs targs) {
    constexpr bool TAP = !std::is_same<TapArgs, NoTapArgs>::value;
    extern __shared__ __attribute__((aligned(16))) char smem_bx[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* ring = smem_bx;
    float* encw = reinterpret_cast<float*>(smem_bx + BX_LDS_RING) + wave * WV_ENC_FLOATS;
    float* cs = reinterpret_cast<float*>(smem_bx + BX_LDS_RING + BX_LDS_ENC);
    float* cm = cs + BX_CONST_SPACE;
    uint32_t* qslot = reinterpret_cast<uint32_t*>(smem_bx + BX_LDS_RING + BX_LDS_ENC + BX_LDS_CONST);
    int64_t* lrows = reinterpret_cast<int64_t*>(qslot + 4);
    // ---- the queue (as in mlp_wave.hip): items (128 rows) of layer slot j are [pre[j], pre[j+1]).  The prefix table lives in
    // LDS, not in 17 SGPRs: this kernel's scalar registers are short (the stream state, the kernel arguments), and what does
    // not fit is kept in VGPR lanes -- of which it has none to spare either.
    uint32_t* lpre = reinterpret_cast<uint32_t*>(lrows + STNERF_MAX_LAYERS);
    uint32_t total = 0;
#pragma unroll 1
    for (int j = 0; j < a.n_layers; ++j) {
        const int64_t rows = layer_rows(a.layer[j], a.n_rays, a.ns);
        if (tid == 0) {
            lrows[j] = rows;
            lpre[j] = total;
        }
        total += (uint32_t)((rows + WV_ITEM - 1) / WV_ITEM);
    }
    // (layer slot, first item of that slot) of an item: wave-uniform
    auto locate = [&](uint32_t item, int& slot, uint32_t& base) {
        slot = 0;
        base = 0;
#pragma unroll 1
        for (int j = 1; j < a.n_layers; ++j) {
            const uint32_t pj = (uint32_t)__builtin_amdgcn_readfirstlane((int)lpre[j]);
            if (item >= pj) {
                slot = j;
                base = pj;
            }
        }
    };
    auto slot_of = [&](uint32_t item) {
        int s_;
        uint32_t b_;
        locate(item, s_, b_);
        return s_;
    };
    auto base_of = [&](uint32_t item) {
        int s_;
        uint32_t b_;
        locate(item, s_, b_);
        return b_;
    };
    auto row_of = [&](uint32_t item, RowRef& rr) {
        rr = RowRef{0, 0, false};
        if (item >= total) return;
        const int s = slot_of(item);
        const int64_t rows = lrows[s];
        const int64_t row = (int64_t)(item - base_of(item)) * WV_ITEM + wave * WV_ROWS + (lane & 31);
        rr.valid = row < rows;
        if (rr.valid) {
            int64_t rslot;
            if (rows <= 0x7fffffffll) {
                const uint32_t q = (uint32_t)row / (uint32_t)a.ns;
                rslot = q;
                rr.k = (int)((uint32_t)row - q * (uint32_t)a.ns);
            } else {
                rslot = row / a.ns;
                rr.k = (int)(row - rslot * a.ns);
            }
            const int32_t* rl = a.layer[s].ray_list;
            rr.ray = rl ? (int64_t)rl[rslot] : rslot;
        }
    };
    auto fetch = [&](uint32_t item, const RowRef& rr, WaveInputs& in) {
        in.valid = rr.valid;
        in.raw_off = 0;
        in.ray = 0;
        in.tv = 0.f;
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) in.p[c3] = 0.f;
        if (rr.valid) {
            const StageLayer& ly = a.layer[slot_of(item)];
            const float* src = ly.xyz + rr.ray * a.xyz_ray_stride + 3 * rr.k;
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) in.p[c3] = src[c3];
            if (ly.motion) in.tv = ly.times[rr.ray * a.times_ray_stride];
            in.raw_off = rr.ray * a.raw_ray_stride + 4 * rr.k;
            in.ray = (int32_t)rr.ray;
        }
    };
    // the weight streams of an item's networks
    const int64_t sp_kind_stream[2] = {bx_layout(DEEP ? STNERF_NET_SPACE_DEEP : STNERF_NET_SPACE).stream_off,
                                       bx_layout(DEEP ? STNERF_NET_SPACE_TIME_DEEP : STNERF_NET_SPACE_TIME).stream_off};
    const int64_t mo_stream = bx_layout(STNERF_NET_MOTION).stream_off;
    auto segs_of = [&](uint32_t item, Seg& m, Seg& s) {
        m = Seg{nullptr, 0u};
        s = Seg{nullptr, 0u};
        if (item >= total) return;
        const StageLayer& ly = a.layer[slot_of(item)];
        s.p = reinterpret_cast<const char*>(ly.space) + sp_kind_stream[ly.use_time ? 1 : 0];
        s.left = (uint32_t)bx_space_slots(DEEP);
        if (ly.motion) {
            m.p = reinterpret_cast<const char*>(ly.motion) + mo_stream;
            m.left = (uint32_t)bx_motion_slots();
        }
    };

    // ---- prime the pipeline: two items popped, the first one's inputs loaded, three slots of its stream in flight
    if (tid == 0) {
        qslot[0] = atomicAdd(a.queue, 1u);
        qslot[1] = atomicAdd(a.queue, 1u);
    }
    __syncthreads();
    uint32_t it0 = __builtin_amdgcn_readfirstlane(qslot[0]);
    uint32_t it1 = __builtin_amdgcn_readfirstlane(qslot[1]);
    __syncthreads();
    if (it0 >= total) return;  // (uniform)
    WaveInputs cur, nxt;
    {
        RowRef rr;
        row_of(it0, rr);
        fetch(it0, rr, cur);
    }
    Ctx cx;
    ring_init(cx, ring, wave, lane);
    cx.st_on = false;
    segs_of(it0, cx.seg[0], cx.seg[1]);
    segs_of(it1, cx.seg[2], cx.seg[3]);
    cx.idle = cx.seg[1].p;
    ring_start(cx);
    int par = 0;
    f32x16 big[4], small[4];
    bf16x8 act[3][16];
#ifdef STNERF_BX_PROF
    BxProf bp;
    for (int i = 0; i < 16; ++i) bp.acc[i] = 0;
    bp.t = clock64();
#endif
    while (it0 < total) {
        // the item after next (consumed at the end of this one) and the ray index of the next item's sample
        uint32_t pending = 0;
        if (tid == 0) pending = atomicAdd(a.queue, 1u);
        RowRef rr_next;
        uint32_t next_ray = 0;   // (tap variant: all that is kept of the next item's row until its inputs are fetched)
        if constexpr (TAP) {
            const int64_t row = (int64_t)it1 * WV_ITEM + wave * WV_ROWS + (lane & 31);
            if (row < a.n_rays * a.ns) next_ray = (uint32_t)row / (uint32_t)a.ns;   // (rows <= 0x7fffff00: stnerf_train_spacenet_fwd)
        } else {
            row_of(it1, rr_next);
        }
        const StageLayer& ly = a.layer[slot_of(it0)];
        // ---- this item's bias vectors / head weights: blob consts -> LDS (12 + 4 chunks of 1 KB over the four waves).  The
        // previous item's last reads of the region are behind the barrier that ended it.
        {
            const char* sc = reinterpret_cast<const char*>(ly.space) + (sp_kind_stream[ly.use_time ? 1 : 0] - BX_CONST_SPACE * 4) + lane * 16;
            auto d = (__attribute__((address_space(3))) char*)(cs);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                __builtin_amdgcn_global_load_lds(sc + (wave + 4 * i) * BX_CHUNK, (__attribute__((address_space(3))) void*)(d + (wave + 4 * i) * BX_CHUNK), 16, 0, 0);
            if (ly.motion) {
                const char* mc = reinterpret_cast<const char*>(ly.motion) + (mo_stream - BX_CONST_MOTION * 4) + lane * 16;
                auto dm = (__attribute__((address_space(3))) char*)(cm);
                __builtin_amdgcn_global_load_lds(mc + wave * BX_CHUNK, (__attribute__((address_space(3))) void*)(dm + wave * BX_CHUNK), 16, 0, 0);
            }
        }
        float p[3];
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) p[c3] = cur.p[c3];
        BX_VMCNT(0);
        __builtin_amdgcn_s_barrier();
        BXP(BXP_TOP);
        // (the lane index the networks see is opaque per item: hoisted out of the item loop, the per-lane LDS addresses and
        // constants derived from it -- ~40 registers of the encodings alone -- do not fit beside the loop's live values and
        // come back from scratch, each reload behind a vmcnt(0) that also drains the weight ring's DMA queue)
        int ln = lane;
        asm volatile("" : "+v"(ln));
        if constexpr (!TAP) {
            if (ly.motion) motion_bx(cx, ly.motion, cm, encw, p, cur.tv, ly.motion_flags, ln, big, small, act BXP_ARG);
        }
        const auto tap = make_bx_tap(targs, it0, a.n_rays * a.ns, wave);
        if constexpr (TAP) cx.st_on = tap_wave_stores(tap, targs);
        float4 o = space_bx<DEEP>(cx, ly.space, ly.use_time != 0, cs, encw, p, ly.raybias, cur.ray, ln, big, small, act,
                                  [&]() {
                                      if constexpr (TAP) {
                                          const int64_t row = (int64_t)it1 * WV_ITEM + wave * WV_ROWS + (lane & 31);
                                          rr_next.valid = row < a.n_rays * a.ns;
                                          rr_next.ray = next_ray;
                                          rr_next.k = (int)((uint32_t)row - next_ray * (uint32_t)a.ns);
                                      }
                                      fetch(it1, rr_next, nxt);
                                  }, tap BXP_ARG);
        if constexpr (TAP) {   // (queue slot 0, every ray: row = 128 item + ..., sample k = row - ray * ns)
            const int64_t row = (int64_t)it0 * WV_ITEM + wave * WV_ROWS + (lane & 31);
            cur.raw_off = (int64_t)cur.ray * a.raw_ray_stride + 4 * (row - (int64_t)cur.ray * a.ns);
        }
        if (cur.valid && lane < 32) {
            if (a.sigmoid_rgb) {  // torch.sigmoid(rgb): 1-ulp v_exp_f32 / v_rcp_f32, the same expression the compositor uses
                o.x = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(o.x * -1.44269504088896340736f));
                o.y = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(o.y * -1.44269504088896340736f));
                o.z = __builtin_amdgcn_rcpf(1.f + __builtin_amdgcn_exp2f(o.z * -1.44269504088896340736f));
            }
            *reinterpret_cast<float4*>(ly.raw + cur.raw_off) = o;
        }
        if (tid == 0) qslot[par] = pending;
        __syncthreads();
        const uint32_t it2 = __builtin_amdgcn_readfirstlane(qslot[par]);
        par ^= 1;
        it0 = it1;
        it1 = it2;
        cur = nxt;
        // the stream: the next item's networks move up, the one after it joins
        cx.seg[0] = cx.seg[2];
        cx.seg[1] = cx.seg[3];
        segs_of(it1, cx.seg[2], cx.seg[3]);
        BXP(BXP_END);
#ifdef STNERF_BX_PROF
        bp.acc[BXP_ITEMS] += 1;
#endif
    }
    BX_VMCNT(0);  // (no LDS-DMA may outlive the workgroup)
#ifdef STNERF_BX_PROF
    if (lane == 0)
        for (int i = 0; i < 16; ++i) atomicAdd(&g_bxphase[i], bp.acc[i]);
#endif
}

int launch_bf16x3_stage(const StageArgs& a, bool deep_rgb, int cus, hipStream_t stream) {
    const int64_t max_items = ((a.n_rays * a.ns + WV_ITEM - 1) / WV_ITEM) * a.n_layers;
    const int grid = (int)(max_items < cus ? max_items : cus);  // one persistent workgroup per CU
    const void* kfn = deep_rgb ? reinterpret_cast<const void*>(mlp_bf16x3_stage_kernel<true, NoTapArgs>)
                               : reinterpret_cast<const void*>(mlp_bf16x3_stage_kernel<false, NoTapArgs>);
    if (const int rc = reserve_dynamic_lds(kfn, BX_LDS, "mlp_stage (bf16x3)")) return rc;
    if (deep_rgb)
        hipLaunchKernelGGL((mlp_bf16x3_stage_kernel<true, NoTapArgs>), dim3(grid), dim3(WV_THREADS), BX_LDS, stream, a, NoTapArgs());
    else
        hipLaunchKernelGGL((mlp_bf16x3_stage_kernel<false, NoTapArgs>), dim3(grid), dim3(WV_THREADS), BX_LDS, stream, a, NoTapArgs());
    STNERF_CHECK_LAUNCH("mlp_stage (bf16x3)");
    return STNERF_OK;
}

// One SpaceNet (queue slot 0 of `a`, every ray, no MotionNet, not deep_rgb) with every layer's input written out: see StoreTapArgs.
int launch_bf16x3_stage_store(const StageArgs& a, const StoreTapArgs& t, int cus, hipStream_t stream) {
    const int64_t max_items = (a.n_rays * a.ns + WV_ITEM - 1) / WV_ITEM;
    const int grid = (int)(max_items < cus ? max_items : cus);
    if (const int rc = reserve_dynamic_lds(reinterpret_cast<const void*>(mlp_bf16x3_stage_kernel<false, StoreTapArgs>), BX_LDS,
                                           "train_space_fwd (bf16x3)"))
        return rc;
    hipLaunchKernelGGL((mlp_bf16x3_stage_kernel<false, StoreTapArgs>), dim3(grid), dim3(WV_THREADS), BX_LDS, stream, a, t);
    STNERF_CHECK_LAUNCH("train_space_fwd (bf16x3)");
    return STNERF_OK;
}

// ---------------------------------------------------------------------------------------------
// MotionNet alone (MotionBxArgs): the stage kernel's item loop with one network.  motion_bx is the fused kernel's code, and a
// sample's flow depends on nothing but its point, frame id and flags (its column of every product): the moved points are the
// bits the stage kernel would have computed for the same rows.  The consts go to LDS once (one network per launch); the weight
// stream is the MotionNet's 19 slots per item, three slots ahead across items as in the stage kernel.
// ---------------------------------------------------------------------------------------------
constexpr int BX_LDS_MOTION = BX_LDS_RING + BX_LDS_ENC + BX_CONST_MOTION * 4 + 16;
static_assert(BX_LDS_MOTION <= 160 * 1024, "bf16x3 motion kernel: LDS budget");

struct MotionBxIn {
    float p[3], tv;
    float* dst;   // the sample's point (valid rows)
    bool valid;
};

__global__ __launch_bounds__(WV_THREADS, 1) void mlp_bf16x3_motion_kernel(MotionBxArgs a) {
    extern __shared__ __attribute__((aligned(16))) char smem_bxm[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    char* ring = smem_bxm;
    float* encw = reinterpret_cast<float*>(smem_bxm + BX_LDS_RING) + wave * WV_ENC_FLOATS;
    float* cm = reinterpret_cast<float*>(smem_bxm + BX_LDS_RING + BX_LDS_ENC);
    uint32_t* qslot = reinterpret_cast<uint32_t*>(cm + BX_CONST_MOTION);
    const int64_t rows = layer_rows(a.ray_count, a.n_rays, a.ns);
    const uint32_t total = (uint32_t)((rows + WV_ITEM - 1) / WV_ITEM);
    // row = 128 item + 32 wave + (lane & 31) = (hit ray rslot, j); both lane halves hold the same row
    auto fetch = [&](uint32_t item, MotionBxIn& in) {
        in.valid = false;
        in.dst = nullptr;
        in.tv = 0.f;
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) in.p[c3] = 0.f;
        const int64_t row = (int64_t)item * WV_ITEM + wave * WV_ROWS + (lane & 31);
        if (item >= total || row >= rows) return;
        const int64_t rslot = row / a.ns;
        const int j = (int)(row - rslot * a.ns);
        const int64_t ray = a.ray_list ? (int64_t)a.ray_list[rslot] : rslot;
        const int k = a.slots ? a.slots[ray * a.slot_ray_stride + j] : j;
        if (k < 0) return;
        float* src = a.xyz + ray * a.xyz_ray_stride + 3 * k;
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) in.p[c3] = src[c3];
        in.tv = a.times[ray * a.times_ray_stride];
        in.dst = src;
        in.valid = true;
    };
    const char* stream0 = reinterpret_cast<const char*>(a.net) + a.stream_off;
    auto seg_of = [&](uint32_t item) { return item < total ? Seg{stream0, (uint32_t)bx_motion_slots()} : Seg{nullptr, 0u}; };

    // ---- prime: the consts, two items popped, the first one's inputs, three slots of the stream in flight
    {
        const char* mc = stream0 - BX_CONST_MOTION * 4 + lane * 16;
        auto dm = (__attribute__((address_space(3))) char*)(cm);
        __builtin_amdgcn_global_load_lds(mc + wave * BX_CHUNK, (__attribute__((address_space(3))) void*)(dm + wave * BX_CHUNK), 16, 0, 0);
    }
    if (tid == 0) {
        qslot[0] = atomicAdd(a.queue, 1u);
        qslot[1] = atomicAdd(a.queue, 1u);
    }
    __syncthreads();
    uint32_t it0 = __builtin_amdgcn_readfirstlane(qslot[0]);
    uint32_t it1 = __builtin_amdgcn_readfirstlane(qslot[1]);
    __syncthreads();
    if (it0 >= total) {  // (uniform)
        BX_VMCNT(0);     // (no LDS-DMA may outlive the workgroup)
        return;
    }
    MotionBxIn cur, nxt;
    fetch(it0, cur);
    Ctx cx;
    ring_init(cx, ring, wave, lane);
    cx.st_on = false;
    cx.seg[0] = seg_of(it0);
    cx.seg[1] = Seg{nullptr, 0u};
    cx.seg[2] = seg_of(it1);
    cx.seg[3] = Seg{nullptr, 0u};
    cx.idle = stream0;
    ring_start(cx);
    int par = 0;
    f32x16 big[4], small[4];
    bf16x8 act[3][16];
#ifdef STNERF_BX_PROF
    BxProf bp;
    for (int i = 0; i < 16; ++i) bp.acc[i] = 0;
    bp.t = clock64();
#endif
    while (it0 < total) {
        uint32_t pending = 0;
        if (tid == 0) pending = atomicAdd(a.queue, 1u);
        // the next item's inputs: a chain of dependent loads (list -> slot -> point) that waits behind the ring's DMA queue,
        // once per item, here rather than between the slots
        fetch(it1, nxt);
        float p[3];
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) p[c3] = cur.p[c3];
        int ln = lane;   // (opaque per item, as in the stage kernel)
        asm volatile("" : "+v"(ln));
        motion_bx<1>(cx, a.net, cm, encw, p, cur.tv, a.flags, ln, big, small, act BXP_ARG);
        if (cur.valid && lane < 32) {
#pragma unroll
            for (int c3 = 0; c3 < 3; ++c3) cur.dst[c3] = p[c3];
        }
        if (tid == 0) qslot[par] = pending;
        __syncthreads();
        const uint32_t it2 = __builtin_amdgcn_readfirstlane(qslot[par]);
        par ^= 1;
        it0 = it1;
        it1 = it2;
        cur = nxt;
        cx.seg[0] = cx.seg[2];
        cx.seg[2] = seg_of(it1);
        BXP(BXP_END);
#ifdef STNERF_BX_PROF
        bp.acc[BXP_ITEMS] += 1;
#endif
    }
    BX_VMCNT(0);  // (no LDS-DMA may outlive the workgroup)
#ifdef STNERF_BX_PROF
    if (lane == 0)
        for (int i = 0; i < 16; ++i) atomicAdd(&g_bxphase[i], bp.acc[i]);
#endif
}

int launch_bf16x3_motion(const MotionBxArgs& args, int cus, hipStream_t stream) {
    MotionBxArgs a = args;
    a.stream_off = bx_layout(STNERF_NET_MOTION).stream_off;
    const int64_t max_items = (a.n_rays * a.ns + WV_ITEM - 1) / WV_ITEM;
    if (max_items == 0) return STNERF_OK;
    const int grid = (int)(max_items < cus ? max_items : cus);  // one persistent workgroup per CU
    if (const int rc = reserve_dynamic_lds(reinterpret_cast<const void*>(mlp_bf16x3_motion_kernel), BX_LDS_MOTION, "motionnet (bf16x3)"))
        return rc;
    hipLaunchKernelGGL(mlp_bf16x3_motion_kernel, dim3(grid), dim3(WV_THREADS), BX_LDS_MOTION, stream, a);
    STNERF_CHECK_LAUNCH("motionnet (bf16x3)");
    return STNERF_OK;
}

}  // namespace stnerf

#ifdef STNERF_BX_PROF
extern "C" int stnerf_debug_bx_phases(unsigned long long* host16, int reset) {
    if (hipMemcpyFromSymbol(host16, HIP_SYMBOL(stnerf::g_bxphase), sizeof(unsigned long long) * 16) != hipSuccess) return STNERF_ELAUNCH;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(stnerf::g_bxphase), z, sizeof(z)) != hipSuccess) return STNERF_ELAUNCH;
    }
    return STNERF_OK;
}
#endif
