// The split-bf16 ("bf16x3") kernels of the render path, on the machinery of mlp_bf16x3_core.h (the design is described there): the
// persistent stage kernel (mlp_bf16x3_stage_kernel<DEEP, NoTapArgs>; with the training tap: <false, StoreTapArgs>) and the stage
// kernel's MotionNet alone (mlp_bf16x3_motion_kernel).  The backward chain: train_bf16x3.hip; the packers: pack_bf16x3.hip.
//
// Reference: modeling/spacenet.py:16-160, modeling/motion_net.py:7-71, modeling/layered_rfrender.py:340-418,495-576.
#define STNERF_STAGE_KERNEL mlp_bf16x3_stage_kernel
#include "mlp_bf16x3_stage_kernel.h"

namespace stnerf {

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
