// The definition of the split-bf16 stage kernel (on the machinery of mlp_bf16x3_core.h), under the name the including file gives it
// in STNERF_STAGE_KERNEL: mlp_bf16x3_stage_kernel (mlp_bf16x3.hip: rows = hit rays x samples; TapArgs = NoTapArgs, or StoreTapArgs
// for training) and mlp_bf16x3_stage_rows_kernel (mlp_bf16x3_rows.hip: TapArgs = StageRowsArgs, a layer's rows may come from a row
// list).  One text, so that the flavours differ in nothing but how an item's rows are located -- and a definition, not an inlined
// function: the kernels a render without row lists launches are instruction for instruction what they were.
#pragma once
#include "mlp_bf16x3_core.h"

namespace stnerf {

#ifdef STNERF_BX_PROF
// Per-phase clocks of the including file's kernels (BXP: mlp_bf16x3_core.h).  Development builds only, and `static`: each file that
// includes this header has a copy of its own.  stnerf_debug_bx_phases() (mlp_bf16x3.hip) reads mlp_bf16x3.hip's copy, so it sees the
// kernels of that file; what the row-list flavour (mlp_bf16x3_rows.hip) adds to its copy is read by nobody.  Profile a render without
// row lists: the two flavours differ in the locate step alone.
static __device__ unsigned long long g_bxphase[16];
#endif

// does this wave issue every store of a boundary?  (some row of its 32 inside the launch, mask planes wanted)
__device__ __forceinline__ bool tap_wave_stores(const BxStoreTap& tap, const StoreTapArgs& t) {
    return (uint32_t)(tap.wave * WV_ROWS) < tap.nrows && t.bits != nullptr;
}
__device__ __forceinline__ BxNoTap make_bx_tap(const NoTapArgs&, uint32_t, int64_t, int) { return BxNoTap(); }
__device__ __forceinline__ BxNoTap make_bx_tap(const StageRowsArgs&, uint32_t, int64_t, int) { return BxNoTap(); }
__device__ __forceinline__ BxStoreTap make_bx_tap(const StoreTapArgs& t, uint32_t item, int64_t rows, int wave) {
    // (training launches one network: items of queue slot 0 are rows 128 item ..)
    const int64_t left = rows - (int64_t)item * WV_ITEM;
    return BxStoreTap{&t, item * (uint32_t)WV_ITEM, (uint32_t)(left < WV_ITEM ? left : WV_ITEM), wave};
}

// The tap variant (training: ONE SpaceNet on every ray, no MotionNet, no ray list) gives the tap's stores the registers they need
// by not carrying per-row values through the item: the next item's (ray, sample) is located where it is fetched, not at the
// top of the item; this item's output offset is recomputed from its ray at the end; the MotionNet path is compiled out.
template <bool DEEP, class TapArgs>
__global__ __launch_bounds__(WV_THREADS, 1) void STNERF_STAGE_KERNEL(StageArgs a, TapArgs targs) {
    constexpr bool TAP = std::is_same<TapArgs, StoreTapArgs>::value;
    constexpr bool ROWS = std::is_same<TapArgs, StageRowsArgs>::value;
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
        const int64_t rows = slot_rows(a.layer[j], targs, j, a.n_rays, a.ns);
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
        if constexpr (ROWS) {   // a listed slot: the packed word replaces the division and the ray list
            const int32_t* rw = targs.row_list[s];
            if (rw) {
                if (rr.valid) {
                    const uint32_t v = (uint32_t)rw[row];
                    rr.ray = v >> 8;
                    rr.k = (int)(v & 255u);
                }
                return;
            }
        }
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

}  // namespace stnerf
