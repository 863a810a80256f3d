// The definition of the exact-f32 stage kernel (the organisation is described in mlp_wave.hip), under the name the including file
// gives it in STNERF_STAGE_KERNEL: mlp_wave_stage_kernel (mlp_wave.hip: rows = hit rays x samples; TapArgs = NoTapArgs, or
// StoreTapArgs for training) and mlp_wave_stage_rows_kernel (mlp_wave_rows.hip: TapArgs = StageRowsArgs, a layer's rows may come
// from a row list).  One text, so that the flavours differ in nothing but how an item's rows are located -- and a definition, not
// an inlined function: the kernels a render without row lists launches are instruction for instruction what they were.
#pragma once
#include "mlp_wave_core.h"

namespace stnerf {

// Training: the same kernel with a tap that writes every layer's input -- the activations the backward pass
// needs -- to row-major matrices the caller owns, as the item's rows pass through the registers: one launch instead of a
// chain of per-layer GEMMs through HBM for the recomputation, and the SAME arithmetic as the forward that produced the loss.
// Slot 0 of the queue only (the training entry point launches one network).  Row r of the launch <-> row r of every matrix.
struct StoreTap {
    const StoreTapArgs* a;
    uint32_t row;
    bool valid;
    template <int NBLK>
    __device__ __forceinline__ void blocks(int stage, const f32x16 (&blk)[NBLK], int nblk, int lane) const {
        if (!valid) return;
        float* base = stage == TAP_PE ? a->pe : a->buf[stage];
        const int ld = stage == TAP_PE ? a->ld_pe : a->ld[stage];
        // register 4 q + r of block fb <-> feature 32 fb + 8 q + 4 h + r: 16 bytes per (fb, q), the two lanes of a sample side by side
        float4* p = reinterpret_cast<float4*>(base + (size_t)row * (size_t)ld + 4 * (lane >> 5));
#pragma unroll
        for (int fb = 0; fb < NBLK; ++fb)
            if (fb < nblk) {
#pragma unroll
                for (int q = 0; q < 4; ++q)
                    p[fb * 8 + 2 * q] = make_float4(blk[fb][4 * q + 0], blk[fb][4 * q + 1], blk[fb][4 * q + 2], blk[fb][4 * q + 3]);
            }
        // The ReLU mask of this lane's values as bits: value 16 fb + i <-> bit (16 fb + i) & 31 of word fb >> 1 -- 16 bytes per lane,
        // 32 per row, which the backward chain (csrc/train_wave.hip: the SAME lane owns the same values there) reads back instead of
        // the 1 KB of activations.  Two instructions per value: min(bits, 1) -- a post-ReLU value is +0 or positive -- and a shift-or.
        if (a->bits && stage != TAP_PE) {
            uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
            for (int wd = 0; wd < NBLK / 2; ++wd)
                if (2 * wd < nblk) {
#pragma unroll
                    for (int j = 31; j >= 0; --j) {
                        // (asm: the compiler's own choice is compare + select + shift-or, three instructions, with the 128 selects hoisted
                        // into registers the kernel does not have)
                        uint32_t t;
                        asm volatile("v_min_u32 %1, 1, %2\n\tv_lshl_or_b32 %0, %0, 1, %1" : "+v"(w[wd]), "=&v"(t) : "v"(blk[2 * wd + (j >> 4)][j & 15]));
                    }
                }
            uint4* bp = reinterpret_cast<uint4*>(a->bits + (size_t)stage * (size_t)a->bits_stride + (size_t)row * 8u + 4u * (uint32_t)(lane >> 5));
            *bp = make_uint4(w[0], w[1], w[2], w[3]);
        }
    }
};
__device__ __forceinline__ NoTap make_tap(const NoTapArgs&, uint32_t, bool) { return NoTap(); }
__device__ __forceinline__ StoreTap make_tap(const StoreTapArgs& t, uint32_t row, bool valid) { return StoreTap{&t, row, valid}; }
__device__ __forceinline__ NoTap make_tap(const StageRowsArgs&, uint32_t, bool) { return NoTap(); }

template <bool DEEP, class TapArgs>
__global__ __launch_bounds__(WV_THREADS, 1) void STNERF_STAGE_KERNEL(StageArgs a, TapArgs targs) {
    constexpr bool ROWS = std::is_same<TapArgs, StageRowsArgs>::value;
    extern __shared__ __attribute__((aligned(16))) float4 smem[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* encw = reinterpret_cast<float*>(smem) + wave * WV_WAVE_FLOATS;  // [encodings | bias vectors]
    uint32_t* qslot = reinterpret_cast<uint32_t*>(reinterpret_cast<float*>(smem) + WV_NW * WV_WAVE_FLOATS);
    // ---- the queue: items (128 rows) of layer slot j are [pre[j], pre[j+1]); the row counts (one global load each) are
    // kept in LDS for the per-item lookups
    int64_t* lrows = reinterpret_cast<int64_t*>(qslot + 4);
    uint32_t pre[STNERF_MAX_LAYERS + 1];
    pre[0] = 0;
#pragma unroll
    for (int j = 0; j < STNERF_MAX_LAYERS; ++j) {
        uint32_t items = 0;
        if (j < a.n_layers) {
            const int64_t rows = slot_rows(a.layer[j], targs, j, a.n_rays, a.ns);
            items = (uint32_t)((rows + WV_ITEM - 1) / WV_ITEM);
            if (tid == 0) lrows[j] = rows;
        }
        pre[j + 1] = pre[j] + items;
    }
    const uint32_t total = pre[STNERF_MAX_LAYERS];
    auto slot_of = [&](uint32_t item) {
        int slot = 0;
#pragma unroll
        for (int j = 1; j < STNERF_MAX_LAYERS; ++j) slot += (item >= pre[j]) ? 1 : 0;
        return slot;
    };
    auto base_of = [&](uint32_t item) {
        uint32_t b = 0;
#pragma unroll
        for (int j = 1; j < STNERF_MAX_LAYERS; ++j) b = (item >= pre[j]) ? pre[j] : b;
        return b;
    };
    // row of this lane's sample in an item, and the ray it belongs to (first half of an item's fetch)
    auto row_of = [&](uint32_t item, RowRef& rr) {
        rr = RowRef{0, 0, false};
        if (item >= total) return;
        const int slot = slot_of(item);
        const int64_t rows = lrows[slot];
        const int64_t row = (int64_t)(item - base_of(item)) * WV_ITEM + wave * WV_ROWS + (lane & 31);
        rr.valid = row < rows;
        if constexpr (ROWS) {   // a listed slot: the packed word replaces the division and the ray list
            const int32_t* rw = targs.row_list[slot];
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
            if (rows <= 0x7fffffffll) {  // (uniform) the usual case: a 32-bit division
                const uint32_t q = (uint32_t)row / (uint32_t)a.ns;
                rslot = q;
                rr.k = (int)((uint32_t)row - q * (uint32_t)a.ns);
            } else {
                rslot = row / a.ns;
                rr.k = (int)(row - rslot * a.ns);
            }
            const int32_t* rl = a.layer[slot].ray_list;
            rr.ray = rl ? (int64_t)rl[rslot] : rslot;
        }
    };
    // second half: the sample's inputs (HBM loads)
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

    // ---- prime the pipeline: two items popped, the first one's inputs loaded.  Without a queue (the op-level entry
    // stnerf_spacenet_fwd has no counter to give) workgroup b takes the items b, b + grid, ... in turn.
    if (tid == 0) {
        qslot[0] = a.queue ? atomicAdd(a.queue, 1u) : blockIdx.x;
        qslot[1] = a.queue ? atomicAdd(a.queue, 1u) : blockIdx.x + gridDim.x;
    }
    __syncthreads();
    uint32_t it0 = __builtin_amdgcn_readfirstlane(qslot[0]);
    uint32_t it1 = __builtin_amdgcn_readfirstlane(qslot[1]);
    __syncthreads();
    WaveInputs cur, nxt;
    {
        RowRef rr;
        row_of(it0, rr);
        fetch(it0, rr, cur);
    }
    int par = 0;
    f32x16 acc[8], in[8];
    float4 wa[8], wb[8];
#ifdef STNERF_WAVE_PROF
    WaveProf wp;
    for (int i = 0; i < 16; ++i) wp.acc[i] = 0;
    wp.t = clock64();
#endif
    while (it0 < total) {
        // the item after next (consumed at the end of this one) and the ray index of the next item's sample
        uint32_t pending = 0;
        if (tid == 0) pending = a.queue ? atomicAdd(a.queue, 1u) : it1 + gridDim.x;
        RowRef rr_next;
        row_of(it1, rr_next);
        const StageLayer& ly = a.layer[slot_of(it0)];
        float p[3];
#pragma unroll
        for (int c3 = 0; c3 < 3; ++c3) p[c3] = cur.p[c3];
#ifdef STNERF_WAVE_DEBUG
        WaveDbg dbg{a.dbg, a.dbg_stage, -1};
        if (slot_of(it0) == 0 && cur.valid) dbg.row = (int64_t)(it0 - base_of(it0)) * WV_ITEM + wave * WV_ROWS + (lane & 31);
#endif
        WP(WP_TOP);
        // (deep_rgb variant: the lane index the networks see is opaque per item -- hoisted out of the item loop, the
        // per-lane LDS addresses derived from it do not fit beside this variant's live values and go to scratch)
        int ln = lane;
        if constexpr (DEEP) asm volatile("" : "+v"(ln));
        if (ly.motion) motion_wave(ly.motion, encw, p, cur.tv, ly.motion_flags, ln, acc, in, wa, wb WV_DBG_ARG WP_ARG);
        // (training: the row of this lane's sample in the launch; items of slot 0 are rows 128 item ..)
        const auto tap = make_tap(targs, it0 * (uint32_t)WV_ITEM + (uint32_t)(wave * WV_ROWS + (lane & 31)), cur.valid);
        float4 o = space_wave<DEEP>(ly.space, ly.use_time != 0, encw, p, ly.raybias, cur.ray, ln, acc, in, wa, wb,
                                    [&]() { fetch(it1, rr_next, nxt); } WV_DBG_ARG WP_ARG, tap);
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
        WP(WP_END);
#ifdef STNERF_WAVE_PROF
        wp.acc[WP_ITEMS] += 1;
#endif
    }
#ifdef STNERF_WAVE_PROF
    if (lane == 0)
        for (int i = 0; i < 16; ++i) atomicAdd(&g_wphase[i], wp.acc[i]);
#endif
}

}  // namespace stnerf
