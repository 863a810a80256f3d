// Persistent stage kernel, second organisation: SAMPLE-split waves with the activations in registers.
//
// The round-2 stage kernel (mlp_stage.hip, removed in round 3) split a layer's OUTPUT FEATURES over the 8 waves of a
// workgroup, so every layer was an all-to-all
// through LDS: 128 KiB of activations are written (ds_write_b128: ~79 B/clk/CU, ~1.1k cycles per layer with the matrix
// pipe idle) and two workgroup barriers are taken per layer; that, the heads' LDS reductions and the issue slots of
// the activation reads are the ~9 % the kernel stands below the f32 MFMA peak.  Here a wave owns 32 SAMPLES and all
// features of a layer:
//   * v_mfma_f32_32x32x2_f32 computed transposed (A = weights, B = activations) leaves a lane (h, c) with the
//     output features 32 fb + 8 q + 4 h + r of sample c in accumulator register 4 q + r of block fb -- and with the
//     k permutation the packed weights already use (lane half h takes k = 8 s + 4 h + {0..3}) that is exactly the B
//     operand the NEXT layer needs from this lane: K step s, instruction kk reads register 4 (s & 3) + kk of block
//     s >> 2.  The activations of the whole network therefore never leave the register file: no LDS traffic, no
//     barrier, no epilogue stores between layers; a layer boundary is 128 ReLUs (v_max_i32) and nothing else.
//   * 256 features x 32 samples = 128 registers in + 128 accumulators out: one wave per SIMD with the unified
//     512-entry register file (accumulators in AGPRs), 4 waves = 128 samples per CU.  (A second wave per SIMD would
//     not buy overlap: f32 MFMAs run on the SIMD's own f32 lanes, a vector instruction costs the MFMA stream its 5 - 6
//     cycles whichever wave issues it -- tools/micro/mfma_two_waves.hip.  What counts is the vector instruction COUNT.)
//   * Weights: the A operand of a K step is 8 x 16 B per lane straight from the packed blob (buffer loads, SGPR
//     offsets, one step ahead); the four waves of a CU run the same network in step, so each line comes out of L2
//     once per CU and the other three waves hit the vector L1.
//   * rgb_net.1's direction / time columns come per RAY from mlp_raybias.hip, added behind the layer's product.
//   * Encodings are staged through a wave-private 11 KiB LDS window (the two lanes of a sample split the frequencies,
//     then each lane reads its half of the feature quads back) -- ordering inside a wave only, no barrier.
//   * Heads: a lane holds every second feature quad of its sample; the partial sums are grouped as 4 parts x 4
//     interleaved chains (mlp_wave_core.h: head_sigma), the two lanes of a sample swap their chains with v_permlane32_swap.
// The op-level entries run this arithmetic too: stnerf_spacenet_fwd is this kernel on one layer without a queue
// (stage_entry.hip), stnerf_motionnet_fwd runs motion_wave in train_motion_fwd_kernel (mlp_wave_core.h, also stage_entry.hip).
//
// Reference: modeling/spacenet.py:16-160, modeling/motion_net.py:7-71, modeling/layered_rfrender.py:340-418,495-576.
#define STNERF_STAGE_KERNEL mlp_wave_stage_kernel
#include "mlp_wave_stage_kernel.h"

namespace stnerf {

#ifdef STNERF_WAVE_DEBUG
static float* g_dbg_buf = nullptr;
static int g_dbg_stage = -1;
#endif

int launch_wave_stage(const StageArgs& a_in, bool deep_rgb, int cus, hipStream_t stream) {
    StageArgs a = a_in;
#ifdef STNERF_WAVE_DEBUG
    a.dbg = g_dbg_buf;
    a.dbg_stage = g_dbg_stage;
#endif
    const int64_t max_items = ((a.n_rays * a.ns + WV_ITEM - 1) / WV_ITEM) * a.n_layers;
    const int grid = (int)(max_items < cus ? max_items : cus);  // one persistent workgroup per CU
    const void* kfn = deep_rgb ? reinterpret_cast<const void*>(mlp_wave_stage_kernel<true, NoTapArgs>)
                               : reinterpret_cast<const void*>(mlp_wave_stage_kernel<false, NoTapArgs>);
    if (const int rc = reserve_dynamic_lds(kfn, WV_LDS, "mlp_stage (wave)")) return rc;
    if (deep_rgb)
        hipLaunchKernelGGL((mlp_wave_stage_kernel<true, NoTapArgs>), dim3(grid), dim3(WV_THREADS), WV_LDS, stream, a, NoTapArgs());
    else
        hipLaunchKernelGGL((mlp_wave_stage_kernel<false, NoTapArgs>), dim3(grid), dim3(WV_THREADS), WV_LDS, stream, a, NoTapArgs());
    STNERF_CHECK_LAUNCH("mlp_stage (wave)");
    return STNERF_OK;
}

// One SpaceNet (queue slot 0 of `a`, no MotionNet, not deep_rgb) with every layer's input written out: see StoreTapArgs.
int launch_wave_stage_store(const StageArgs& a, float* const (&buf)[8], const int32_t (&ld)[8], float* pe, int32_t ld_pe, uint32_t* bits,
                            int64_t bits_stride, int cus, hipStream_t stream) {
    StoreTapArgs t;
    t.bits = bits;
    t.bits_stride = bits_stride;
    for (int i = 0; i < 8; ++i) {
        t.buf[i] = buf[i];
        t.ld[i] = ld[i];
    }
    t.pe = pe;
    t.ld_pe = ld_pe;
    const int64_t max_items = (a.n_rays * a.ns + WV_ITEM - 1) / WV_ITEM;
    const int grid = (int)(max_items < cus ? max_items : cus);
    if (const int rc = reserve_dynamic_lds(reinterpret_cast<const void*>(mlp_wave_stage_kernel<false, StoreTapArgs>), WV_LDS, "train_space_fwd"))
        return rc;
    hipLaunchKernelGGL((mlp_wave_stage_kernel<false, StoreTapArgs>), dim3(grid), dim3(WV_THREADS), WV_LDS, stream, a, t);
    STNERF_CHECK_LAUNCH("train_space_fwd");
    return STNERF_OK;
}

}  // namespace stnerf

#ifdef STNERF_WAVE_PROF
extern "C" int stnerf_debug_wave_phases(unsigned long long* host16, int reset) {
    if (hipMemcpyFromSymbol(host16, HIP_SYMBOL(stnerf::g_wphase), sizeof(unsigned long long) * 16) != hipSuccess) return STNERF_ELAUNCH;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(stnerf::g_wphase), z, sizeof(z)) != hipSuccess) return STNERF_ELAUNCH;
    }
    return STNERF_OK;
}
#endif

#ifdef STNERF_WAVE_DEBUG
// development builds only: where the next stnerf_mlp_stage launches dump the activations of queue slot 0
extern "C" int stnerf_debug_wave_dump(float* buf, int stage) {
    stnerf::g_dbg_buf = buf;
    stnerf::g_dbg_stage = stage;
    return STNERF_OK;
}
#endif
