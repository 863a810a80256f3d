// Wave64 building blocks of the compositor (composite.hip), its backward (render_bwd.hip) and the resampler (resample.hip):
// cross-lane moves and in-place prefix scans on DPP, the wave-private LDS phase fence, the hardware exponential / sigmoid,
// the bounded LDS searches, and the optional per-phase cycle counters.
#pragma once
#include "common.h"

namespace stnerf {

// Optional per-phase cycle accounting (development builds: -DSTNERF_COMP_PROF): every wave adds its s_memtime deltas per
// phase.  The counters are per translation unit (a static __device__ array is not shared without relocatable device code):
// read back with stnerf_debug_composite_phases() (composite.hip) / stnerf_debug_resample_phases() (resample.hip).
#ifdef STNERF_COMP_PROF
static __device__ unsigned long long g_cphase[8];
#define CP_DECL unsigned long long cp_t = clock64(), cp_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#define CP(i) do { const unsigned long long n_ = clock64(); cp_acc[i] += n_ - cp_t; cp_t = n_; } while (0)
#define CP_FLUSH do { if ((threadIdx.x & 63) == 0) for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_cphase[i_], cp_acc[i_]); } while (0)
#else
#define CP_DECL
#define CP(i) do { } while (0)
#define CP_FLUSH do { } while (0)
#endif

// ---- wave64 cross-lane primitives on DPP (gfx9 row_shr / row_bcast / wave_shr controls: one VALU op per
// scan step, no LDS crossbar traffic; ds_bpermute-based __shfl_up costs ~5 instructions per step).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ float dpp_move(float identity, float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(identity), __float_as_int(v), CTRL, ROW_MASK, 0xf, false));
}
constexpr int DPP_ROW_SHR1 = 0x111, DPP_ROW_SHR2 = 0x112, DPP_ROW_SHR4 = 0x114, DPP_ROW_SHR8 = 0x118;
constexpr int DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143, DPP_WAVE_SHR1 = 0x138, DPP_WAVE_SHL1 = 0x130;

// The fp32 scans run IN PLACE: `v_mul_f32_dpp v, v, v row_shr:1` multiplies every lane whose source lane exists by that lane's
// value and leaves the others untouched (bound_ctrl off: a lane without a source is not executed) -- one vector
// instruction per step.  Written through the update_dpp builtin the same step is three (identity into a scratch
// register, DPP move over it, multiply), and the compositor is bound by its vector-instruction count.
// The two wait states a DPP read needs behind the write of its source are the s_nop 1 in front of every step.  The FIRST
// step of a block waits five: LLVM's hazard recognizer does not look inside inline asm, so a VALU write of EXEC (v_cmpx of
// the predicated code these scans are called behind) directly in front of the block would otherwise leave the
// "VALU writes EXEC -> DPP" hazard (5 wait states) uncovered.  tests/test_kernel_resources.py scans the ISA of every
// other DPP instruction of composite.hip and resample.hip for the same hazard.
#define STNERF_DPP_STEP(op, ctrl) "s_nop 1\n\t" op " %0, %0, %0 " ctrl "\n\t"
#define STNERF_DPP_FIRST(op, ctrl) "s_nop 4\n\t" op " %0, %0, %0 " ctrl "\n\t"
__device__ __forceinline__ float wave_scan_mul(float v) {  // inclusive
    asm(STNERF_DPP_FIRST("v_mul_f32_dpp", "row_shr:1 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_mul_f32_dpp", "row_shr:2 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_mul_f32_dpp", "row_shr:4 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_mul_f32_dpp", "row_shr:8 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_mul_f32_dpp", "row_bcast:15 row_mask:0xa bank_mask:0xf")
        STNERF_DPP_STEP("v_mul_f32_dpp", "row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(v));
    return v;
}

__device__ __forceinline__ float wave_scan_add(float v) {  // inclusive
    asm(STNERF_DPP_FIRST("v_add_f32_dpp", "row_shr:1 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_add_f32_dpp", "row_shr:2 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_add_f32_dpp", "row_shr:4 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_add_f32_dpp", "row_shr:8 row_mask:0xf bank_mask:0xf")
        STNERF_DPP_STEP("v_add_f32_dpp", "row_bcast:15 row_mask:0xa bank_mask:0xf")
        STNERF_DPP_STEP("v_add_f32_dpp", "row_bcast:31 row_mask:0xc bank_mask:0xf")
        : "+v"(v));
    return v;
}

// Inclusive add-scan in fp64 (cdf accumulation of the resampler, see resample_kernel in resample.hip): the same DPP ladder as the fp32
// scans, moving the two halves of the double separately (2 DPP moves + one v_add_f64 per step; a __shfl_up of a double
// is two ds_bpermute round trips per step).
template <int CTRL, int ROW_MASK = 0xf>
__device__ __forceinline__ double dpp_move_f64(double v) {  // lanes the control leaves out receive +0.0
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(b & 0xffffffffll), CTRL, ROW_MASK, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, ROW_MASK, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned int)lo);
}
__device__ __forceinline__ double wave_scan_add_f64(double v) {
    v += dpp_move_f64<DPP_ROW_SHR1>(v);
    v += dpp_move_f64<DPP_ROW_SHR2>(v);
    v += dpp_move_f64<DPP_ROW_SHR4>(v);
    v += dpp_move_f64<DPP_ROW_SHR8>(v);
    v += dpp_move_f64<DPP_ROW_BCAST15, 0xa>(v);
    v += dpp_move_f64<DPP_ROW_BCAST31, 0xc>(v);
    return v;
}

// value of the previous lane (lane 0 gets `first`)
__device__ __forceinline__ float wave_prev(float v, float first) { return dpp_move<DPP_WAVE_SHR1>(first, v); }
__device__ __forceinline__ float wave_last(float v) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63)); }

// Branch-free binary lifting over an ascending LDS array: #{x in a[0..n) : x < v} / #{x <= v}.
// `p2` = largest power of two <= n (wave-uniform).
__device__ __forceinline__ int lower_bound_lds(const float* a, int n, int p2, float v) {
    int pos = 0;
    for (int step = p2; step > 0; step >>= 1) {
        const int np = pos + step;
        const float x = a[(np < n ? np : n) - 1];
        pos = (np <= n && x < v) ? np : pos;
    }
    return pos;
}
__device__ __forceinline__ int upper_bound_lds(const float* a, int n, int p2, float v) {
    int pos = 0;
    for (int step = p2; step > 0; step >>= 1) {
        const int np = pos + step;
        const float x = a[(np < n ? np : n) - 1];
        pos = (np <= n && x <= v) ? np : pos;
    }
    return pos;
}
// The same two counts over a strictly DESCENDING array, read back to front (a[n-1-i] is ascending).
__device__ __forceinline__ int lower_bound_lds_rev(const float* a, int n, int p2, float v) {
    int pos = 0;
    for (int step = p2; step > 0; step >>= 1) {
        const int np = pos + step;
        const float x = a[n - (np < n ? np : n)];
        pos = (np <= n && x < v) ? np : pos;
    }
    return pos;
}
__device__ __forceinline__ int upper_bound_lds_rev(const float* a, int n, int p2, float v) {
    int pos = 0;
    for (int step = p2; step > 0; step >>= 1) {
        const int np = pos + step;
        const float x = a[n - (np < n ? np : n)];
        pos = (np <= n && x <= v) ? np : pos;
    }
    return pos;
}
__host__ __device__ __forceinline__ int floor_pow2(int n) {
    int p = 1;
    while (p * 2 <= n) p *= 2;
    return p;
}

// Every LDS region below is private to one wave, so phases only need ordering inside the wave: LDS operations of
// a wave execute in issue order, the fences stop the compiler from moving accesses across the phase boundary.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// exp(-x) on the hardware exponential: v_exp_f32 is 2^y to 1 ulp; the scaling by log2(e) adds |x| * 2^-24 of relative
// error, which only matters where exp(-x) has already left the fp32 range of 1 - exp(-x).  ocml's expf costs ~3x the
// issue slots and this kernel is bound by them.
__device__ __forceinline__ float exp_neg(float x) { return __builtin_amdgcn_exp2f(x * -1.44269504088896340736f); }
// torch.sigmoid: 1/(1+exp(-x)), 1-ulp exponential and 1-ulp reciprocal
__device__ __forceinline__ float sigmoidf(float x) { return __builtin_amdgcn_rcpf(1.f + exp_neg(x)); }

}  // namespace stnerf
