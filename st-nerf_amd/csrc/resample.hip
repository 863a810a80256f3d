// Inverse-CDF resampler.  One WAVE (64 lanes) owns one (ray, layer) pair; the cdf is a wavefront prefix scan, the new
// samples are sorted in registers and merged into the coarse list by ranks.
//
// HBM-bound by its bytes: reads 8 B per coarse sample and writes 16 B per fine sample (t + xyz).
//
// Reference: utils/sample_pdf.py:18-63, modeling/layered_rfrender.py:455-465.
#include "common.h"
#include "wave_prims.h"

// Occupancy target (waves per SIMD) of the kernel: the VGPR budget follows from it (512 / waves).
#ifndef STNERF_WAVES_RESAMPLE
#define STNERF_WAVES_RESAMPLE 8
#endif

namespace stnerf {

// torch.sum(x, -1) of one contiguous fp32 row, bit for bit as ATen computes it on a CPU: the reference's
// `torch.sum(weights, -1, keepdim=True)` (utils/sample_pdf.py:22) is an fp32 reduction whose rounding depends on the
// order, so "the reference's value" is defined by ATen's kernel (aten/src/ATen/native/cpu/SumKernel.cpp, dispatched
// with 8-float vectors on every x86 capability level -- DEFAULT, AVX2 and AVX512 alike, checked against torch 2.10 in
// tests/test_oracle_golden.py::test_aten_sum_order): rows of >= 8 elements go through vectorized_inner_sum = 8 vector
// lanes x 4 interleaved accumulators over the full vectors (row_sum / multi_row_sum, with its 16-row cascade level),
// the accumulators folded ((a0+a1)+a2)+a3, then a scalar chain over the < 8 leftover elements followed by the 8
// lanes in order; shorter rows take the scalar row_sum.  x lives in (wave-private) LDS; every lane returns the sum.
__device__ __forceinline__ float aten_cpu_row_sum(const float* x, int n, int lane) {
    if (n < 8) {
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, p3 = 0.f;
        const int rows = n >> 2;
        for (int i = 0; i < rows; ++i) {
            p0 += x[4 * i + 0];
            p1 += x[4 * i + 1];
            p2 += x[4 * i + 2];
            p3 += x[4 * i + 3];
        }
        for (int j = rows * 4; j < n; ++j) p0 += x[j];
        return ((p0 + p1) + p2) + p3;
    }
    const int nv = n >> 3, rows = nv >> 2, j = lane & 7;  // lanes 8.. repeat column lane & 7 (uniform control flow)
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, b0 = 0.f, b1 = 0.f, b2 = 0.f, b3 = 0.f;
    int i = 0;
#pragma unroll 1
    for (; i + 16 <= rows;) {  // cascade level 1: every 16 rows the running accumulators are folded away
#pragma unroll 1
        for (int r = 0; r < 16; ++r, ++i) {
            a0 += x[(4 * i + 0) * 8 + j];
            a1 += x[(4 * i + 1) * 8 + j];
            a2 += x[(4 * i + 2) * 8 + j];
            a3 += x[(4 * i + 3) * 8 + j];
        }
        b0 += a0; b1 += a1; b2 += a2; b3 += a3;
        a0 = a1 = a2 = a3 = 0.f;
    }
#pragma unroll 1
    for (; i < rows; ++i) {
        a0 += x[(4 * i + 0) * 8 + j];
        a1 += x[(4 * i + 1) * 8 + j];
        a2 += x[(4 * i + 2) * 8 + j];
        a3 += x[(4 * i + 3) * 8 + j];
    }
    a0 += b0; a1 += b1; a2 += b2; a3 += b3;  // (levels 2 and 3 stay zero below 256 rows = 8192 elements)
#pragma unroll 1
    for (int v = rows * 4; v < nv; ++v) a0 += x[v * 8 + j];
    const float col = ((a0 + a1) + a2) + a3;
    float fin = 0.f;
#pragma unroll 1
    for (int k = nv * 8; k < n; ++k) fin += x[k];
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) fin += __int_as_float(__builtin_amdgcn_readlane(__float_as_int(col), jj));
    return fin;
}

// ---- searches over an ascending LDS array padded with +inf up to (a power of two) - 1 entries: no bounds logic, the running
// position is a byte address -- add, ds_read, compare, select per step (the bounded form of wave_prims.h: eight instructions).
// `half_bytes` = 4 * P / 2 for P = the smallest power of two > n (wave-uniform).  Returns #{x <= v} / #{x < v}.
__host__ __device__ __forceinline__ int pow2_above(int n) {
    int p = 1;
    while (p <= n) p *= 2;
    return p;
}
__device__ __forceinline__ int upper_bound_padded(const float* a, int half_bytes, float v) {
    const char* base = reinterpret_cast<const char*>(a) - 4;
    const char* q = base;
    for (int step = half_bytes; step >= 4; step >>= 1) {
        const char* c = q + step;
        const float x = *reinterpret_cast<const float*>(c);
        q = (x <= v) ? c : q;
    }
    return (int)(q - base) >> 2;
}
__device__ __forceinline__ int lower_bound_padded(const float* a, int half_bytes, float v) {
    const char* base = reinterpret_cast<const char*>(a) - 4;
    const char* q = base;
    for (int step = half_bytes; step >= 4; step >>= 1) {
        const char* c = q + step;
        const float x = *reinterpret_cast<const float*>(c);
        q = (x < v) ? c : q;
    }
    return (int)(q - base) >> 2;
}

// ---- ascending bitonic sort of one value per lane (64 lanes).  The partner of a compare-exchange at distance 1, 2 and 8 is
// a DPP operand of the min / max themselves (quad_perm / row_ror:8), at distance 4 two bank-masked DPP moves, at 16 a
// ds_swizzle, at 32 a ds_bpermute; which lanes keep the minimum is a lane pattern, i.e. a 64-bit constant per stage fed to
// v_cndmask as a scalar mask.  3 - 5 vector instructions per stage (21 stages) against ~ 7 with __shfl_xor and a computed
// direction.
constexpr unsigned long long bitonic_keep_min_mask(int kk, int j) {
    unsigned long long m = 0;
    for (int lane = 0; lane < 64; ++lane)
        if (((lane & j) == 0) == ((lane & kk) == 0)) m |= 1ull << lane;
    return m;
}
template <int KK, int J>
__device__ __forceinline__ float bitonic_stage(float v, int lane) {
    constexpr unsigned long long KEEP_MIN = bitonic_keep_min_mask(KK, J);
    float lo, hi;
    if constexpr (J == 1) {
        asm("s_nop 1\n\tv_min_f32_dpp %0, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf\n\t"
            "v_max_f32_dpp %1, %2, %2 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf" : "=&v"(lo), "=&v"(hi) : "v"(v));
    } else if constexpr (J == 2) {
        asm("s_nop 1\n\tv_min_f32_dpp %0, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf\n\t"
            "v_max_f32_dpp %1, %2, %2 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf" : "=&v"(lo), "=&v"(hi) : "v"(v));
    } else if constexpr (J == 8) {
        asm("s_nop 1\n\tv_min_f32_dpp %0, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf\n\t"
            "v_max_f32_dpp %1, %2, %2 row_ror:8 row_mask:0xf bank_mask:0xf" : "=&v"(lo), "=&v"(hi) : "v"(v));
    } else {
        float pv;
        if constexpr (J == 4) {   // lanes 0-3 / 8-11 of a row take lane + 4, lanes 4-7 / 12-15 lane - 4
            pv = v;
            asm("s_nop 1\n\tv_mov_b32_dpp %0, %1 row_shl:4 row_mask:0xf bank_mask:0x5\n\t"
                "v_mov_b32_dpp %0, %1 row_shr:4 row_mask:0xf bank_mask:0xa" : "+&v"(pv) : "v"(v));   // early clobber: %0 is
            // written by the first move before the second reads %1 -- the two must never share a register
        } else if constexpr (J == 16) {
            pv = __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x401f));   // bit mode: and 0x1f, or 0, xor 0x10
        } else {
            pv = __shfl_xor(v, J);
        }
        lo = fminf(v, pv);
        hi = fmaxf(v, pv);
    }
    // (the mask is materialised next to its use: as an "s" operand the 21 constants are hoisted out of the pair loop -- 42 scalar
    // registers, which the allocator then parks in vector lanes and fetches back with two v_readlane per stage)
    float r;
    asm("s_mov_b32 vcc_lo, %3\n\ts_mov_b32 vcc_hi, %4\n\tv_cndmask_b32_e32 %0, %1, %2, vcc"
        : "=v"(r) : "v"(hi), "v"(lo), "n"((unsigned)(KEEP_MIN & 0xffffffffull)), "n"((unsigned)(KEEP_MIN >> 32)) : "vcc");
    (void)lane;
    return r;
}
__device__ __forceinline__ float bitonic_sort64(float v, int lane) {
    v = bitonic_stage<2, 1>(v, lane);
    v = bitonic_stage<4, 2>(v, lane);   v = bitonic_stage<4, 1>(v, lane);
    v = bitonic_stage<8, 4>(v, lane);   v = bitonic_stage<8, 2>(v, lane);   v = bitonic_stage<8, 1>(v, lane);
    v = bitonic_stage<16, 8>(v, lane);  v = bitonic_stage<16, 4>(v, lane);  v = bitonic_stage<16, 2>(v, lane);  v = bitonic_stage<16, 1>(v, lane);
    v = bitonic_stage<32, 16>(v, lane); v = bitonic_stage<32, 8>(v, lane);  v = bitonic_stage<32, 4>(v, lane);  v = bitonic_stage<32, 2>(v, lane);
    v = bitonic_stage<32, 1>(v, lane);
    v = bitonic_stage<64, 32>(v, lane); v = bitonic_stage<64, 16>(v, lane); v = bitonic_stage<64, 8>(v, lane);  v = bitonic_stage<64, 4>(v, lane);
    v = bitonic_stage<64, 2>(v, lane);  v = bitonic_stage<64, 1>(v, lane);
    return v;
}

// ---------------------------------------------------------------------------------------------
// Resampler: one wave per (ray, layer).
// ---------------------------------------------------------------------------------------------
// floats of LDS per wave of resample_kernel
__host__ __device__ __forceinline__ int resample_lds_floats(int n1, int n2) {
    return pow2_above(n1) + pow2_above(n1 - 1) + pow2_above(n2) + 2 * n1 + n1 + n2;
}

struct ResampleArgs {
    const float* t;
    const float* weights;
    int64_t n;
    int l, n1, n2;
    const float* u;
    uint64_t seed;
    RayWindow win;
    const float* rays;
    int ray_stride;
    EditArgs ed;
    const uint8_t* mask;   // [n][l] or null: bit 1 = the sampler's "every depth of this pair is -1000" hint -> the pair is skipped
    float* t_fine;
    float* xyz_fine;
    float* z_new;
    int32_t* inds;
    float* cdf_out;
    RotArgs rot;           // per-layer rotations (include/stnerf.h); last, and read by the non-PLAIN flavours only
};

// NB1 > 0: the coarse list fits NB1 blocks of 64 lanes and is software pipelined -- the depths, weights and ray of pair
// i + 1 are in flight (in registers) while pair i is worked on.  The kernel is otherwise a chain of dependent round
// trips per pair ("are all depths -1000?" -> "stage depths and weights" -> compute -> stores) with ~ 150 instructions
// between them: measured, 80 % of a pair's cycles were waits for the first two (tools/resample_phase_prof.py).
// NB1 = 0: lists of any length, loads where they are needed.
// EXACT: n1 = 64 * NB1 and n2 = 64 (every BASELINE configuration: 64+64, 128+64) are compile-time constants -- the lane
// predicates (k < n1, k < n1 - 2, lane < n2, ...) fold away instead of living as 64-bit masks in spilled scalar registers,
// the searches unroll onto immediate LDS offsets: -30 % vector instructions (rocprofv3 SQ_INSTS_VALU), -25 % time.
// PLAIN: the production call -- device draws, no debug outputs, no box edits.  The arguments of the other flavours (u, z_new,
// inds, cdf, the edit table) are then dead: a third of this kernel's vector instructions were v_readlane / v_writelane
// traffic of scalar registers spilled into vector lanes, most of it kernel arguments it never uses on this path.
template <int NB1, bool PLAIN, bool EXACT>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(NB1 >= 4 ? 6 : NB1 >= 2 ? 7 : STNERF_WAVES_RESAMPLE, 8))) resample_kernel(ResampleArgs a) {
    const float* const u_in = PLAIN ? nullptr : a.u;
    float* const z_out = PLAIN ? nullptr : a.z_new;
    int32_t* const inds_out = PLAIN ? nullptr : a.inds;
    float* const cdf_dbg = PLAIN ? nullptr : a.cdf_out;
    const bool edited = PLAIN ? false : a.ed.any != 0;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // uniform: the pair index, its 64-bit divisions and
                                                                        // the RNG key of the pair stay on the scalar unit
    const int n1 = EXACT ? 64 * NB1 : a.n1, n2 = EXACT ? 64 : a.n2, S = n1 + n2, nb = n1 - 1;  // nb = #bins = len(cdf)
    // the three searched arrays are padded with +inf to (a power of two) - 1 entries, once (upper_bound_padded)
    const int P1 = pow2_above(n1), PC = pow2_above(nb), P2 = pow2_above(n2);
    float* mine = reinterpret_cast<float*>(smem_raw) + (size_t)wave * resample_lds_floats(n1, n2);
    float* tc = mine;          // [n1 | pad to P1]  coarse depths
    float* cdf = tc + P1;      // [n1-1 | pad to PC]
    float* zs = cdf + PC;      // [n2 | pad to P2]
    float* bins = zs + P2;     // [n1-1]
    float* wv = bins + n1;     // [n1-2] pdf numerators w + 1e-5
    float* tf = wv + n1;       // [S]
    for (int k = n1 + lane; k < P1; k += 64) tc[k] = __builtin_inff();
    for (int k = nb + lane; k < PC; k += 64) cdf[k] = __builtin_inff();
    for (int k = n2 + lane; k < P2; k += 64) zs[k] = __builtin_inff();
    const int p2_n1 = floor_pow2(n1);
    const int64_t pairs = a.n * a.l;
    const int64_t per_iter = (int64_t)gridDim.x * 4;
    constexpr int NBR = NB1 > 0 ? NB1 : 1;
    struct Pre {
        float t[NBR], w[NBR], r;   // r: lane i < 6 holds component i of the ray (origin, direction)
        int m;                     // the pair's mask byte (every lane), fetched with the rest: no round trip of its own
    };
    auto issue = [&](Pre& q, int64_t pr, int64_t ray_of_pr) {
        q.m = (a.mask && pr < pairs) ? (int)a.mask[pr] : 0;
        if (NB1 > 0 && pr < pairs) {
            const float* tsrc = a.t + pr * n1;
            const float* wsrc = a.weights + pr * n1;
#pragma unroll
            for (int b = 0; b < NBR; ++b) {
                const int k = b * 64 + lane;
                q.t[b] = tsrc[k < n1 ? k : n1 - 1];
                q.w[b] = wsrc[k + 1 < n1 ? k + 1 : n1 - 1];   // (the caller's w[..., 1:-1]: numerator k is weight k + 1)
            }
            q.r = a.rays[ray_of_pr * a.ray_stride + (lane < 6 ? lane : 5)];
        }
    };
    Pre nxt_in;
#pragma unroll
    for (int b = 0; b < NBR; ++b) nxt_in.t[b] = nxt_in.w[b] = 0.f;
    nxt_in.r = 0.f;
    nxt_in.m = 0;
    // (ray, layer) of the wave's pair are carried along instead of divided out of the pair index every iteration: a 64-bit
    // division is ~ 80 scalar + vector instructions, and there were two per pair
    const int64_t dray = per_iter / a.l;
    const int dlayer = (int)(per_iter - dray * a.l);
    int64_t ray_n = ((int64_t)blockIdx.x * 4 + wave) / a.l;
    int layer_n = (int)((int64_t)blockIdx.x * 4 + wave - ray_n * a.l);
    issue(nxt_in, (int64_t)blockIdx.x * 4 + wave, ray_n);
    CP_DECL
    for (int64_t p0 = (int64_t)blockIdx.x * 4; p0 < pairs; p0 += per_iter) {
        const int64_t pr = p0 + wave;
        CP(7);
        const Pre in = nxt_in;
        const int64_t ray = ray_n;
        const int layer = layer_n;
        ray_n += dray;
        layer_n += dlayer;
        if (layer_n >= a.l) {
            layer_n -= a.l;
            ++ray_n;
        }
        issue(nxt_in, pr + per_iter, ray_n);
        __builtin_amdgcn_sched_barrier(0);  // the next pair's loads go out ahead of this pair's arithmetic
        const bool active = pr < pairs;
        // the sampler flagged the pair as missed (include/stnerf.h): nothing of it is read downstream -- nothing is written
        if (active && !z_out && !inds_out && !cdf_dbg && (__builtin_amdgcn_readfirstlane(in.m) & 2)) continue;
        bool sorted_z = false;
        float o0 = 0.f, o1 = 0.f, o2 = 0.f, d0 = 0.f, d1 = 0.f, d2 = 0.f;
        if (active) {
            if (NB1 > 0) {
                o0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(in.r), 0));
                o1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(in.r), 1));
                o2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(in.r), 2));
                d0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(in.r), 3));
                d1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(in.r), 4));
                d2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(in.r), 5));
            } else {
                const float* r = a.rays + ray * a.ray_stride;
                o0 = r[0], o1 = r[1], o2 = r[2], d0 = r[3], d1 = r[4], d2 = r[5];
            }
            // a rotated layer's points are those of the ray in the layer's frame (the depths are the ray's own): before the
            // all-missed shortcut's point and the fine points below
            if (!PLAIN && (a.rot.on >> layer & 1)) {
                float o[3] = {o0, o1, o2}, d[3] = {d0, d1, d2};
                rotate_ray(a.rot.m[layer], a.rot.c[layer], o, d);
                o0 = o[0], o1 = o[1], o2 = o[2], d0 = d[0], d1 = d[1], d2 = d[2];
            }
        }
        // ---- a layer the ray misses altogether: every coarse depth is -1000 (bin width 0), so every bin edge and every
        // resampled depth is exactly -1000 whatever the draws; write that and skip the work (60 % of the performer
        // pairs of a typical view).  The optional debug outputs take the general path.
        if (active && !z_out && !inds_out && !cdf_dbg) {
            const float* tsrc = a.t + pr * n1;
            bool missed = true;
            if (NB1 > 0) {
#pragma unroll
                for (int b = 0; b < NBR; ++b) missed = missed && in.t[b] == -1000.f;   // (idle lanes hold the last depth)
            } else {
                for (int k = lane; k < n1; k += 64) missed = missed && tsrc[k] == -1000.f;
            }
            if (__all(missed)) {
                float x = -1000.f * d0 + o0, y = -1000.f * d1 + o1, w = -1000.f * d2 + o2;  // :465
                if (edited) unedit_point(x, y, w, a.ed.e[layer], a.ed.pivot);
                for (int m = lane; m < S; m += 64) {
                    a.t_fine[pr * S + m] = -1000.f;
                    if (a.xyz_fine) {
                        float* dst = a.xyz_fine + (pr * S + m) * 3;
                        dst[0] = x;
                        dst[1] = y;
                        dst[2] = w;
                    }
                }
                CP(0);
                continue;
            }
        }
        CP(0);
        // ---- pdf / cdf / bins   (sample_pdf.py:20-24; the caller passes w[..., 1:-1], layered_rfrender.py:460)
        if (active) {
            if (NB1 > 0) {
#pragma unroll
                for (int b = 0; b < NBR; ++b) {
                    const int k = b * 64 + lane;
                    if (k < n1) tc[k] = in.t[b];
                    if (k < n1 - 2) wv[k] = in.w[b] + 1e-5f;  // weights + 1e-5 (sample_pdf.py:21)
                }
            } else {
                const float* tsrc = a.t + pr * n1;
                const float* wsrc = a.weights + pr * n1;
                for (int k = lane; k < n1; k += 64) tc[k] = tsrc[k];
                for (int k = lane; k < n1 - 2; k += 64) wv[k] = wsrc[k + 1] + 1e-5f;  // weights + 1e-5 (sample_pdf.py:21)
            }
        }
        wave_sync();
        CP(1);
        if (active) {
            // pdf = w / torch.sum(w) in ATen's CPU summation order; cdf = torch.cumsum(pdf): ATen's CPU cumsum
            // accumulates fp32 rows in DOUBLE and rounds every prefix to fp32 (cumsum_cpu_kernel: at::acc_type<float,
            // false>).  The pdf values are fp32 numbers in [2^-17, 1], so every fp64 partial sum is exact and the
            // parallel scan below yields the sequential loop's bits: cdf, and with it inds and z, are bit-equal to the
            // reference's CPU evaluation for the same (t, w, u).
            const float total = aten_cpu_row_sum(wv, n1 - 2, lane);
            double carry = 0.0;
            if (lane == 0) cdf[0] = 0.f;
            for (int base = 0; base < n1 - 2; base += 64) {
                const int k = base + lane;
                const double pdf = (k < n1 - 2) ? (double)(wv[k] / total) : 0.0;
                const double incl = wave_scan_add_f64(pdf);
                if (k < n1 - 2) cdf[k + 1] = (float)(carry + incl);
                carry = carry + __longlong_as_double(((long long)__builtin_amdgcn_readlane((int)(__double_as_longlong(incl) >> 32), 63) << 32) |
                                                     (unsigned int)__builtin_amdgcn_readlane((int)(__double_as_longlong(incl) & 0xffffffffll), 63));
            }
        }
        wave_sync();
        CP(2);
        if (active) {
            for (int k = lane; k < nb; k += 64) bins[k] = 0.5f * (tc[k + 1] + tc[k]);
            if (cdf_dbg)
                for (int k = lane; k < nb; k += 64) cdf_dbg[pr * nb + k] = cdf[k];
        }
        wave_sync();
        CP(3);
        // ---- invert the cdf (sample_pdf.py:44-61)
        if (active) {
            const uint64_t gray = u_in ? 0ull : (uint64_t)global_ray(a.win, ray);  // (wave-uniform)
            for (int j = lane; j < n2; j += 64) {
                const float u = u_in ? u_in[((int64_t)layer * a.n + ray) * n2 + j]
                                    : philox_uniform(a.seed, gray, (uint32_t)layer, 1u, (uint32_t)j);
                const int ind = upper_bound_padded(cdf, 2 * PC, u);   // searchsorted(right=True)
                const int below = ind - 1 > 0 ? ind - 1 : 0;
                const int above = ind < nb - 1 ? ind : nb - 1;
                float den = cdf[above] - cdf[below];
                if (den < 1e-5f) den = 1.f;
                const float frac = (u - cdf[below]) / den;
                const float z = bins[below] + frac * (bins[above] - bins[below]);
                zs[j] = z;
                if (z_out) z_out[pr * n2 + j] = z;
                if (inds_out) inds_out[pr * n2 + j] = ind;
            }
        }
        wave_sync();
        CP(4);
        // ---- sort(cat[t, z])  (layered_rfrender.py:462) by ranks == a stable sort with t before z on ties.
        // The coarse list is ascending (unless a box edit made the bin width negative), so a t keeps its index
        // plus the number of smaller z, and a z its index among the sorted z plus the number of t <= z.  Up to 64
        // new samples are sorted in registers (bitonic network over the wave's lanes); equal z are interchangeable
        // because only values leave this kernel.
        if (active) {
            bool desc = false, ndesc = false;
            for (int k = lane; k + 1 < n1; k += 64) {
                desc = desc || (tc[k + 1] < tc[k]);
                ndesc = ndesc || !(tc[k + 1] < tc[k]);
            }
            bool asc = !__any(desc);
            if (!asc && !__any(ndesc)) {
                // strictly descending coarse list (negative bin width: a ray that misses the background box, or an
                // edited box): only the sorted VALUES leave this kernel and bins / cdf are done with, so turn the
                // list round in place and take the sorted path
                for (int k = lane; k < n1 / 2; k += 64) {
                    const float lo = tc[k], hi = tc[n1 - 1 - k];
                    tc[k] = hi;
                    tc[n1 - 1 - k] = lo;
                }
                wave_sync();
                asc = true;
            }
            if (asc && n2 <= 64) {
                const float v = bitonic_sort64(lane < n2 ? zs[lane] : __builtin_inff(), lane);
                if (lane < n2) {
                    zs[lane] = v;  // now ascending
                    tf[lane + upper_bound_padded(tc, 2 * P1, v)] = v;
                }
            }
            sorted_z = asc && n2 <= 64;
        }
        wave_sync();
        if (active) {
            if (sorted_z) {
                for (int k = lane; k < n1; k += 64) {
                    const float v = tc[k];
                    tf[k + lower_bound_padded(zs, 2 * P2, v)] = v;
                }
            } else {
                bool desc = false;
                for (int k = lane; k + 1 < n1; k += 64) desc = desc || (tc[k + 1] < tc[k]);
                const bool asc = !__any(desc);
                for (int e = lane; e < S; e += 64) {
                    const bool is_t = e < n1;
                    const float v = is_t ? tc[e] : zs[e - n1];
                    int rank;
                    if (asc) {
                        rank = is_t ? e : upper_bound_lds(tc, n1, p2_n1, v);
                    } else {
                        rank = 0;
                        for (int x = 0; x < n1; ++x) {
                            const float xv = tc[x];
                            rank += (xv < v || (xv == v && (!is_t || x < e))) ? 1 : 0;
                        }
                    }
                    for (int x = 0; x < n2; ++x) {
                        const float xv = zs[x];
                        rank += (xv < v || (xv == v && !is_t && x < e - n1)) ? 1 : 0;
                    }
                    tf[rank] = v;
                }
            }
        }
        wave_sync();
        CP(5);
        if (active) {
            for (int m = lane; m < S; m += 64) {
                const float z = tf[m];
                a.t_fine[pr * S + m] = z;
                if (a.xyz_fine) {
                    float x = z * d0 + o0, y = z * d1 + o1, w = z * d2 + o2;  // :465
                    if (edited) unedit_point(x, y, w, a.ed.e[layer], a.ed.pivot);
                    float* dst = a.xyz_fine + (pr * S + m) * 3;  // (staging these through LDS for 16-B stores measured slower)
                    dst[0] = x;
                    dst[1] = y;
                    dst[2] = w;
                }
            }
        }
        wave_sync();
        CP(6);
    }
    CP_FLUSH;
}

}  // namespace stnerf

using namespace stnerf;

#ifdef STNERF_COMP_PROF
extern "C" int stnerf_debug_resample_phases(unsigned long long* host8, int reset) {
    if (hipMemcpyFromSymbol(host8, HIP_SYMBOL(g_cphase), sizeof(unsigned long long) * 8) != hipSuccess) return STNERF_ELAUNCH;
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_cphase), z, sizeof(z)) != hipSuccess) return STNERF_ELAUNCH;
    }
    return STNERF_OK;
}
#endif

extern "C" int stnerf_resample(const float* t, const float* weights, int64_t n, int l, int n1, int n2, const float* u,
                               uint64_t seed, int64_t ray_index_base, int64_t ray_index_stripe, int64_t ray_index_period,
                               const float* rays, int ray_stride,
                               const stnerf_layer_edit* edits_host, const float* pivot_host, const uint8_t* mask, float* t_fine,
                               float* xyz_fine, float* z_new, int32_t* inds, float* cdf, stnerf_stream_t stream) {
    return stnerf_resample_rot(t, weights, n, l, n1, n2, u, seed, ray_index_base, ray_index_stripe, ray_index_period, rays, ray_stride,
                               edits_host, pivot_host, nullptr, mask, t_fine, xyz_fine, z_new, inds, cdf, stream);
}

extern "C" int stnerf_resample_rot(const float* t, const float* weights, int64_t n, int l, int n1, int n2, const float* u,
                                   uint64_t seed, int64_t ray_index_base, int64_t ray_index_stripe, int64_t ray_index_period,
                                   const float* rays, int ray_stride,
                                   const stnerf_layer_edit* edits_host, const float* pivot_host,
                                   const stnerf_layer_rotation* rotations_host, const uint8_t* mask, float* t_fine,
                                   float* xyz_fine, float* z_new, int32_t* inds, float* cdf, stnerf_stream_t stream) {
    STNERF_REQUIRE(t && weights && rays && t_fine, "resample: null pointer");
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && n1 >= 3 && n2 >= 0 && ray_stride >= 6,
                   "resample: bad shape n=%lld l=%d n1=%d n2=%d", (long long)n, l, n1, n2);
    STNERF_REQUIRE_WINDOW("resample", ray_index_stripe, ray_index_period);
    if (n == 0) return STNERF_OK;
    ResampleArgs a;
    a.t = t; a.weights = weights; a.n = n; a.l = l; a.n1 = n1; a.n2 = n2; a.u = u; a.seed = seed;
    a.win = RayWindow{ray_index_base, ray_index_stripe, ray_index_period}; a.rays = rays; a.ray_stride = ray_stride;
    fill_edit_args(a.ed, edits_host, pivot_host, l);
    fill_rot_args(a.rot, rotations_host, l);
    a.mask = mask;
    a.t_fine = t_fine; a.xyz_fine = xyz_fine; a.z_new = z_new; a.inds = inds; a.cdf_out = cdf;
    const int lds = 4 * resample_lds_floats(n1, n2) * (int)sizeof(float);
    // (the +inf padding of the branch-free searches rounds three of the arrays up to powers of two: 512+512 samples need
    // 73.7 KB for the block's four waves -- above the 64 KB a kernel gets without asking, inside the CU's 160 KB)
    STNERF_REQUIRE(lds <= 160 * 1024, "resample: %d+%d samples per ray exceed the LDS budget", n1, n2);
    int64_t blocks = (n * l + 3) / 4;
    if (blocks > 256 * 32) blocks = 256 * 32;
    LaunchTimer timer(PROF_RESAMPLE, 0, n, n1 + n2, (int64_t)l * (8ll * n1 + (xyz_fine ? 16ll : 4ll) * (n1 + n2)) + 24,
                      as_stream(stream));
    const bool plain = !u && !z_new && !inds && !cdf && !a.ed.any && !a.rot.on;
    const dim3 grid((unsigned)blocks), block(256);
    int reserve_rc = STNERF_OK;
    auto launch = [&](auto kernel) {
        if (lds > 64 * 1024) reserve_rc = reserve_dynamic_lds(reinterpret_cast<const void*>(kernel), lds, "resample");
        if (reserve_rc == STNERF_OK) hipLaunchKernelGGL(kernel, grid, block, lds, as_stream(stream), a);
    };
    const bool exact = plain && n2 == 64 && (n1 == 64 || n1 == 128);
    if (exact) n1 == 64 ? launch(resample_kernel<1, true, true>) : launch(resample_kernel<2, true, true>);
    else if (n1 <= 64) plain ? launch(resample_kernel<1, true, false>) : launch(resample_kernel<1, false, false>);
    else if (n1 <= 128) plain ? launch(resample_kernel<2, true, false>) : launch(resample_kernel<2, false, false>);
    else if (n1 <= 256) plain ? launch(resample_kernel<4, true, false>) : launch(resample_kernel<4, false, false>);
    else launch(resample_kernel<0, false, false>);
    if (reserve_rc) return reserve_rc;
    STNERF_CHECK_LAUNCH("resample");
    return STNERF_OK;
}
