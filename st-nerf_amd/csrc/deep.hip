// Deep frames (include/stnerf.h: stnerf_deep_count, stnerf_deep_offsets, stnerf_deep_fill, stnerf_deep_composite; DESIGN.md sections
// 4.2 and 7): the final stage's merged weights kept as a per-ray list of deep samples -- the kept samples of every layer, merged into
// depth segments -- in CSR form, and the compositing of up to eight depth-tested elements per ray on that list, after the render.
// Count and fill walk a ray alike (deep_ray_kernel<FILL>): one wave per ray over a persistent grid, a layer's t and wM loaded in
// four blocks before the first use, the segment starts found with ballots; the offsets are csrc/ordered_compact.h's one-workgroup
// scan over 256-ray block sums.  Compiled with -ffp-contract=off: every product and every sum of the definitions is one fp32 operation.
#include <math.h>

#include "common.h"
#include "composite_rules.h"
#include "ordered_compact.h"
#include "wave_prims.h"

namespace stnerf {

constexpr int kDeepMaxS = 256;   // first_k is eight bits of meta
constexpr int kDeepBlocks = kDeepMaxS / 64;

struct DeepRayArgs {
    const float* t;
    const float4* raw;
    const uint8_t* mask;
    const float* merged_weights;
    int64_t n;
    int l, S;
    stnerf_composite_params p;
    float w_min, merge_dz;
    int32_t* counts;          // count
    const int64_t* offsets;   // fill
    float4* samples;
    int64_t capacity;
    int64_t* deep_total;
};

__device__ __forceinline__ float read_lane(float v, int lane) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane)); }

// One wave per ray.  Per layer with output: the four blocks of t and wM are loaded, then walked in source order; `carry` is the bin of
// the last kept sample so far, `starts` the layer's segments so far, both wave-uniform.  FILL: the lane of a segment's first sample
// sums the segment and writes its record.
template <bool FILL>
__global__ void __launch_bounds__(256) deep_ray_kernel(DeepRayArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const unsigned long long below = (1ull << lane) - 1ull;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t first = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t LS = (int64_t)a.l * a.S;
    const EvalBits ev = eval_bits<false>(a.p, a.l);
    const bool activated = a.p.rgb_activated != 0;
    const bool merge = a.merge_dz > 0.f;
    if (FILL && blockIdx.x == 0 && threadIdx.x == 0) *a.deep_total = a.offsets[a.n];
    for (int64_t ray = first; ray < a.n; ray += stride) {
        int64_t lo = 0, hi = 0;
        if (FILL) {
            lo = a.offsets[ray];
            hi = a.offsets[ray + 1];
            if (lo < 0 || hi < lo || hi > a.capacity) continue;   // (uniform) the ray's range would pass the capacity: nothing is written
        }
        const int mv = (a.mask && (int)lane < a.l) ? (int)a.mask[ray * a.l + lane] : 0;
        const unsigned have_m = have_layers(ev, a.mask != nullptr, (unsigned)__ballot((mv & 1) != 0));
        int64_t total = 0;   // the ray's segments so far
        for (int layer = 0; layer < a.l; ++layer) {
            if (!(have_m >> layer & 1u)) continue;   // (uniform) a layer without output has no deep sample
            const float* tl = a.t + ray * LS + (int64_t)layer * a.S;
            const float* wl = a.merged_weights + ray * LS + (int64_t)layer * a.S;
            float tv[kDeepBlocks], wv[kDeepBlocks];
#pragma unroll
            for (int b = 0; b < kDeepBlocks; ++b) {   // every load of the layer is issued before the first is used
                const int k = b * 64 + (int)lane;
                tv[b] = wv[b] = 0.f;
                if (k < a.S) {
                    wv[b] = wl[k];
                    tv[b] = tl[k];
                }
            }
            bool seen = false;   // a kept sample of the layer lies in an earlier block
            float t0 = 0.f, carry = 0.f;
            int starts = 0;
#pragma unroll
            for (int b = 0; b < kDeepBlocks; ++b) {
                if (b * 64 >= a.S) break;
                const int k = b * 64 + (int)lane;
                const bool kept = k < a.S && !(wv[b] <= a.w_min);
                const unsigned long long kb = __ballot(kept);
                if (kb == 0ull) continue;   // (uniform)
                bool start = kept;
                float bin = 0.f;
                if (merge) {
                    if (!seen) t0 = read_lane(tv[b], __builtin_ctzll(kb));
                    bin = floorf((tv[b] - t0) / a.merge_dz);
                    const unsigned long long before = kb & below;
                    const int src = before ? 63 - __builtin_clzll(before) : 0;
                    const float lane_prev = __shfl(bin, src, 64);
                    const bool has_prev = before != 0ull || seen;
                    const float prev = before ? lane_prev : carry;
                    start = kept && (!has_prev || bin != prev);
                    carry = read_lane(bin, 63 - __builtin_clzll(kb));
                }
                seen = true;
                const unsigned long long sb = __ballot(start);
                if (FILL && start) {
                    const int64_t at = lo + total + starts + __popcll(sb & below);
                    const float4* rl = a.raw + ray * LS + (int64_t)layer * a.S;
                    const float tk = tv[b], wk = wv[b];
                    const float4 c = edit_sample(rl[k], tk, false, -INFINITY, 1.f, false, 0.f, activated);
                    float r = 0.f + wk * c.x, g = 0.f + wk * c.y, bl = 0.f + wk * c.z, zw = 0.f + wk * tk, al = 0.f + wk, zb = tk;
                    unsigned count = 1u;
                    if (merge)   // the samples that follow in the segment: kept, and in the head's bin
                        for (int k2 = k + 1; k2 < a.S; ++k2) {
                            const float w2 = wl[k2];
                            if (w2 <= a.w_min) continue;
                            const float t2 = tl[k2];
                            if (floorf((t2 - t0) / a.merge_dz) != bin) break;
                            const float4 c2 = edit_sample(rl[k2], t2, false, -INFINITY, 1.f, false, 0.f, activated);
                            r += w2 * c2.x;
                            g += w2 * c2.y;
                            bl += w2 * c2.z;
                            zw += w2 * t2;
                            al += w2;
                            zb = t2;
                            ++count;
                        }
                    if (at < hi) {   // (offsets that are not this call's counts: never outside the ray's own range)
                        a.samples[at * 2] = make_float4(r, g, bl, al);
                        a.samples[at * 2 + 1] = make_float4(zw, tk, zb, __uint_as_float((unsigned)layer | (unsigned)k << 8 | count << 16));
                    }
                }
                starts += __popcll(sb);
            }
            total += starts;
        }
        if (!FILL && lane == 0u) a.counts[ray] = (int32_t)total;
    }
}

// ---- the offsets: block sums, csrc/ordered_compact.h's scan of them, then the scan inside every block of 256 rays
__global__ void __launch_bounds__(kSelectBlock) deep_block_sum_kernel(const int32_t* __restrict__ counts, int64_t n, int32_t* __restrict__ block_sum) {
    __shared__ int wave_total[kSelectBlock / 64];
    const int64_t q = (int64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    int v = q < n ? counts[q] : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);   // (integers: the order is free)
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int i = 0; i < kSelectBlock / 64; ++i) tot += wave_total[i];
        block_sum[blockIdx.x] = tot;
    }
}

__global__ void __launch_bounds__(kSelectBlock) deep_offsets_kernel(const int32_t* __restrict__ counts, int64_t n,
                                                                    const int32_t* __restrict__ block_offset, int64_t* __restrict__ offsets) {
    __shared__ int wave_total[kSelectBlock / 64];
    const int64_t q = (int64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int v = q < n ? counts[q] : 0;
    int inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wave_total[wave] = inc;
    __syncthreads();
    if (q >= n) return;
    int64_t at = block_offset[blockIdx.x];
    for (int i = 0; i < wave; ++i) at += wave_total[i];
    offsets[q] = at + inc - v;
    if (q == n - 1) offsets[n] = at + inc;
}

// ---- compositing elements on the list
struct DeepCompositeArgs {
    const int64_t* offsets;
    const float4* samples;
    int64_t n;
    int l, E;
    const float* elements;
    float* mixed_out;
    float* scene_out;
    float* shares;
};

constexpr int kE = STNERF_DEEP_MAX_ELEMENTS;

// lane c < 5: channel c of five wave-uniform totals
__device__ __forceinline__ float deep_pick5(const float (&v)[5], unsigned lane) {
    return lane == 0u ? v[0] : lane == 1u ? v[1] : lane == 2u ? v[2] : lane == 3u ? v[3] : v[4];
}

// One wave per ray over a persistent grid.  The rows are ranked with E^2 wave-uniform compares and put into sorted slots with
// selects (no dynamic index: everything stays in registers).  The list is walked in blocks of 64 records; a block holds the records
// of consecutive layers, which are finished one after the other: lanes 0..4 hold the channels {r, g, b, depth, acc} of the running
// sum of the passes.
__global__ void __launch_bounds__(256) deep_composite_kernel(DeepCompositeArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t first = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int E = a.E;
    for (int64_t ray = first; ray < a.n; ray += stride) {
        // the rows, read once: lane j holds word j of the ray's E rows
        const float ew = (int)lane < E * 5 ? a.elements[ray * E * 5 + lane] : 0.f;
        float ap[kE], z[kE];   // by the rows' own index; an absent row: a' = 0, z = +inf (it sorts last and hides nothing)
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            ap[e] = 0.f;
            z[e] = INFINITY;
            if (e < E) {
                const float oa = read_lane(ew, e * 5 + 3), oz = read_lane(ew, e * 5 + 4);
                float c = oa > 0.f ? oa : 0.f;
                c = c < 1.f ? c : 1.f;
                if (c > 0.f && fabsf(oz) < INFINITY) {
                    ap[e] = c;
                    z[e] = oz;
                }
            }
        }
        int rank[kE];
#pragma unroll
        for (int e = 0; e < kE; ++e) {
            rank[e] = 0;
#pragma unroll
            for (int f = 0; f < kE; ++f)
                if (f != e && f < E) rank[e] += (z[f] < z[e] || (z[f] == z[e] && f < e)) ? 1 : 0;
        }
        float zs[kE], as[kE], P[kE + 1];   // the sorted slots; P_j = the product of (1 - a') over the slots before j
        P[0] = 1.f;
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            zs[j] = INFINITY;
            as[j] = 0.f;
#pragma unroll
            for (int e = 0; e < kE; ++e)
                if (e < E && rank[e] == j) {
                    zs[j] = z[e];
                    as[j] = ap[e];
                }
            P[j + 1] = P[j] * (1.f - as[j]);
        }
        const int64_t lo = a.offsets[ray], hi = a.offsets[ray + 1];
        float af[kE];   // this lane's part of Af_j
#pragma unroll
        for (int j = 0; j < kE; ++j) af[j] = 0.f;
        float sum = 0.f;   // lanes 0..4: ((pass_0 + pass_1) + ..) of this lane's channel
        int cur = 0;       // the layer being summed (uniform)
        CompositeAcc A;
        auto finish = [&](int layer, const float (&tot)[5]) {
            const float pass = deep_pick5(tot, lane);
            sum = layer == 0 ? pass : sum + pass;
            if (a.scene_out && lane < 5u) a.scene_out[(ray * a.l + layer) * 5 + lane] = pass;
        };
        for (int64_t d0 = lo; d0 < hi; d0 += 64) {
            const int64_t d = d0 + lane;
            const bool in = d < hi;
            float4 u = make_float4(0.f, 0.f, 0.f, 0.f), v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in) {
                u = a.samples[d * 2];
                v = a.samples[d * 2 + 1];
            }
            int layer = in ? (int)(__float_as_uint(v.w) & 0xffu) : 0x7fffffff;
            if (layer >= a.l && in) layer = a.l - 1;   // (a record that is not this library's: no store outside scene_out)
            const float zf = v.y;
            float q = 1.f;
#pragma unroll
            for (int j = 0; j < kE; ++j) {
                if (j < E) {
                    const bool behind = zf >= zs[j];   // (a NaN zf is in front; an absent slot: z = +inf, a' = 0)
                    q = behind ? P[j + 1] : q;
                    if (in) af[j] = af[j] + (behind ? 0.f : u.w);
                }
            }
            for (;;) {   // (uniform) the layers of the block, in order
                if (in && layer == cur) {
                    A.cr += q * u.x;
                    A.cg += q * u.y;
                    A.cb += q * u.z;
                    A.cd += q * v.x;
                    A.ca += q * u.w;
                }
                const unsigned long long later = __ballot(in && layer > cur);
                if (later == 0ull) break;
                float tot[5];
                composite_total5(A, tot);
                finish(cur, tot);
                A = CompositeAcc();
                const int next = __builtin_amdgcn_readlane(layer, __builtin_ctzll(later));
                const float zero[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
                for (int i = cur + 1; i < next; ++i) finish(i, zero);
                cur = next;
            }
        }
        {
            float tot[5];
            composite_total5(A, tot);
            finish(cur, tot);
            const float zero[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
            for (int i = cur + 1; i < a.l; ++i) finish(i, zero);
        }
        // the rows' shares, slot by slot in sorted order
        float share[kE];
#pragma unroll
        for (int j = 0; j < kE; ++j) {
            share[j] = 0.f;
            if (j < E) {
                const float Af = wave_last(wave_scan_add(af[j]));
                const float left = 1.f - Af;
                const float T = left > 0.f ? left : 0.f;   // (a NaN leaves nothing)
                const float s = (as[j] * T) * P[j];
                float x = 1.f;   // this lane's channel of the slot's row {r, g, b, z, 1}
#pragma unroll
                for (int e = 0; e < kE; ++e)
                    if (e < E && rank[e] == j) {
                        const float own = __shfl(ew, e * 5 + (int)(lane < 3u ? lane : 0u), 64);
                        x = lane < 3u ? own : lane == 3u ? zs[j] : 1.f;
                    }
                share[j] = as[j] > 0.f ? s * x : 0.f;   // (an absent row: five exact zeros, whatever its words hold)
                sum = sum + share[j];
            }
        }
        if (lane < 5u) {
            a.mixed_out[ray * 5 + lane] = sum;
            if (a.shares) {
#pragma unroll
                for (int e = 0; e < kE; ++e)
                    if (e < E) {
                        float sv = 0.f;
#pragma unroll
                        for (int j = 0; j < kE; ++j) sv = rank[e] == j ? share[j] : sv;
                        a.shares[(ray * E + e) * 5 + lane] = sv;
                    }
            }
        }
    }
}

static int check_deep_ray(const char* what, const float* t, const float* merged_weights, int64_t n, int l, int S,
                          const stnerf_composite_params* params_host, float w_min, float merge_dz) {
    STNERF_REQUIRE(t && merged_weights && params_host, "%s: null pointer", what);
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && S >= 1 && S <= kDeepMaxS, "%s: bad shape n=%lld l=%d S=%d (S <= %d)", what,
                   (long long)n, l, S, kDeepMaxS);
    STNERF_REQUIRE(w_min >= 0.f, "%s: w_min = %g is negative or NaN", what, (double)w_min);
    STNERF_REQUIRE(merge_dz >= 0.f, "%s: merge_dz = %g is negative or NaN", what, (double)merge_dz);
    return STNERF_OK;
}

static unsigned ray_blocks(int64_t n) {
    const int64_t blocks = (n + 3) / 4;
    return (unsigned)(blocks > 256 * 16 ? 256 * 16 : blocks);
}

}  // namespace stnerf

using namespace stnerf;

extern "C" int64_t stnerf_deep_workspace_bytes(int64_t n) {
    if (n < 0) {
        set_error("deep_workspace_bytes: n = %lld", (long long)n);
        return STNERF_EINVAL;
    }
    return select_workspace_bytes(n) + 256;   // the block sums, then the scan's total
}

extern "C" int stnerf_deep_count(const float* t, const uint8_t* mask, const float* merged_weights, int64_t n, int l, int S,
                                 const stnerf_composite_params* params_host, float w_min, float merge_dz, int32_t* counts, stnerf_stream_t stream) {
    const int rc = check_deep_ray("deep_count", t, merged_weights, n, l, S, params_host, w_min, merge_dz);
    if (rc) return rc;
    STNERF_REQUIRE(counts, "deep_count: null pointer");
    if (n == 0) return STNERF_OK;
    hipStream_t st = as_stream(stream);
    DeepRayArgs a{t, nullptr, mask, merged_weights, n, l, S, *params_host, w_min, merge_dz, counts, nullptr, nullptr, 0, nullptr};
    {
        LaunchTimer timer(PROF_DEEP_COUNT, 0, n, S, 8ll * l * S + l + 4, st);
        hipLaunchKernelGGL(deep_ray_kernel<false>, dim3(ray_blocks(n)), dim3(256), 0, st, a);
    }
    STNERF_CHECK_LAUNCH("deep_count");
    return STNERF_OK;
}

extern "C" int stnerf_deep_offsets(const int32_t* counts, int64_t n, int64_t max_count, int64_t* offsets, void* workspace, int64_t workspace_bytes,
                                   stnerf_stream_t stream) {
    STNERF_REQUIRE(counts && offsets, "deep_offsets: null pointer");
    STNERF_REQUIRE(n >= 0 && max_count >= 0 && (max_count == 0 || n <= (int64_t)INT32_MAX / max_count),
                   "deep_offsets: n = %lld rays of up to %lld records exceed the 2^31 - 1 records of one call", (long long)n, (long long)max_count);
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemsetAsync(offsets, 0, sizeof(int64_t), st) != hipSuccess) {
            set_error("deep_offsets: hipMemsetAsync failed");
            return STNERF_ELAUNCH;
        }
        return STNERF_OK;
    }
    STNERF_REQUIRE(workspace && workspace_bytes >= stnerf_deep_workspace_bytes(n) && ((uintptr_t)workspace & 3) == 0,
                   "deep_offsets: the workspace holds %lld bytes, %lld are needed (4-byte aligned)", (long long)workspace_bytes,
                   (long long)stnerf_deep_workspace_bytes(n));
    int32_t* blocks = static_cast<int32_t*>(workspace);
    int32_t* total = reinterpret_cast<int32_t*>(static_cast<char*>(workspace) + select_workspace_bytes(n));
    const int64_t nb = select_blocks(n);
    LaunchTimer timer(PROF_DEEP_OFFSETS, 0, n, 1, 12, st);
    hipLaunchKernelGGL(deep_block_sum_kernel, dim3((unsigned)nb), dim3(kSelectBlock), 0, st, counts, n, blocks);
    STNERF_CHECK_LAUNCH("deep_offsets (block sums)");
    hipLaunchKernelGGL(select_scan_kernel<kScanBlock>, dim3(1), dim3(kScanBlock), 0, st, blocks, nb, total);
    STNERF_CHECK_LAUNCH("deep_offsets (scan)");
    hipLaunchKernelGGL(deep_offsets_kernel, dim3((unsigned)nb), dim3(kSelectBlock), 0, st, counts, n, (const int32_t*)blocks, offsets);
    STNERF_CHECK_LAUNCH("deep_offsets");
    return STNERF_OK;
}

extern "C" int stnerf_deep_fill(const float* t, const float* raw, const uint8_t* mask, const float* merged_weights, int64_t n, int l, int S,
                                const stnerf_composite_params* params_host, float w_min, float merge_dz, const int64_t* offsets, float* samples,
                                int64_t capacity, int64_t* deep_total, stnerf_stream_t stream) {
    const int rc = check_deep_ray("deep_fill", t, merged_weights, n, l, S, params_host, w_min, merge_dz);
    if (rc) return rc;
    STNERF_REQUIRE(raw && offsets && deep_total && (samples || capacity == 0), "deep_fill: null pointer");
    STNERF_REQUIRE(capacity >= 0, "deep_fill: capacity = %lld", (long long)capacity);
    STNERF_REQUIRE((((uintptr_t)raw | (uintptr_t)samples) & 15) == 0, "deep_fill: raw and samples must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    if (n == 0) {
        if (hipMemcpyAsync(deep_total, offsets, sizeof(int64_t), hipMemcpyDeviceToDevice, st) != hipSuccess) {
            set_error("deep_fill: hipMemcpyAsync failed");
            return STNERF_ELAUNCH;
        }
        return STNERF_OK;
    }
    DeepRayArgs a{t, reinterpret_cast<const float4*>(raw), mask, merged_weights, n, l, S, *params_host, w_min, merge_dz, nullptr, offsets,
                  reinterpret_cast<float4*>(samples), capacity, deep_total};
    {
        LaunchTimer timer(PROF_DEEP_FILL, 0, n, S, 24ll * l * S + l + 16, st);
        hipLaunchKernelGGL(deep_ray_kernel<true>, dim3(ray_blocks(n)), dim3(256), 0, st, a);
    }
    STNERF_CHECK_LAUNCH("deep_fill");
    return STNERF_OK;
}

extern "C" int stnerf_deep_composite(const int64_t* offsets, const float* samples, int64_t n, int l, const float* elements, int E,
                                     float* mixed_out, float* scene_out, float* shares, stnerf_stream_t stream) {
    STNERF_REQUIRE(offsets && mixed_out, "deep_composite: null pointer");
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS, "deep_composite: bad shape n=%lld l=%d", (long long)n, l);
    STNERF_REQUIRE(E >= 0 && E <= STNERF_DEEP_MAX_ELEMENTS, "deep_composite: E = %d elements per ray, 0..%d are built", E, STNERF_DEEP_MAX_ELEMENTS);
    STNERF_REQUIRE(E == 0 || elements, "deep_composite: %d elements per ray but no rows", E);
    STNERF_REQUIRE(((uintptr_t)samples & 15) == 0, "deep_composite: samples must be 16-byte aligned");
    if (n == 0) return STNERF_OK;
    hipStream_t st = as_stream(stream);
    DeepCompositeArgs a{offsets, reinterpret_cast<const float4*>(samples), n, l, E, elements, mixed_out, scene_out, shares};
    {
        LaunchTimer timer(PROF_DEEP_COMPOSITE, E, n, 1, 16 + 20ll * (1 + E + (scene_out ? l : 0) + (shares ? E : 0)), st);
        hipLaunchKernelGGL(deep_composite_kernel, dim3(ray_blocks(n)), dim3(256), 0, st, a);
    }
    STNERF_CHECK_LAUNCH("deep_composite");
    return STNERF_OK;
}
