// stnerf_copy_layer_raw_listed: the compact sibling of stnerf_copy_layer_raw (csrc/pipeline.hip), for the layer cache
// (include/stnerf.h: stnerf_layer_cache).  A performer covers a fraction of the view, so its cached raw
// outputs follow its hit rays: slot j of dense[capacity][ns][4] holds raw[rays[j]][layer], and rays[] / *count are the list the
// slice was captured under.  HBM-bound: 32 ns + 4 bytes per slot.
#include "common.h"

using namespace stnerf;

namespace {

constexpr int SLOTS_IN_FLIGHT = 4;   // independent slots per wave and trip: at ns = 64 four 1 KB runs in flight per wave

// One WAVE moves one slot: the ns float4s of a (ray, layer) pair are contiguous in raw and in dense, so a wave instruction is one
// run of up to 1 KB on both sides.  The slot's ray index is one wave-uniform load; lane `lane` takes samples lane, lane + 64, ..:
// no integer division.  A persistent grid strides over the slots; the count is read here, on the device.  64-bit indices (a 1080p
// view at 64 + 64 samples has 2.7e8 samples per layer).
//   TO_DENSE (capture): list / count_in = the frame's ray list of the layer; writes dense, rays_out and *count_out (= the count, or
//     -1 and nothing else when it does not fit `capacity`).  rays_out may BE list and count_out count_in (the fine capture walks the
//     list the coarse one kept): they are then left as they are.
//   !TO_DENSE (restore): list / count_in = the entry's rays / count; writes raw[list[j]][layer] for j < count and nothing else; a
//     negative count, or one above capacity, copies nothing.  mismatch (optional) += 1 when *frame_count differs from the count.
// A ray index outside [0, n) is skipped (never produced by the library; a guard for the buffers).
template <bool TO_DENSE>
__global__ void __launch_bounds__(256) copy_layer_raw_listed_kernel(float4* __restrict__ raw, float4* __restrict__ dense,
                                                                    const int32_t* list, const int32_t* count_in, int32_t* rays_out,
                                                                    int32_t* count_out, const int32_t* frame_count,
                                                                    unsigned long long* mismatch, int64_t n, int64_t capacity, int l,
                                                                    int layer, int ns) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t stride = (int64_t)gridDim.x * 4;
    const int64_t c = *count_in;
    const bool fits = c >= 0 && c <= capacity && (!TO_DENSE || c <= n);   // (a frame's list never holds more than n rays)
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (TO_DENSE) {
            if (count_out != count_in) *count_out = fits ? (int32_t)c : -1;
        } else if (mismatch && frame_count && (int64_t)*frame_count != c) {
            atomicAdd(mismatch, 1ull);
        }
    }
    if (!fits) return;
    // (the four slots are named, not an array: a private array here is moved to the LDS by the compiler)
    struct Slot {
        int64_t at, slot;   // float4 index of the slot's first sample in raw / in dense
        bool ok;
    };
    auto locate = [&](int64_t j) -> Slot {
        const int32_t ray = j < c ? __builtin_amdgcn_readfirstlane(list[j]) : -1;
        const bool ok = ray >= 0 && ray < n;
        if (TO_DENSE && ok && lane == 0 && rays_out != list) rays_out[j] = ray;
        return Slot{((int64_t)ray * l + layer) * ns, j * ns, ok};
    };
    auto load = [&](const Slot& s, int k) -> float4 { return s.ok ? (TO_DENSE ? raw[s.at + k] : dense[s.slot + k]) : float4{0.f, 0.f, 0.f, 0.f}; };
    auto store = [&](const Slot& s, int k, const float4& v) {
        if (s.ok) (TO_DENSE ? dense[s.slot + k] : raw[s.at + k]) = v;
    };
    for (int64_t j0 = wave; j0 < c; j0 += SLOTS_IN_FLIGHT * stride) {
        const Slot s0 = locate(j0), s1 = locate(j0 + stride), s2 = locate(j0 + 2 * stride), s3 = locate(j0 + 3 * stride);
        for (int k = lane; k < ns; k += 64) {
            const float4 v0 = load(s0, k), v1 = load(s1, k), v2 = load(s2, k), v3 = load(s3, k);
            store(s0, k, v0);
            store(s1, k, v1);
            store(s2, k, v2);
            store(s3, k, v3);
        }
    }
}

}  // namespace

extern "C" int stnerf_copy_layer_raw_listed(float* raw, int64_t n, int l, int layer, int ns, const int32_t* ray_list,
                                            const int32_t* ray_count, float* dense, int32_t* rays, int32_t* count, int64_t capacity,
                                            int to_dense, int64_t* mismatch, stnerf_stream_t stream) {
    STNERF_REQUIRE(raw && dense && rays && count, "copy_layer_raw_listed: null pointer");
    STNERF_REQUIRE(!to_dense || (ray_list && ray_count), "copy_layer_raw_listed: a capture needs the frame's ray list and count");
    STNERF_REQUIRE(n >= 0 && l >= 2 && l <= STNERF_MAX_LAYERS && ns >= 1, "copy_layer_raw_listed: bad shape");
    STNERF_REQUIRE(layer >= 1 && layer < l, "copy_layer_raw_listed: layer %d is not a performer of %d layers (the background has a dense cache)",
                   layer, l);
    STNERF_REQUIRE(capacity >= 0, "copy_layer_raw_listed: negative capacity");
    STNERF_REQUIRE((((uintptr_t)raw | (uintptr_t)dense) & 15) == 0, "copy_layer_raw_listed: raw and dense must be 16-byte aligned");
    STNERF_REQUIRE(((uintptr_t)mismatch & 7) == 0, "copy_layer_raw_listed: the mismatch counter must be 8-byte aligned");
    // memory-bound: a wave per slot, at most 2048 workgroups, the rest by the stride loop.  One workgroup at least: a capture
    // always reports its count.
    const int64_t bound = to_dense && n < capacity ? n : capacity;
    const int64_t blocks = (bound + 3) / 4;
    const dim3 grid((unsigned)(blocks < 1 ? 1 : (blocks < 2048 ? blocks : 2048)));
    hipStream_t st = as_stream(stream);
    LaunchTimer timer(PROF_COPY_LAYER_RAW_LISTED, to_dense ? 1 : 0, bound, ns, 32 * (int64_t)ns + 4, st);
    if (to_dense)
        hipLaunchKernelGGL(copy_layer_raw_listed_kernel<true>, grid, dim3(256), 0, st, reinterpret_cast<float4*>(raw),
                           reinterpret_cast<float4*>(dense), ray_list, ray_count, rays, count, (const int32_t*)nullptr,
                           (unsigned long long*)nullptr, n, capacity, l, layer, ns);
    else
        hipLaunchKernelGGL(copy_layer_raw_listed_kernel<false>, grid, dim3(256), 0, st, reinterpret_cast<float4*>(raw),
                           reinterpret_cast<float4*>(dense), (const int32_t*)rays, (const int32_t*)count, (int32_t*)nullptr,
                           (int32_t*)nullptr, ray_count, reinterpret_cast<unsigned long long*>(mismatch), n, capacity, l, layer, ns);
    STNERF_CHECK_LAUNCH("copy_layer_raw_listed");
    return STNERF_OK;
}
