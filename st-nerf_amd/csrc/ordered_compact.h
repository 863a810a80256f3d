// Ordered, deterministic compaction in three launches, stated once: the ascending list of the q in [0, P) for which a predicate
// holds, and its length in one device int32.  Launch 1 takes the popcount of every 256 entries with a ballot, launch 2 scans the
// popcounts in ONE workgroup (1024 per pass, with a running carry), launch 3 evaluates the predicate again and writes.  No
// workgroup waits on another.  Used by stnerf_accumulate_select (csrc/accumulate.hip) and stnerf_reproject_holes
// (csrc/reproject.hip); Pred is a small struct passed by value with  __device__ bool operator()(int64_t q) const.
#pragma once
#include "common.h"

namespace stnerf {

constexpr int kSelectBlock = 256;   // entries per workgroup of launches 1 and 3
constexpr int kScanBlock = 1024;    // workgroup popcounts per pass of launch 2

#if defined(__HIPCC__)
// Launch 1: block_count[b] = entries of [256 b, 256 b + 256) that pass.
template <class Pred>
__global__ void __launch_bounds__(kSelectBlock) select_count_kernel(Pred pred, int64_t P, int32_t* __restrict__ block_count) {
    __shared__ int wave_total[kSelectBlock / 64];
    const int64_t q = (int64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    const bool act = q < P && pred(q);
    const unsigned long long ball = __ballot(act);
    if ((threadIdx.x & 63) == 0) wave_total[threadIdx.x >> 6] = __popcll(ball);
    __syncthreads();
    if (threadIdx.x == 0) {
        int tot = 0;
        for (int i = 0; i < kSelectBlock / 64; ++i) tot += wave_total[i];
        block_count[blockIdx.x] = tot;
    }
}

// Launch 2: ONE workgroup turns the nb popcounts into exclusive offsets, in place, 1024 per pass with a running carry, and
// writes the total.  It waits on no other workgroup: there is none.  (A template only so that two files may hold it.)
template <int kBlock>
__global__ void __launch_bounds__(kBlock) select_scan_kernel(int32_t* __restrict__ block_count, int64_t nb, int32_t* __restrict__ total) {
    __shared__ int wave_sum[kBlock / 64];
    __shared__ int carry_s;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) carry_s = 0;
    __syncthreads();
    for (int64_t base = 0; base < nb; base += kBlock) {
        const int64_t b = base + threadIdx.x;
        const int v = b < nb ? block_count[b] : 0;
        int inc = v;  // inclusive scan of the wave
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int up = __shfl_up(inc, d, 64);
            if (lane >= d) inc += up;
        }
        if (lane == 63) wave_sum[wave] = inc;
        __syncthreads();
        int before = carry_s;
        for (int i = 0; i < wave; ++i) before += wave_sum[i];
        if (b < nb) block_count[b] = before + inc - v;
        __syncthreads();
        if (threadIdx.x == kBlock - 1) carry_s = before + inc;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry_s;
}

// Launch 3: the predicate again, the entry's place = its workgroup's offset + the waves before it + the lanes before it.
template <class Pred>
__global__ void __launch_bounds__(kSelectBlock) select_write_kernel(Pred pred, int64_t P, const int32_t* __restrict__ block_offset,
                                                                    int32_t* __restrict__ out) {
    __shared__ int wave_total[kSelectBlock / 64];
    const int64_t q = (int64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    const bool act = q < P && pred(q);
    const unsigned long long ball = __ballot(act);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) wave_total[wave] = __popcll(ball);
    __syncthreads();
    if (!act) return;
    int at = block_offset[blockIdx.x];
    for (int i = 0; i < wave; ++i) at += wave_total[i];
    at += __popcll(ball & ((1ull << lane) - 1ull));
    out[at] = (int32_t)q;     // at < the total <= P: as many places as entries that pass
}

// The three launches.  blocks: select_blocks(P) int32 of device memory, overwritten.
template <class Pred>
static inline int ordered_compact(const Pred& pred, int64_t P, int32_t* blocks, int32_t* out, int32_t* n_out, hipStream_t stream,
                                  const char* what_count, const char* what_scan, const char* what_write) {
    const int64_t nb = (P + kSelectBlock - 1) / kSelectBlock;
    hipLaunchKernelGGL(select_count_kernel<Pred>, dim3((unsigned)nb), dim3(kSelectBlock), 0, stream, pred, P, blocks);
    STNERF_CHECK_LAUNCH(what_count);
    hipLaunchKernelGGL(select_scan_kernel<kScanBlock>, dim3(1), dim3(kScanBlock), 0, stream, blocks, nb, n_out);
    STNERF_CHECK_LAUNCH(what_scan);
    hipLaunchKernelGGL(select_write_kernel<Pred>, dim3((unsigned)nb), dim3(kSelectBlock), 0, stream, pred, P, (const int32_t*)blocks, out);
    STNERF_CHECK_LAUNCH(what_write);
    return STNERF_OK;
}
#endif

static inline int64_t select_blocks(int64_t P) { return (P + kSelectBlock - 1) / kSelectBlock; }
static inline int64_t select_workspace_bytes(int64_t P) { return (select_blocks(P) * (int64_t)sizeof(int32_t) + 255) / 256 * 256; }

}  // namespace stnerf
