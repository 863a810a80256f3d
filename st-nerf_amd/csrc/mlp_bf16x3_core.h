// The split-bf16 ("bf16x3") machinery: fp32-faithful matrix products on the bf16 MFMA pipe.  Shared by the kernels of mlp_bf16x3.hip
// (the persistent stage kernel, the MotionNet kernel) and train_bf16x3.hip (the backward chain).
//
// gfx950 has no tf32/xf32 MFMA and its f32 MFMA runs at the f32 vector rate (157 TF/s), 1/16 of the bf16 rate.  Here every
// fp32 operand is split into THREE bf16 pieces, x = x0 + x1 + x2 (8 + 8 + 8 significand bits: the split is exact and keeps
// fp32's exponent range -- no scaling, no range limit), and a product a*b is evaluated with its six leading cross terms
//     a0 b0 + (a0 b1 + a1 b0) + (a1 b1 + a0 b2 + a2 b0)            (dropped: a1 b2, a2 b1, a2 b2 <= 2^-24 |a b|)
// on v_mfma_f32_32x32x16_bf16 (bf16 products are exact in fp32; f32 accumulate).  The a0 b0 terms go to one accumulator,
// the five small terms (<= 2^-8 of it) to a second one: the hardware rounds the running sum after every 8 products, and
// with one accumulator the 96 MFMAs of a 256-deep layer put 192 roundings at the scale of the full sum -- measured
// 1.09 x the error of an fp32 fma chain (tools/micro/bf16x3_proto.hip); split, the large accumulator sees 32 of them and
// the small one's are 2^-8 smaller: ~0.45 x the fp32 chain's error.
//
// Organisation = csrc/mlp_wave.hip's: a wave owns 32 samples and all features, the accumulator layout of a layer is the
// B-operand layout of the next one (K step t of 16 = registers 8 (t & 1) .. + 7 of block t >> 1, both lane halves), so the
// activations never leave the register file: a layer boundary is { big + small, ReLU, split into three bf16 planes }.
// What differs:
//   * 256-wide layers run as two PASSES of 128 output features (4 blocks x {big, small} = 128 accumulator registers);
//     a pass's outputs are parked in AGPRs (ReLU'd fp32) and split into the bf16 planes under the MFMAs of the NEXT pass:
//     the first pass's under the second half of the second pass, the second pass's under the first half of the next
//     layer's first pass (UnparkHook).
//   * Weights: 6 B per value and 2.7 x the f32 kernel's MFMA rate -- four waves streaming the blob through the vector L1
//     would need ~60 B/clk/CU (measured ceiling 53).  They are fetched ONCE per CU by LDS-DMA (global_load_lds_dwordx4,
//     no registers involved) into a ring of four 24 KB slots in consumption order and read by every wave with
//     ds_read_b128 straight into AGPRs (1 KB contiguous per instruction: conflict-free), one read behind each of the
//     first MFMAs of a unit; one raw s_barrier per slot (= 48 MFMAs) orders "slot landed" and "slot free" at once.
//   * Bias vectors and head weights: one copy per workgroup in LDS (LDS-DMA at the start of a work item).
//   * PE, bias, ReLU, heads, outputs: fp32, as in the exact-f32 kernels; rgb_net.1's direction / time columns come per
//     ray from mlp_raybias.hip (exact f32), added behind the layer's K loop.
//
// Four kernels are built from this machinery.  mlp_bf16x3.hip: the stage kernel of the render path (mlp_bf16x3_stage_kernel<DEEP,
// NoTapArgs>); the same kernel with the training tap (<false, StoreTapArgs>: every layer's post-ReLU output and its mask bits written
// out as the rows pass -- stnerf_train_spacenet_fwd_bf16x3); the stage kernel's MotionNet alone over rows of its own
// (mlp_bf16x3_motion_kernel: the render pipeline's MotionNet reuse, pipeline.hip).  train_bf16x3.hip: the backward chain
// d x = (d y AND mask) W over the TRANSPOSED weights as a second bf16x3 stream (train_space_dx_bx_kernel --
// stnerf_train_spacenet_dx_bf16x3).  The blobs they stream: mlp_bf16x3.h (layout), pack_bf16x3.hip (packers, host and device).
//
// Reference: modeling/spacenet.py:16-160, modeling/motion_net.py:7-71, modeling/layered_rfrender.py:340-418,495-576; training:
// engine/layered_trainer.py:281 (loss.backward() through modeling/spacenet.py:101-160).
#pragma once
#include <type_traits>

#include "mlp_wave_common.h"
#include "mlp_bf16x3.h"

namespace stnerf {

using bf16x8 = __attribute__((ext_vector_type(8))) __bf16;
using bf16x2 = __attribute__((ext_vector_type(2))) __bf16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

constexpr int BX_LDS_RING = BX_RING * BX_SLOT;
constexpr int BX_LDS_ENC = WV_NW * WV_ENC_FLOATS * 4;
constexpr int BX_LDS_CONST = (BX_CONST_SPACE + BX_CONST_MOTION) * 4;
constexpr int BX_LDS = BX_LDS_RING + BX_LDS_ENC + BX_LDS_CONST + 16 + STNERF_MAX_LAYERS * 8 + (STNERF_MAX_LAYERS + 1) * 4 + 12;
static_assert(BX_LDS <= 160 * 1024, "bf16x3 stage kernel: LDS budget");

#define BX_SB() __builtin_amdgcn_sched_barrier(0)

// Optional per-phase cycle accounting (development builds: -DSTNERF_BX_PROF, tools/bx_prof.py): every wave adds its clock
// deltas per phase into g_bxphase (mlp_bf16x3.hip); read back with stnerf_debug_bx_phases().  Only the kernels of mlp_bf16x3.hip
// call the instrumented functions (motion_bx, space_bx) and flush their BxProf into g_bxphase; a kernel of another file that
// called them under the flag would have to do the same.
#ifdef STNERF_BX_PROF
struct BxProf {
    unsigned long long t, acc[16];
};
#define BXP_PARAM , BxProf& bp
#define BXP_ARG , bp
#define BXP(i) do { const unsigned long long n_ = clock64(); bp.acc[i] += n_ - bp.t; bp.t = n_; } while (0)
#else
#define BXP_PARAM
#define BXP_ARG
#define BXP(i) do { } while (0)
#endif
enum { BXP_TOP = 0, BXP_MOTION_ENC = 1, BXP_MOTION_PASS = 2, BXP_MOTION_FIN = 3, BXP_PE = 4, BXP_PASS = 5, BXP_PARK = 6, BXP_ACT = 7,
       BXP_LOADC = 8, BXP_SIGMA = 9, BXP_RGB_TAIL = 10, BXP_END = 11, BXP_ITEMS = 12 };
// s_waitcnt vmcnt(n) only (gfx9 encoding: vmcnt = [3:0] + [15:14], expcnt [6:4], lgkmcnt [11:8])
#define BX_VMCNT(n) __builtin_amdgcn_s_waitcnt(((n) & 0xf) | (((n) >> 4) << 14) | 0x0f70)

// ---------------------------------------------------------------------------------------------
// fp32 -> three bf16 pieces (round to nearest even at every step: x = p0 + p1 + p2 exactly)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned pk_bf16(float a, float b) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    f32x2_ v = {a, b};
    bf16x2 h = __builtin_convertvector(v, bf16x2);  // v_cvt_pk_bf16_f32
    return *reinterpret_cast<unsigned*>(&h);
}
__device__ __forceinline__ void split8(const float (&v)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
    // (scalar source on purpose: the compiler pairs the subtractions into v_pk_add_f32 by itself; written on explicit
    // 2-vectors the value array is not promoted to registers and the split goes through scratch memory)
    u32x4 w0, w1, w2;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float x0 = v[2 * i], x1 = v[2 * i + 1];
        const unsigned u = pk_bf16(x0, x1);
        const float r0 = x0 - __uint_as_float(u << 16), r1 = x1 - __uint_as_float(u & 0xffff0000u);
        const unsigned m = pk_bf16(r0, r1);
        const float s0 = r0 - __uint_as_float(m << 16), s1 = r1 - __uint_as_float(m & 0xffff0000u);
        w0[i] = u;
        w1[i] = m;
        w2[i] = pk_bf16(s0, s1);
    }
    p0 = *reinterpret_cast<bf16x8*>(&w0);
    p1 = *reinterpret_cast<bf16x8*>(&w1);
    p2 = *reinterpret_cast<bf16x8*>(&w2);
}

// ---------------------------------------------------------------------------------------------
// Training tap (the split-bf16 twin of mlp_wave.hip's StoreTap): every layer's post-ReLU output goes to the row-major
// matrices of StoreTapArgs on its way into the park, the ReLU masks as bit planes beside them.  Plain global stores from a
// per-lane pointer (two registers, built where they are used): with BUFFER stores -- descriptor on the scalar ALU, rows past the
// end of the launch dropped by the range check, one offset register -- the four aligned scalar registers of a descriptor do not
// exist at a boundary of this kernel, and the allocator answers with ~170 spilled vector registers (round 6; a global store with
// the same data: none).  Stores count in vmcnt like the weight ring's LDS-DMA: the slot turns behind a boundary that stored wait
// for `6 + stores` (slot_turn<ST>), or they would wait for the stores too.
// ---------------------------------------------------------------------------------------------
struct BxNoTap {
    static constexpr bool on = false;
};
struct BxStoreTap {
    static constexpr bool on = true;
    const StoreTapArgs* a;   // the kernel's argument block (scalar loads)
    uint32_t row0;           // first row of the work item
    uint32_t nrows;          // rows of the launch in this item (1 .. WV_ITEM)
    int wave;
};
constexpr int BX_TAP_PARK = 18;   // VMEM stores of one park: 16 x 16 B of activations + two mask words
constexpr int BX_TAP_PE = 8;
__device__ __forceinline__ uint32_t tap_row_in_item(const BxStoreTap& tap, int lane) { return (uint32_t)(tap.wave * WV_ROWS + (lane & 31)); }
__device__ __forceinline__ bool tap_valid(const BxStoreTap& tap, int lane) {
#ifdef STNERF_DEV_TAP_ALWAYS_VALID      // (development A/B: what the per-store validity branches cost; launches of whole items only)
    return true;
#else
    return tap_row_in_item(tap, lane) < tap.nrows;
#endif
}
// this lane's 16 bytes of (stage, column col0) of its row; stage: 0 .. 7 or TAP_PE
__device__ __forceinline__ float* tap_row(const BxStoreTap& tap, int stage, int col0, int lane) {
    // (opaque here: the per-lane addresses of all fifteen boundaries are loop invariants of the item loop -- hoisted, they are live
    // through every K loop of a kernel that has no register to spare)
    asm volatile("" : "+v"(lane));
    const bool is_pe = stage == TAP_PE;
    float* base = is_pe ? tap.a->pe : tap.a->buf[is_pe ? 0 : stage];
    const uint32_t ld = (uint32_t)(is_pe ? tap.a->ld_pe : tap.a->ld[is_pe ? 0 : stage]);
    return base + (size_t)(tap.row0 + tap_row_in_item(tap, lane)) * ld + (uint32_t)(col0 + 4 * (lane >> 5));
}
// word (col0 / 128) * 2 of this lane's four mask words of its row (null: the caller wants no masks)
__device__ __forceinline__ uint32_t* tap_bits_row(const BxStoreTap& tap, int stage, int col0, int lane) {
    asm volatile("" : "+v"(lane));
    uint32_t* bw = tap.a->bits;
    if (!bw) return nullptr;
    return bw + (size_t)stage * (size_t)tap.a->bits_stride + (size_t)(tap.row0 + tap_row_in_item(tap, lane)) * 8u +
           (uint32_t)(4 * (lane >> 5) + (col0 ? 2 : 0));
}
// value i of block fb <-> bit (16 fb + i) & 31 of word fb >> 1 (mlp_wave.hip: StoreTap); a post-ReLU value is +0 or positive
__device__ __forceinline__ void tap_bit(uint32_t& w, float v, int pos /* a constant once the loops are unrolled */) {
    uint32_t t;
    asm volatile("v_min_u32 %1, 1, %2\n\tv_lshl_or_b32 %0, %1, %3, %0" : "+v"(w), "=&v"(t) : "v"(v), "i"(pos));
}

// ---------------------------------------------------------------------------------------------
// The weight stream: which global slot the workgroup fetches next (wave-uniform), the ring, the A-operand buffers.
// ---------------------------------------------------------------------------------------------
struct Seg {
    const char* p;
    uint32_t left;  // slots
};
struct ABuf {
    bf16x8 p[3];  // the three pieces of one unit's A operand (AGPRs)
};
struct Ctx {
    Seg seg[4];         // this work item's networks (deformation net, SpaceNet), then the next item's
    const char* idle;   // a valid source when nothing is left to fetch
    uint32_t gi;        // slots issued so far
    uint32_t rcur, rnext;  // this lane's LDS byte address inside the slot being consumed / the next one
    uint32_t gc;        // slots consumed so far
    char* ring;
    int wave, lane;
    bool st_on;         // training kernels: this wave issues the boundary stores its slot turns count in (slot_turn<ST>)
    ABuf A[4];
};

__device__ __forceinline__ const char* feed_next(Ctx& cx) {
    const char* p = cx.idle;
    bool done = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const bool take = !done && cx.seg[i].left != 0;
        p = take ? cx.seg[i].p : p;
        cx.seg[i].p += take ? BX_SLOT : 0;
        cx.seg[i].left -= take ? 1u : 0u;
        done = done || take;
    }
    return p;
}

// This wave's quarter (6 x 1 KB) of the next slot of the stream on its way into ring slot gi & 3.  Issued in a clump, the
// six LDS-DMA instructions (each with its M0 write) hold the wave's issue port for ~240 cycles with one MFMA in flight to
// cover them (tools/micro/bf16x3_proto.hip: 5 of 42 cycles per MFMA); dma_begin() does the scalar part at the slot turn,
// dma_chunk<c>() goes out one behind each of the MFMAs of the slot's last two units that carry no operand read.
struct Dma {
    const char* src;                                  // this lane's source address of chunk 0
    __attribute__((address_space(3))) char* dst;      // (wave-uniform) LDS destination of chunk 0
};
__device__ __forceinline__ void dma_begin(Ctx& cx, Dma& d) {
    d.src = feed_next(cx) + cx.wave * (6 * BX_CHUNK) + cx.lane * 16;
    d.dst = (__attribute__((address_space(3))) char*)(cx.ring) + (cx.gi & (BX_RING - 1)) * BX_SLOT + cx.wave * (6 * BX_CHUNK);
    cx.gi += 1;
}
template <int C>
__device__ __forceinline__ void dma_chunk(const Dma& d) {
    __builtin_amdgcn_global_load_lds(d.src + C * BX_CHUNK, (__attribute__((address_space(3))) void*)(d.dst + C * BX_CHUNK), 16, 0, 0);
}
__device__ __forceinline__ void dma_issue(Ctx& cx) {   // (all six at once: priming)
    Dma d;
    dma_begin(cx, d);
    dma_chunk<0>(d);
    dma_chunk<1>(d);
    dma_chunk<2>(d);
    dma_chunk<3>(d);
    dma_chunk<4>(d);
    dma_chunk<5>(d);
}

// A operands: ds_read_b128 straight into AGPRs, as asm -- the compiler does not count these reads; a_wait() is their
// s_waitcnt and names every destination, so no consumer can be scheduled above it.  `keep` = reads of LATER units that may
// stay outstanding (LDS returns in order; anything else in flight only makes the wait more conservative).
template <int OFF>
__device__ __forceinline__ void a_read(bf16x8& dst, uint32_t addr) {
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=a"(dst) : "v"(addr), "i"(OFF) : "memory");
}
template <int KEEP>
__device__ __forceinline__ void a_wait(ABuf& A) {
    asm volatile("s_waitcnt lgkmcnt(%3)" : "+a"(A.p[0]), "+a"(A.p[1]), "+a"(A.p[2]) : "i"(KEEP));
}

__device__ __forceinline__ f32x16 mfma_bf16(const bf16x8& a, const bf16x8& b, const f32x16& c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}

// One unit = the six MFMAs of (K step, feature block): five into `small` (the first of a pass starts it from 0), a0 b0
// into `big`.  U = position in the slot (K step U >> 2, block U & 3); the reads of unit U + 2 go out one behind each of the
// first three MFMAs (four buffers; the one they fill was consumed by unit U - 2).  With the reads only one unit ahead --
// 160 cycles -- the K passes ran at 1.33 x their MFMA time (tools/bx_prof.py): the LDS round trip under four waves' load is
// longer than that.
// What may ride in the shadow of a unit's last three MFMAs (the ones without an operand read behind them): ~4 vector
// instructions each are free (tools/micro/bf16x3_proto.hip: 2 per MFMA cost 0.5 cycles of 32).
struct NoHook {
    template <int U, int I>
    __device__ __forceinline__ void at() {}
};
template <int U, bool FIRST, bool BIG0 = false, int DMA0 = -1, class Hook = NoHook>
__device__ __forceinline__ void unit(Ctx& cx, f32x16& big, f32x16& small, const bf16x8& b0, const bf16x8& b1, const bf16x8& b2,
                                     const Dma* dma = nullptr, Hook* hook = nullptr) {
    ABuf& cur = cx.A[U & 3];
    ABuf& nx = cx.A[(U + 2) & 3];
    constexpr int OFF = ((U + 2) & 7) * BX_UNIT;
    const uint32_t ra = (U + 2) < 8 ? cx.rcur : cx.rnext;
    a_wait<3>(cur);   // (the three reads of unit U + 1 may stay in flight)
    BX_SB();
    if (FIRST) {
        const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        small = mfma_bf16(cur.p[2], b0, z);
    } else {
        small = mfma_bf16(cur.p[2], b0, small);
    }
    BX_SB();
    a_read<OFF>(nx.p[0], ra);
    BX_SB();
    small = mfma_bf16(cur.p[0], b2, small);
    BX_SB();
    a_read<OFF + BX_CHUNK>(nx.p[1], ra);
    BX_SB();
    small = mfma_bf16(cur.p[1], b1, small);
    BX_SB();
    a_read<OFF + 2 * BX_CHUNK>(nx.p[2], ra);
    BX_SB();
    small = mfma_bf16(cur.p[1], b0, small);
    if (DMA0 >= 0) {
        BX_SB();
        dma_chunk<DMA0 < 0 ? 0 : DMA0>(*dma);
        BX_SB();
    }
    if constexpr (!std::is_same<Hook, NoHook>::value) {
        BX_SB();
        hook->template at<U, 0>();
        BX_SB();
    }
    small = mfma_bf16(cur.p[0], b1, small);
    if (DMA0 >= 0) {
        BX_SB();
        dma_chunk<DMA0 < 0 ? 0 : DMA0 + 1>(*dma);
        BX_SB();
    }
    if constexpr (!std::is_same<Hook, NoHook>::value) {
        BX_SB();
        hook->template at<U, 1>();
        BX_SB();
    }
    if (FIRST && BIG0) {  // (rgb_net.1: its C operand is added behind the K loop, see space_bx)
        const f32x16 z = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        big = mfma_bf16(cur.p[0], b0, z);
    } else {
        big = mfma_bf16(cur.p[0], b0, big);
    }
    if (DMA0 >= 0) {
        BX_SB();
        dma_chunk<DMA0 < 0 ? 0 : DMA0 + 2>(*dma);
    }
    if constexpr (!std::is_same<Hook, NoHook>::value) {
        BX_SB();
        hook->template at<U, 2>();
    }
    BX_SB();
}

// Between units 5 and 6 of a slot: the next slot has landed everywhere and the previous one is free everywhere (every wave
// has issued -- and, to get here, completed -- its reads of it); the fetch three slots ahead goes into its place.
// ST: VMEM stores this wave issued behind the DMA of the slot it is waiting for (the training kernels' boundary stores).  The
// immediate must never exceed 6 + the stores really in flight, or the wait no longer covers the wave's share of the LDS-DMA: a
// wave whose 32 rows are all past the end of the launch branches around its conditional stores (and a launch without mask planes
// skips two per boundary) -- such a wave runs with st_on == false and waits for vmcnt(6), which is always sufficient.
template <int ST = 0>
__device__ __forceinline__ void slot_turn(Ctx& cx, Dma& d) {
    if constexpr (ST > 0) {
        if (cx.st_on)      // (wave-uniform: a scalar branch)
            BX_VMCNT(6 + ST);
        else
            BX_VMCNT(6);
    } else {
        BX_VMCNT(6);
    }
    __builtin_amdgcn_s_barrier();
    dma_begin(cx, d);
    BX_SB();
}
__device__ __forceinline__ void slot_done(Ctx& cx) {
    cx.gc += 1;
    cx.rcur = cx.rnext;
    // the slot after it, wrapping at the end of the ring (from rnext itself: a third per-lane address kept through the item
    // only to be added to here was spilled, and its reload waits behind vmcnt(0) -- the DMA queue)
    cx.rnext = cx.rnext + (((cx.gc + 1) & (BX_RING - 1)) == 0 ? BX_SLOT - BX_RING * BX_SLOT : BX_SLOT);
}

// one ring slot: K steps k0, k1 (their B operands: the three planes of the input) for the pass's four blocks
template <bool FIRST, bool BIG0 = false, class Hook = NoHook, int ST = 0>
__device__ __forceinline__ void slot(Ctx& cx, f32x16 (&big)[4], f32x16 (&small)[4], const bf16x8& k0p0, const bf16x8& k0p1,
                                     const bf16x8& k0p2, const bf16x8& k1p0, const bf16x8& k1p1, const bf16x8& k1p2, Hook* hook = nullptr) {
    unit<0, FIRST, BIG0, -1, Hook>(cx, big[0], small[0], k0p0, k0p1, k0p2, nullptr, hook);
    unit<1, FIRST, BIG0, -1, Hook>(cx, big[1], small[1], k0p0, k0p1, k0p2, nullptr, hook);
    unit<2, FIRST, BIG0, -1, Hook>(cx, big[2], small[2], k0p0, k0p1, k0p2, nullptr, hook);
    unit<3, FIRST, BIG0, -1, Hook>(cx, big[3], small[3], k0p0, k0p1, k0p2, nullptr, hook);
    unit<4, false, false, -1, Hook>(cx, big[0], small[0], k1p0, k1p1, k1p2, nullptr, hook);
    unit<5, false, false, -1, Hook>(cx, big[1], small[1], k1p0, k1p1, k1p2, nullptr, hook);
    Dma d;
    slot_turn<ST>(cx, d);
    unit<6, false, false, 0, Hook>(cx, big[2], small[2], k1p0, k1p1, k1p2, &d, hook);
    unit<7, false, false, 3, Hook>(cx, big[3], small[3], k1p0, k1p1, k1p2, &d, hook);
    slot_done(cx);
}

// K steps KS0 .. KS0 + 2 NSLOT - 1 of the activation planes
// (ST: stores issued in the boundary in front of the pass -- they are younger than the DMA its first TWO slot turns wait for)
template <int KS0, int NSLOT, bool FIRST, bool BIG0 = false, int ST = 0>
__device__ __forceinline__ void pass_act(Ctx& cx, f32x16 (&big)[4], f32x16 (&small)[4], const bf16x8 (&act)[3][16]) {
#pragma unroll
    for (int sl = 0; sl < NSLOT; ++sl) {
        const int k = KS0 + 2 * sl;
        if (sl == 0)
            slot<FIRST, BIG0, NoHook, ST>(cx, big, small, act[0][k], act[1][k], act[2][k], act[0][k + 1], act[1][k + 1], act[2][k + 1]);
        else if (sl == 1)
            slot<false, false, NoHook, ST>(cx, big, small, act[0][k], act[1][k], act[2][k], act[0][k + 1], act[1][k + 1], act[2][k + 1]);
        else
            slot<false>(cx, big, small, act[0][k], act[1][k], act[2][k], act[0][k + 1], act[1][k + 1], act[2][k + 1]);
    }
}

// ---------------------------------------------------------------------------------------------
// Layer boundaries (vector ALU).  Register 4 q + r of block fb <-> feature 32 fb + 8 q + 4 h + r of the pass.
// ---------------------------------------------------------------------------------------------
// big = this lane's 64 values of a 128-float vector in LDS (the next pass's bias = the C operand of its a0 b0 chain)
__device__ __forceinline__ void load_c(f32x16 (&big)[4], const float* v128, int lane) {
    const float4* b4 = reinterpret_cast<const float4*>(v128) + (lane >> 5);
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 b = b4[fb * 8 + 2 * q];
            big[fb][4 * q + 0] = b.x;
            big[fb][4 * q + 1] = b.y;
            big[fb][4 * q + 2] = b.z;
            big[fb][4 * q + 3] = b.w;
            BX_SB();
        }
}
// block fb of load_c: issued as soon as the block's accumulators have been consumed by a boundary pass, so that the LDS
// round trip runs under the vector work of the following blocks (as relu_rebias of mlp_wave.hip)
__device__ __forceinline__ void load_c_block(f32x16& bigfb, const float* v128, int fb, int lane) {
    const float4* b4 = reinterpret_cast<const float4*>(v128) + (lane >> 5);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 b = b4[fb * 8 + 2 * q];
        bigfb[4 * q + 0] = b.x;
        bigfb[4 * q + 1] = b.y;
        bigfb[4 * q + 2] = b.z;
        bigfb[4 * q + 3] = b.w;
    }
}
__device__ __forceinline__ float out_relu(const f32x16& big, const f32x16& small, int i) { return relu_bits(big[i] + small[i]); }

// the first pass's outputs wait in AGPRs while the second pass still reads the layer's input
struct Park {
    float v[64];
};
__device__ __forceinline__ void park_put(float& dst, float v) { asm("v_accvgpr_write_b32 %0, %1" : "=a"(dst) : "v"(v)); }
__device__ __forceinline__ float park_get(const float& src) {
    float v;
    asm("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(src));
    return v;
}

// The heads (density_net.0: 256 -> 1; the 128 -> 3 colour / flow layers) accumulate in FP64 on the vector ALU: 128 + 192
// v_fma_f64 per lane and work item are nothing next to 4.3 k MFMAs, and they take the heads out of the error budget -- with
// the split accumulators the backbone's h is ~2.3 x closer to fp64 than an fp32 fma chain's, and a 256-term fp32 dot
// product on top of it (however it is grouped) was most of the error left in sigma.
__device__ __forceinline__ double pair_sum_d(double x) {  // x + the other lane's (lane ^ 32) x, in every lane
    return x + __shfl_xor(x, 32, 64);
}
struct SigAcc {
    double c[4];
};
__device__ __forceinline__ void sig_take(SigAcc& sg, const float (&v)[8], const float* w, int lane, int feat0 /* of v[0], h = 0 */) {
    const float4* w4 = reinterpret_cast<const float4*>(w + feat0) + (lane >> 5);
    const float4 wa = w4[0], wb = w4[2];
    sg.c[0] = fma((double)v[0], (double)wa.x, sg.c[0]);
    sg.c[1] = fma((double)v[1], (double)wa.y, sg.c[1]);
    sg.c[2] = fma((double)v[2], (double)wa.z, sg.c[2]);
    sg.c[3] = fma((double)v[3], (double)wa.w, sg.c[3]);
    sg.c[0] = fma((double)v[4], (double)wb.x, sg.c[0]);
    sg.c[1] = fma((double)v[5], (double)wb.y, sg.c[1]);
    sg.c[2] = fma((double)v[6], (double)wb.z, sg.c[2]);
    sg.c[3] = fma((double)v[7], (double)wb.w, sg.c[3]);
}

// pass A of a 256-wide layer: relu(big + small) -> park
// next_c: the 128 C-operand values (bias) of the pass that follows
__device__ __forceinline__ void finish_park(f32x16 (&big)[4], const f32x16 (&small)[4], Park& pk, const float* next_c, int lane) {
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
#pragma unroll
            for (int j = 0; j < 8; ++j) park_put(pk.v[16 * fb + 8 * t + j], out_relu(big[fb], small[fb], 8 * t + j));
            BX_SB();  // (group by group: keeps the live values of this straight-line code bounded)
        }
        if (next_c) {  // (uniform; nullptr where the next pass starts from 0: rgb_net.1)
            load_c_block(big[fb], next_c, fb, lane);
            BX_SB();
        }
    }
}
// the same with the training tap: the pass's 128 outputs = columns col0 .. col0 + 127 of stage `stage`'s matrix
__device__ __forceinline__ void finish_park(f32x16 (&big)[4], const f32x16 (&small)[4], Park& pk, const float* next_c, int lane, const BxNoTap&,
                                            int, int) {
    finish_park(big, small, pk, next_c, lane);
}
// (Register budget: the kernel's 256 arch registers are full -- 192 of activation planes -- and the park itself runs on two
// temporaries.  Here: four values at a time (the data of one 16-byte store), one mask word, the row pointer; the kernel's tap
// variant makes room for them by recomputing per-row values it would otherwise carry through the item, see
// mlp_bf16x3_stage_kernel.)
template <bool PARK = true>
__device__ __forceinline__ void finish_park(f32x16 (&big)[4], const f32x16 (&small)[4], Park& pk, const float* next_c, int lane,
                                            const BxStoreTap& tap, int stage, int col0) {
    const bool valid = tap_valid(tap, lane);
    float4* dst = reinterpret_cast<float4*>(tap_row(tap, stage, col0, lane));
    uint32_t w = 0u;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                v[r] = out_relu(big[fb], small[fb], 4 * q + r);
                if (PARK) park_put(pk.v[16 * fb + 4 * q + r], v[r]);
#ifndef STNERF_DEV_TAP_NO_BITS      // (development A/B of what the tap costs: profiles/retired_designs.md)
                tap_bit(w, v[r], (16 * fb + 4 * q + r) & 31);
#endif
            }
            // register 4 q + r of block fb <-> feature 32 fb + 8 q + 4 h + r: 16 bytes per (fb, q), the two lanes of a sample side by side
#ifndef STNERF_DEV_TAP_NO_STORES
            if (valid) dst[fb * 8 + 2 * q] = make_float4(v[0], v[1], v[2], v[3]);
#endif
            if (q & 1) BX_SB();
        }
        if (fb & 1) {
            uint32_t* bw = tap_bits_row(tap, stage, col0, lane);
            if (valid && bw) bw[fb >> 1] = w;
            if (stage == 7 && fb == 3 && valid && bw) {   // a 128-wide stage (rgb_net.1's output) owns all four words of the lane
                bw[2] = 0u;
                bw[3] = 0u;
            }
            w = 0u;
            BX_SB();
        }
        if (next_c) {
            load_c_block(big[fb], next_c, fb, lane);
            BX_SB();
        }
    }
}
// the pass's outputs -> K steps KS0 .. KS0 + 7 of the activation planes
template <int KS0>
__device__ __forceinline__ void finish_act(f32x16 (&big)[4], const f32x16 (&small)[4], bf16x8 (&act)[3][16], const float* next_c, int lane) {
#pragma unroll
    for (int fb = 0; fb < 4; ++fb) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = out_relu(big[fb], small[fb], 8 * t + j);
            split8(v, act[0][KS0 + 2 * fb + t], act[1][KS0 + 2 * fb + t], act[2][KS0 + 2 * fb + t]);
            BX_SB();
        }
        if (next_c) {  // (uniform; nullptr where the next pass starts from 0: rgb_net.1)
            load_c_block(big[fb], next_c, fb, lane);
            BX_SB();
        }
    }
}
// sigma head (density_net.0, 256 -> 1) on the last backbone layer's outputs, before they are converted: features 0..127 wait
// in the park, 128..255 in the accumulators.  (A pass of its own over the values -- 2 x 128 reads once per work item --
// rather than a flavour of finish_act: the layer loop's body must define the activation planes on ONE path; with two
// the planes' 192 registers meet in phi nodes the register coalescer cannot resolve, and half of them get copied.)
__device__ __forceinline__ float sigma_head(const f32x16 (&big)[4], const f32x16 (&small)[4], const Park& pk, const float* wsig, float bias,
                                            int lane) {
    SigAcc sg;
#pragma unroll
    for (int i = 0; i < 4; ++i) sg.c[i] = 0.0;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = park_get(pk.v[16 * fb + 8 * t + j]);
            sig_take(sg, v, wsig, lane, 32 * fb + 16 * t);
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = out_relu(big[fb], small[fb], 8 * t + j);
            sig_take(sg, v, wsig, lane, 128 + 32 * fb + 16 * t);
            BX_SB();
        }
    return (float)((double)bias + pair_sum_d((sg.c[0] + sg.c[1]) + (sg.c[2] + sg.c[3])));
}
template <int KS0 = 0>
__device__ __forceinline__ void unpark_act(const Park& pk, bf16x8 (&act)[3][16]) {
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = park_get(pk.v[16 * fb + 8 * t + j]);
            split8(v, act[0][KS0 + 2 * fb + t], act[1][KS0 + 2 * fb + t], act[2][KS0 + 2 * fb + t]);
            BX_SB();
        }
}

// The same conversion as unpark_act's, for ONE block, spread over the MFMA shadows of one ring slot (a pair of values per
// unit, in three steps).  BOTH passes of a 256-wide layer carry one:
//   * KS_OUT = 0, inside the SECOND pass, slots 4 .. 7: K steps 0 .. 7 of the input planes are dead by then and take the first
//     pass's outputs (round 3);
//   * KS_OUT = 8, inside the FIRST pass of the NEXT layer, slots 0 .. 3 (round 4): the previous layer's second pass parks its
//     outputs as well (finish_park, 320 cycles) instead of converting them in the open (finish_act, 1350), and the conversion
//     into K steps 8 .. 15 -- which the pass reads from slot 4 on -- rides under the MFMAs of K steps 0 .. 7.
// 832 of a layer's 1344 boundary instructions under MFMAs; what stays in the open are the two parks (ReLU + v_accvgpr_write).
template <int FB, int KS_OUT>
struct UnparkHook {
    const Park& pk;
    bf16x8 (&act)[3][16];
    float x0, x1, r0, r1;
    unsigned w0, w1;
    template <int U, int I>
    __device__ __forceinline__ void at() {
        constexpr int T = KS_OUT + 2 * FB + (U >> 2), W = U & 3;
        if (I == 0) {
            x0 = park_get(pk.v[16 * FB + 2 * U]);
            x1 = park_get(pk.v[16 * FB + 2 * U + 1]);
            w0 = pk_bf16(x0, x1);
        } else if (I == 1) {
            r0 = x0 - __uint_as_float(w0 << 16);
            r1 = x1 - __uint_as_float(w0 & 0xffff0000u);
            w1 = pk_bf16(r0, r1);
        } else {
            const float s0 = r0 - __uint_as_float(w1 << 16), s1 = r1 - __uint_as_float(w1 & 0xffff0000u);
            reinterpret_cast<u32x4&>(act[0][T])[W] = w0;
            reinterpret_cast<u32x4&>(act[1][T])[W] = w1;
            reinterpret_cast<u32x4&>(act[2][T])[W] = pk_bf16(s0, s1);
        }
    }
};
// one slot of a pass (K steps 2 FB, 2 FB + 1 of the half the pass is reading: the upper one for KS_OUT = 0, the lower one for
// KS_OUT = 8) with block FB of the park converted into the OTHER half of the planes on the way
template <int FB, int KS_OUT, bool FIRST = false, bool BIG0 = false, int ST = 0>
__device__ __forceinline__ void slot_unpark(Ctx& cx, f32x16 (&big)[4], f32x16 (&small)[4], bf16x8 (&act)[3][16], const Park& pk) {
    constexpr int k = (8 - KS_OUT) + 2 * FB;
    UnparkHook<FB, KS_OUT> hook{pk, act, 0.f, 0.f, 0.f, 0.f, 0u, 0u};
    slot<FIRST, BIG0, UnparkHook<FB, KS_OUT>, ST>(cx, big, small, act[0][k], act[1][k], act[2][k], act[0][k + 1], act[1][k + 1], act[2][k + 1], &hook);
}
// second pass of a 256-wide layer: 16 K steps, the parked first pass converted on the way
template <int ST = 0, bool BIG0 = false>
__device__ __forceinline__ void pass_b_unpark(Ctx& cx, f32x16 (&big)[4], f32x16 (&small)[4], bf16x8 (&act)[3][16], const Park& pk) {
    pass_act<0, 4, true, BIG0, ST>(cx, big, small, act);
    slot_unpark<0, 0>(cx, big, small, act, pk);
    slot_unpark<1, 0>(cx, big, small, act, pk);
    slot_unpark<2, 0>(cx, big, small, act, pk);
    slot_unpark<3, 0>(cx, big, small, act, pk);
}
// K steps 0 .. 7 of a pass whose input's upper half (features 128 .. 255 = the previous layer's second pass) still waits in
// the park: converted into K steps 8 .. 15 on the way.  The caller continues with pass_act<8, ..., false>.
template <bool BIG0 = false, int ST = 0>
__device__ __forceinline__ void pass_a_unpark(Ctx& cx, f32x16 (&big)[4], f32x16 (&small)[4], bf16x8 (&act)[3][16], const Park& pk) {
    slot_unpark<0, 8, true, BIG0, ST>(cx, big, small, act, pk);
    slot_unpark<1, 8, false, false, ST>(cx, big, small, act, pk);
    slot_unpark<2, 8>(cx, big, small, act, pk);
    slot_unpark<3, 8>(cx, big, small, act, pk);
}

// 128 -> 3 head (rgb_net's last layer, MotionNet's flow) on relu(big + small): w = [3][128] in LDS; fp64 accumulation, two
// chains per output and lane
__device__ __forceinline__ void head3(const f32x16 (&big)[4], const f32x16 (&small)[4], const float* w, const float* __restrict__ b3,
                                      int lane, float (&out)[3]) {
    const float4* w4 = reinterpret_cast<const float4*>(w) + (lane >> 5);
    double c[3][2];
#pragma unroll
    for (int o = 0; o < 3; ++o) c[o][0] = c[o][1] = 0.0;
#pragma unroll
    for (int fb = 0; fb < 4; ++fb)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            double v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) v[r] = (double)out_relu(big[fb], small[fb], 4 * q + r);
#pragma unroll
            for (int o = 0; o < 3; ++o) {
                const float4 wv = w4[o * 32 + fb * 8 + 2 * q];
                double& cc = c[o][q & 1];
                cc = fma(v[0], (double)wv.x, cc);
                cc = fma(v[1], (double)wv.y, cc);
                cc = fma(v[2], (double)wv.z, cc);
                cc = fma(v[3], (double)wv.w, cc);
            }
            BX_SB();
        }
#pragma unroll
    for (int o = 0; o < 3; ++o) out[o] = (float)((double)b3[o] + pair_sum_d(c[o][0] + c[o][1]));
}

// K steps 0 .. STEPS - 1 of the activation planes from the wave's staged encoding (feature 16 t + 8 h + j; NQ quads staged)
struct NoEncTap {
    __device__ __forceinline__ void operator()(int, const float (&)[8]) const {}
};
template <int STEPS, int NQ, class EncTap = NoEncTap>
__device__ __forceinline__ void enc_to_act(const float* encw, int lane, bf16x8 (&act)[3][16], EncTap enc_tap = EncTap()) {
    const float4* e4 = reinterpret_cast<const float4*>(encw);
    const int h = lane >> 5, c = lane & 31;
#pragma unroll
    for (int t = 0; t < STEPS; ++t) {
        float v[8];
#pragma unroll
        for (int qq = 0; qq < 2; ++qq) {
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (4 * t + 2 + qq < NQ) {  // (static) both lane halves inside the staged quads
                x = e4[(4 * t + 2 * h + qq) * WV_ROWS + c];
            } else if (4 * t + qq < NQ) {  // only the lower half
                // (component by component: a select between two float4 values is lowered to a scratch array indexed by h)
                const float4 y = e4[(4 * t + qq) * WV_ROWS + c];
                x.x = h == 0 ? y.x : 0.f;
                x.y = h == 0 ? y.y : 0.f;
                x.z = h == 0 ? y.z : 0.f;
                x.w = h == 0 ? y.w : 0.f;
            }
            v[4 * qq + 0] = x.x;
            v[4 * qq + 1] = x.y;
            v[4 * qq + 2] = x.z;
            v[4 * qq + 3] = x.w;
        }
        enc_tap(t, v);
        split8(v, act[0][t], act[1][t], act[2][t]);
        BX_SB();
    }
}

// ---------------------------------------------------------------------------------------------
// MotionNet on the wave's 32 samples: p += flow (modeling/layered_rfrender.py:356,510).  19 slots.
// ---------------------------------------------------------------------------------------------
// INST: which kernel inlines it (0: the stage kernel, 1: mlp_bf16x3_motion_kernel).  One shared function body changed the stage
// kernel's code (the same arithmetic, other registers and address constants in the MotionNet loop); two keep it as it was.
template <int INST = 0>
__device__ __forceinline__ void motion_bx(Ctx& cx, const float* net, const float* cm, float* encw, float (&p)[3], float tv, int flags,
                                          int lane, f32x16 (&big)[4], f32x16 (&small)[4], bf16x8 (&act)[3][16] BXP_PARAM) {
    const MotionLayout L = motion_layout();
    load_c(big, cm + BXM_B, lane);   // (in front of the encoding arithmetic: its LDS round trip is covered)
    encode_motion(encw, lane, p, tv, flags);
    wave_lds_sync();
    enc_to_act<6, WV_ENC_QUADS>(encw, lane, act);
    BXP(BXP_MOTION_ENC);
    pass_act<0, 3, true>(cx, big, small, act);  // motion_net.0: 84 (+4) inputs, 6 K steps
    BXP(BXP_MOTION_PASS);
#pragma unroll 1
    for (int li = 1; li <= 4; ++li) {
        finish_act<0>(big, small, act, cm + BXM_B + 128 * li, lane);
        BXP(BXP_MOTION_FIN);
        pass_act<0, 4, true>(cx, big, small, act);
        BXP(BXP_MOTION_PASS);
    }
    float fl[3];
    head3(big, small, cm + BXM_W_OUT, net + L.b_out, lane, fl);
#pragma unroll
    for (int c3 = 0; c3 < 3; ++c3) p[c3] = p[c3] + fl[c3];
    BXP(BXP_MOTION_FIN);
}

// ---------------------------------------------------------------------------------------------
// SpaceNet on the wave's 32 samples; returns {r, g, b, sigma} (raw) in every lane.  `mid` is called once, in front of the
// last backbone layer's boundary arithmetic (the caller issues the next work item's HBM loads there).
// ---------------------------------------------------------------------------------------------
// `tap` (training): BxStoreTap writes PE(pos) and every layer's post-ReLU output (stage 0 .. 6 = stage1.0 .. stage2.4, 7 = rgb_net.1)
// to the caller's matrices as they pass; BxNoTap compiles to the inference kernel.
template <bool DEEP, class Mid, class Tap>
__device__ __forceinline__ float4 space_bx(Ctx& cx, const float* net, const bool use_time, const float* cs, float* encw, const float (&p)[3],
                                           const float* __restrict__ raybias, int32_t ray, int lane, f32x16 (&big)[4], f32x16 (&small)[4],
                                           bf16x8 (&act)[3][16], Mid mid, const Tap& tap BXP_PARAM) {
    const SpaceLayout L = space_layout(use_time, DEEP);
    const int h = lane >> 5;
    constexpr int ST = Tap::on ? BX_TAP_PARK : 0;   // stores behind every park
    Park pk;
    load_c(big, cs + BXC_B, lane);   // (in front of the encoding arithmetic)
    encode_pos(encw, lane, p);
    wave_lds_sync();
    if constexpr (Tap::on) {   // feature 16 t + 8 h + j of the staged encoding: 32 bytes per lane and K step
        const bool valid = tap_valid(tap, lane);
        // (tap_row's "4 h" is 8 h here: a lane half owns 8 consecutive features of a K step)
        float4* dst = reinterpret_cast<float4*>(tap_row(tap, TAP_PE, 4 * h, lane));
        enc_to_act<4, 16>(encw, lane, act, [&](int t, const float (&v)[8]) {
            if (valid) {
                dst[4 * t] = make_float4(v[0], v[1], v[2], v[3]);
                dst[4 * t + 1] = make_float4(v[4], v[5], v[6], v[7]);
            }
        });
    } else {
        enc_to_act<4, 16>(encw, lane, act);
    }
    BXP(BXP_PE);
    // ---- stage1.0: 63 (+1) -> 256.  Every pass's C operand (its bias) is read block by block inside the boundary pass in
    // front of it, as soon as a block's accumulators have been consumed.
    pass_act<0, 2, true, false, Tap::on ? BX_TAP_PE : 0>(cx, big, small, act);
    BXP(BXP_PASS);
    finish_park(big, small, pk, cs + BXC_B + 128, lane, tap, 0, 0);
    BXP(BXP_PARK);
    pass_act<0, 2, true, false, ST>(cx, big, small, act);
    BXP(BXP_PASS);
    unpark_act(pk, act);                                     // first pass -> K steps 0 .. 7 (in the open: the only layer whose
    BXP(BXP_ACT);                                            // successor's first pass cannot start before it)
    finish_park(big, small, pk, cs + BXC_B + 256, lane, tap, 0, 128);   // second pass -> park: converted under stage1.2's first K steps
    BXP(BXP_PARK);
    // ---- stage1.2 .. stage2.4: six 256-wide layers, two passes each; stage2.0 (li == 4) takes PE(pos) again behind its 256
    // features (modeling/spacenet.py:45-57,136-138): four more K steps per pass, their B operands split on the spot from the
    // staged encoding (the activation planes are full)
    // (The three lambdas below are inlined into the inference kernel by the inliner's own choice; with the tap's code in them it
    // declines, and a real call passes the wave's 400 live registers through memory.  The tap variant forces them AT THE CALL -- an
    // attribute on the lambdas themselves changes the inlining order, and with it the code, of the inference kernel.)
#define BX_INLINED(call)                           \
    do {                                           \
        if constexpr (Tap::on) {                   \
            [[clang::always_inline]] call;         \
        } else {                                   \
            call;                                  \
        }                                          \
    } while (0)
    auto pe_slots = [&]() {
        const float4* e4 = reinterpret_cast<const float4*>(encw);
#pragma unroll
        for (int sl = 0; sl < 2; ++sl) {
            bf16x8 pe[2][3];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float v[8];
#pragma unroll
                for (int qq = 0; qq < 2; ++qq) {
                    const float4 x = e4[(4 * (2 * sl + t) + 2 * h + qq) * WV_ROWS + (lane & 31)];
                    v[4 * qq + 0] = x.x;
                    v[4 * qq + 1] = x.y;
                    v[4 * qq + 2] = x.z;
                    v[4 * qq + 3] = x.w;
                }
                split8(v, pe[t][0], pe[t][1], pe[t][2]);
            }
            slot<false>(cx, big, small, pe[0][0], pe[0][1], pe[0][2], pe[1][0], pe[1][1], pe[1][2]);
        }
    };
    // (stage2.0 is peeled out of the layer loop: inside it, as a conditional block, its extra K steps redefine the
    // accumulators on one of two paths and the register allocator answers with ~200 spills)
    auto layer = [&](int li, auto with_pe) {
        pass_a_unpark<false, ST>(cx, big, small, act, pk);   // K steps 0 .. 7, the previous layer's second pass -> K steps 8 .. 15
        pass_act<8, 4, false>(cx, big, small, act);
        if constexpr (decltype(with_pe)::value) BX_INLINED(pe_slots());
        BXP(BXP_PASS);
        finish_park(big, small, pk, cs + BXC_B + 256 * li + 128, lane, tap, li, 0);
        BXP(BXP_PARK);
        pass_b_unpark<ST>(cx, big, small, act, pk);
        if constexpr (decltype(with_pe)::value) BX_INLINED(pe_slots());
        BXP(BXP_PASS);
    };
    auto layer_end = [&](int li) {   // (+ the next layer's first C operand; behind stage2.4 comes rgb_net.1, which starts from 0)
        finish_park(big, small, pk, li < 6 ? cs + BXC_B + 256 * (li + 1) : nullptr, lane, tap, li, 128);
        BXP(BXP_PARK);
    };
#pragma unroll 1
    for (int li = 1; li <= 3; ++li) {
        BX_INLINED(layer(li, std::false_type{}));
        BX_INLINED(layer_end(li));
    }
    BX_INLINED(layer(4, std::true_type{}));
    BX_INLINED(layer_end(4));
    float sigma = 0.f;
#pragma unroll 1
    for (int li = 5; li <= 6; ++li) {
        BX_INLINED(layer(li, std::false_type{}));
        if (li == 6) {  // sigma = density_net(h) (:139), raw; the next work item's HBM loads go out in front of it
            mid();
            sigma = sigma_head(big, small, pk, cs + BXC_W_SIGMA, net[L.b_sigma], lane);
            BXP(BXP_SIGMA);
        }
        BX_INLINED(layer_end(li));
    }
#undef BX_INLINED
    // ---- rgb_net: relu -> Linear(283|304, 128) -> relu -> Linear(128, 3) (:80-86); the 256 backbone columns here, the
    // bias + direction / time columns = this sample's row of the ray-bias table (mlp_raybias.hip).  It is added BEHIND the K loop
    // (in the exact-f32 kernels likewise: relu_add_rebias, mlp_wave_core.h): it is an order of magnitude larger than the backbone
    // part, and as the C operand it would put every rounding of the a0 b0 chain at its scale (measured: the colour output at
    // 1.3 x the fp32 CPU chain's error instead of 0.5 x).  Its 16 loads go out in front of the pass's last slot (14 of the 16
    // K steps' activation registers are dead by then).
    pass_a_unpark<true, ST>(cx, big, small, act, pk);        // (stage2.4's second pass is converted under its first K steps)
    pass_act<8, 3, false>(cx, big, small, act);
    BXP(BXP_PASS);
    {
        float4 crow[4][4];
        const float* row = raybias + (int64_t)ray * 128 + 4 * h;
#pragma unroll
        for (int fb = 0; fb < 4; ++fb)
#pragma unroll
            for (int q = 0; q < 4; ++q) crow[fb][q] = *reinterpret_cast<const float4*>(row + fb * 32 + 8 * q);
        pass_act<14, 1, false>(cx, big, small, act);
        BXP(BXP_PASS);
#pragma unroll
        for (int fb = 0; fb < 4; ++fb) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                big[fb][4 * q + 0] = (big[fb][4 * q + 0] + small[fb][4 * q + 0]) + crow[fb][q].x;
                big[fb][4 * q + 1] = (big[fb][4 * q + 1] + small[fb][4 * q + 1]) + crow[fb][q].y;
                big[fb][4 * q + 2] = (big[fb][4 * q + 2] + small[fb][4 * q + 2]) + crow[fb][q].z;
                big[fb][4 * q + 3] = (big[fb][4 * q + 3] + small[fb][4 * q + 3]) + crow[fb][q].w;
            }
#pragma unroll
            for (int i = 0; i < 16; ++i) small[fb][i] = 0.f;
            BX_SB();
        }
    }
    if constexpr (Tap::on) finish_park<false>(big, small, pk, nullptr, lane, tap, 7, 0);   // relu(rgb_net.1): rgb_net.3's input
    if constexpr (DEEP) {  // deep_rgb (:68-79): two more 128-wide hidden layers
#pragma unroll 1
        for (int i = 0; i < 2; ++i) {
            finish_act<0>(big, small, act, cs + BXC_B_DEEP + 128 * i, lane);
            pass_act<0, 4, true>(cx, big, small, act);
        }
    }
    float rgb[3];
    head3(big, small, cs + BXC_W_RGB2, net + L.b_rgb2, lane, rgb);
    BXP(BXP_RGB_TAIL);
    return make_float4(rgb[0], rgb[1], rgb[2], sigma);
}

// ---------------------------------------------------------------------------------------------
// The ring's start, the same in every kernel built on it.  ring_init() in front of the caller's own set-up (the segments, `idle`,
// `st_on` stay with the kernel: they are what differs), ring_start() behind it: three slots in flight, the first one landed
// everywhere, the A operands of its first two units on their way -- the first unit<0, ..> can run.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void ring_init(Ctx& cx, char* ring, int wave, int lane) {
    cx.ring = ring;
    cx.wave = wave;
    cx.lane = lane;
    cx.gi = 0;
    cx.gc = 0;
    cx.rcur = (uint32_t)(uintptr_t)ring + (uint32_t)lane * 16u;   // LDS byte address of the ring + lane * 16
    cx.rnext = cx.rcur + BX_SLOT;
}
__device__ __forceinline__ void ring_start(Ctx& cx) {
    dma_issue(cx);
    dma_issue(cx);
    dma_issue(cx);
    BX_VMCNT(12);
    __builtin_amdgcn_s_barrier();
    a_read<0>(cx.A[0].p[0], cx.rcur);
    a_read<BX_CHUNK>(cx.A[0].p[1], cx.rcur);
    a_read<2 * BX_CHUNK>(cx.A[0].p[2], cx.rcur);
    a_read<BX_UNIT>(cx.A[1].p[0], cx.rcur);
    a_read<BX_UNIT + BX_CHUNK>(cx.A[1].p[1], cx.rcur);
    a_read<BX_UNIT + 2 * BX_CHUNK>(cx.A[1].p[2], cx.rcur);
}

}  // namespace stnerf
