// Compositor: density edits + per-layer composite + cross-layer depth merge + merged composite.  One WAVE (64 lanes) owns
// one ray; every cumulative quantity (the transmittance product, the five weighted sums) is a wavefront prefix scan.
//
// HBM-bound by its bytes: reads 20 B/sample (+1 B/layer mask) and writes 20 B per (ray, output).
//
// Reference: layers/render_layer.py:8-58, modeling/layered_rfrender.py:414-448, :538-606.
#include "common.h"
#include "composite_rules.h"
#include "wave_prims.h"
#include <cstdlib>
#include <cstring>

// Occupancy targets (waves per SIMD) of the kernels: the VGPR budget follows from them (512 / waves).
#ifndef STNERF_WAVES_COMPOSITE
#define STNERF_WAVES_COMPOSITE 6
#endif
#ifndef STNERF_WAVES_SINGLE
#define STNERF_WAVES_SINGLE 6
#endif

namespace stnerf {

// ---------------------------------------------------------------------------------------------
// Alpha-composite (gen_weight + VolumeRenderer.forward: layers/render_layer.py:8-17, :37-49), 64 samples at a time:
//   delta_k = t_{k+1}-t_k, last = border;  alpha = 1-exp(-relu(sigma) delta);
//   T_k = prod_{j<k} (1-alpha_j+1e-10);  w = alpha T;  color = sum w sigmoid(rgb); depth = sum w t.
// ---------------------------------------------------------------------------------------------
// (CompositeAcc, the running state of one composite, and composite_store5 are in composite_rules.h)
// One block of 64 samples (lane = sample): weight of the lane's sample, sums updated.  Every composite of this file is a loop
// over this function (the kernels are compared bit for bit).  `ok`: the lane holds a sample; an idle lane (ALL = false
// only) passes finite values, contributes the factor 1 to the transmittance and weight 0 to the sums.
template <bool ALL>
__device__ __forceinline__ float composite_block(CompositeAcc& A, float sigma, float delta, float r, float g, float b, float t, bool ok) {
    float alpha = 1.f - exp_neg(fmaxf(sigma, 0.f) * delta);
    float tr = (1.f - alpha) + 1e-10f;
    if (!ALL) {
        alpha = ok ? alpha : 0.f;
        tr = ok ? tr : 1.f;
    }
    const float incl = wave_scan_mul(tr);
    const float excl = wave_prev(incl, 1.f);
    float w = alpha * (A.carry * excl);
    A.carry = A.carry * wave_last(incl);
    if (!ALL) w = ok ? w : 0.f;   // (alpha = 0 does not make it zero when the transmittance has overflowed)
    A.cr += w * r;
    A.cg += w * g;
    A.cb += w * b;
    A.cd += w * t;
    A.ca += w;
    return w;
}

// `count` samples read through accessor functors, in index order.  raw_at(k) returns the edited sample
// {sigmoid(r), sigmoid(g), sigmoid(b), sigma}.  Returns bit 0: some t_{k+1} < t_k (the list is not ascending); bit 1: some
// t_{k+1} >= t_k (it is not strictly descending) -- per lane, the caller reduces over the wave.
template <class TAt, class RawAt, class WOut>
__device__ __forceinline__ int composite_run(CompositeAcc& A, int count, float border, int lane, TAt t_at, RawAt raw_at, WOut w_out) {
    bool descending = false, not_descending = false;
    for (int base = 0; base < count; base += 64) {
        const int k = base + lane;
        const bool ok = k < count;
        float tk = 0.f, delta = 0.f;
        float4 rw = make_float4(0.f, 0.f, 0.f, 0.f);
        if (ok) {
            tk = t_at(k);
            rw = raw_at(k);
            delta = border;
            if (k + 1 < count) {
                const float tn = t_at(k + 1);
                descending = descending || (tn < tk);
                not_descending = not_descending || !(tn < tk);
                delta = tn - tk;
            }
        }
        const float w = composite_block<false>(A, rw.w, delta, rw.x, rw.y, rw.z, tk, ok);
        if (ok) w_out(k, w);
    }
    return (descending ? 1 : 0) | (not_descending ? 2 : 0);
}

// A whole layer in registers (block b of lane i = sample 64 b + i, tn = the depth of the sample behind it; FULL: S = 64 * MAXB,
// no lane is ever idle): the layers of the single-layer and the merge kernel, which need no LDS staging.  cut_near: the
// merged stream's `t < near` cut of the fine stage (modeling/layered_rfrender.py:605).  wdst: the layer's weights, or null;
// wdst2: a second copy of them (the layer's row of merged_weights where the merged composite IS this one), or null.
template <int MAXB, bool FULL>
__device__ __forceinline__ void composite_regs(CompositeAcc& A, unsigned S, float border, unsigned lane, const float (&tk)[MAXB],
                                               const float (&tn)[MAXB], const float4 (&rw)[MAXB], bool cut_near, float nearv,
                                               float* wdst, float* wdst2 = nullptr) {
#pragma unroll
    for (int b = 0; b < MAXB; ++b) {
        if (FULL || (unsigned)b * 64u < S) {  // (uniform)
            const unsigned k = (unsigned)b * 64u + lane;
            const bool ok = FULL || k < S;
            const bool last = FULL ? (b + 1 == MAXB && lane == 63u) : (k + 1u >= S);
            const float delta = last ? border : tn[b] - tk[b];
            const float sg = (cut_near && tk[b] < nearv) ? 0.f : rw[b].w;
            const float w = composite_block<FULL>(A, sg, delta, rw[b].x, rw[b].y, rw[b].z, tk[b], ok);
            if (wdst && ok) wdst[k] = w;
            if (wdst2 && ok) wdst2[k] = w;
        }
    }
}

// gen_weight stand-alone: one wave per row.
__global__ void gen_weight_kernel(const float* __restrict__ sigma, const float* __restrict__ delta, int64_t n, int S,
                                  float* __restrict__ weights) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (row >= n) return;
    CompositeAcc A;   // (only the transmittance carry is used: the sums are dead code here)
    for (int base = 0; base < S; base += 64) {
        const int k = base + lane;
        const bool ok = k < S;
        const float w = composite_block<false>(A, ok ? sigma[row * S + k] : 0.f, ok ? delta[row * S + k] : 0.f, 0.f, 0.f, 0.f, 0.f, ok);
        if (ok) weights[row * S + k] = w;
    }
}

struct CompositeArgs {
    const float* t;
    const float4* raw;
    const uint8_t* mask;
    int64_t n;
    int l, S;
    stnerf_composite_params p;
    float* layer_out;
    float* mixed_out;
    float* weights;
    int32_t* order;
    int waves_per_block;
    int p2;  // floor_pow2(S)
    uint8_t* handled;  // [n] or nullptr: rays composite_single_kernel has already finished (it writes 0 / 1 for every ray)
    int lds_layers;    // composite_merge_kernel: layers its merged list holds (rays with more live layers are left to the next launch)
    // [n][l][S] or nullptr: the weight of every sample in the MERGED composite, stored at its source index (zeros for a layer that
    // is not live).  Needs mixed_out.  Only the MW instantiations of the production kernels look at it.
    float* merged_weights;
};

// ONE live layer whose list is ascending, held in registers as composite_regs takes it (idle lanes: zeros): edit it,
// composite it and write every output of the ray -- the layer's weights and composite, zeros for the layers the ray
// misses, and the mix, which is that layer's composite (same samples, deltas, arithmetic) unless the fine stage's
// `t < near` cut (:605) bites, which costs a second pass over the registers.  have: the layer has network output
// (without it -- a hidden layer, a grazing hit -- its samples are the zero tensors of :398-399).  MW: a.merged_weights (may
// still be null) gets the weights of whichever pass made the mix; the others' rows are zero.
template <int MAXB, bool MW>
__device__ __forceinline__ void composite_single_layer(const CompositeArgs& a, int64_t ray, int layer, bool have, unsigned lane,
                                                       const float (&tk)[MAXB], const float (&tn)[MAXB], float4 (&rw)[MAXB]) {
    const float nearv = a.p.near;
    if (have) {
        const LayerEdit ed = layer_edit(a.p, layer);
#pragma unroll
        for (int b = 0; b < MAXB; ++b) rw[b] = edit_sample(rw[b], tk[b], ed.cut_neg, ed.thr, ed.scale, ed.cut_near, nearv, a.p.rgb_activated != 0);
    }
    float* mw = nullptr;      // the layer's row of merged_weights
    bool mw_first = false;    // ... which the first pass writes: the mix is the layer's composite
    if (MW && a.merged_weights) {
        mw = a.merged_weights + (ray * a.l + layer) * a.S;
        mw_first = !(a.p.fine && __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tk[0]), 0)) < nearv);
    }
    CompositeAcc A;
    composite_regs<MAXB, false>(A, (unsigned)a.S, a.p.border, lane, tk, tn, rw, false, 0.f,
                                a.weights ? a.weights + (ray * a.l + layer) * a.S : nullptr, MW && mw_first ? mw : nullptr);
    for (int other = 0; other < a.l; ++other) {  // the layers the ray misses: zero weights and outputs
        if (other == layer) continue;
        if (a.weights)
            for (int k = (int)lane; k < a.S; k += 64) a.weights[(ray * a.l + other) * a.S + k] = 0.f;
        if (MW && a.merged_weights)
            for (int k = (int)lane; k < a.S; k += 64) a.merged_weights[(ray * a.l + other) * a.S + k] = 0.f;
        if (a.layer_out && lane < 5u) a.layer_out[(ray * a.l + other) * 5 + lane] = 0.f;
    }
    const float t_first = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tk[0]), 0));
    const bool mix_is_layer = !(a.p.fine && t_first < nearv);
    composite_store5(A, a.layer_out ? a.layer_out + (ray * a.l + layer) * 5 : nullptr,
                     a.mixed_out && mix_is_layer ? a.mixed_out + ray * 5 : nullptr, lane);
    if (a.mixed_out && !mix_is_layer) {
        CompositeAcc M;
        composite_regs<MAXB, false>(M, (unsigned)a.S, a.p.border, lane, tk, tn, rw, true, nearv, MW ? mw : nullptr);
        composite_store5(M, a.mixed_out + ray * 5, nullptr, lane);
    }
}

// The LDS-staged compositor: every ray on its own, the whole ray (all l * S samples) in LDS, rank merge by binary
// searches.  Since round 3 it serves the `order` parity output and layers of more than 192 samples only; production
// calls take composite_single_kernel + composite_merge_kernel below (same numbers, bit for bit).
__global__ void __attribute__((amdgpu_waves_per_eu(STNERF_WAVES_COMPOSITE, 8))) composite_kernel(CompositeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // (uniform: ray index and addresses on the scalar unit)
    const int LS = a.l * a.S;
    // per-wave LDS: raws[LS] float4 | ts[LS] float | mord[LS] u16 (merged position -> source sample), 16-B rounded
    const int per_wave = ((LS * 22 + 15) / 16) * 16;
    unsigned char* mine = smem_raw + (size_t)wave * per_wave;
    float4* raws = reinterpret_cast<float4*>(mine);
    float* ts = reinterpret_cast<float*>(mine + (size_t)LS * 16);
    unsigned short* mord = reinterpret_cast<unsigned short*>(ts + LS);
    const EvalBits ev = eval_bits<false>(a.p, a.l);
    const unsigned all_layers = a.l >= 32 ? ~0u : (1u << a.l) - 1u;

    // Rank of every sample of the layers in `take` among them == its position in a stable sort of their concatenation
    // (ties resolve by source index, layer-major): put(rank, source sample).  Layers are ascending or (bit of `reversed`)
    // strictly descending, searched through a reversed view; !sorted: the general O(n^2) rank over every sample of the ray
    // (missed layers included: they sort first, weight 0).  Returns the number of samples ranked.
    auto rank_samples = [&](unsigned take, unsigned reversed, bool sorted, auto put) -> int {
        if (!sorted) {
            for (int e = lane; e < LS; e += 64) {
                const float v = ts[e];
                int rank = 0;
                for (int x = 0; x < LS; ++x) {
                    const float xv = ts[x];
                    rank += (xv < v || (xv == v && x < e)) ? 1 : 0;
                }
                put(rank, e);
            }
            return LS;
        }
        int count = 0;
        for (int la = 0; la < a.l; ++la) {
            if (!(take >> la & 1u)) continue;
            for (int k = lane; k < a.S; k += 64) {
                const int e = la * a.S + k;
                const float v = ts[e];
                int rank = (reversed >> la & 1u) ? a.S - 1 - k : k;
                for (int lb = 0; lb < la; ++lb)
                    if (take >> lb & 1u)
                        rank += (reversed >> lb & 1u) ? upper_bound_lds_rev(ts + lb * a.S, a.S, a.p2, v)
                                                      : upper_bound_lds(ts + lb * a.S, a.S, a.p2, v);
                for (int lb = la + 1; lb < a.l; ++lb)
                    if (take >> lb & 1u)
                        rank += (reversed >> lb & 1u) ? lower_bound_lds_rev(ts + lb * a.S, a.S, a.p2, v)
                                                      : lower_bound_lds(ts + lb * a.S, a.S, a.p2, v);
                put(rank, e);
            }
            count += a.S;
        }
        return count;
    };

    const int64_t rays_per_iter = (int64_t)gridDim.x * a.waves_per_block;
    // hit mask (lanes 0 .. l-1) and `handled` flag (lane 63) of a ray in ONE load each, fetched one ray ahead: the
    // chain "flags -> which layers -> their samples" is otherwise two or more dependent HBM round trips per ray
    auto ray_flags = [&](int64_t ray) -> int {
        int v = 0;
        if (ray < a.n) {
            if (lane < a.l && a.mask) v = a.mask[ray * a.l + lane];
            if (lane == 63 && a.handled) v = a.handled[ray];
        }
        return v;
    };
    int flags_next = ray_flags((int64_t)blockIdx.x * a.waves_per_block + wave);
    CP_DECL
    for (int64_t ray0 = (int64_t)blockIdx.x * a.waves_per_block; ray0 < a.n; ray0 += rays_per_iter) {
        const int64_t ray = ray0 + wave;
        const unsigned long long fb = __ballot((flags_next & 1) != 0 || (lane == 63u && flags_next != 0));
        const unsigned miss_bits = (unsigned)__ballot((flags_next & 2) != 0) & 0xffffu;   // (hint of the sampler: every depth is -1000)
        flags_next = ray_flags(ray + rays_per_iter);
        const unsigned mask_bits = (unsigned)fb;
        const bool active = ray < a.n && !(fb >> 63 & 1ull);
        int n_merged = 0;
        CP(0);
        // ---- which layers take part.
        // A layer the ray misses altogether (not evaluated, every t == -1000: bin width 0 from start = end = -1000,
        // layers/RaySamplePoint.py:53-62,98-102) is dropped from everything below: its samples have sigma = 0, so
        // alpha = 0, w = 0 and the transmittance factor fl(1 - 0 + 1e-10) is exactly 1; they sort in front of every
        // real sample, so they are nobody's successor and change no delta.  The composites are the same numbers (the
        // dropped factors are exact ones; only the association order of the parallel transmittance scan moves with the
        // lane a sample lands in, i.e. fp32 rounding), and with performers covering a fraction of the image most rays
        // carry one or two live layers instead of l.  The `order` parity output does not change what is composited
        // (tests/test_gpu_ops.py::test_composite_production_shortcuts_are_bitwise_neutral).
        // (A not-evaluated layer with real depths -- hidden, or a grazing hit -- still takes part: its depths
        // shape its neighbours' deltas.)
        unsigned live = 0, have_m = 0;  // bit i: layer i takes part / has network output on this ray
        if (active) {
            const float* tsrc = a.t + ray * LS;
            have_m = have_layers(ev, a.mask != nullptr, mask_bits) & all_layers;
            live = have_m;
            for (int layer = 0; layer < a.l; ++layer) {
                if (!(have_m >> layer & 1u) && !(miss_bits >> layer & 1u)) {  // without output a layer still takes part if it has real depths (hidden, or a grazing hit)
                    bool missed = true;
                    for (int k = lane; k < a.S; k += 64) missed = missed && tsrc[layer * a.S + k] == -1000.f;
                    if (!__all(missed)) live |= 1u << layer;
                }
            }
        }
        CP(1);
        // ---- ONE live layer (about half the rays of a view: the background alone): composite it straight from
        // registers -- no LDS staging, no merge.
        bool done = false;
        constexpr int MAXB = 3;
        if (active && __popc(live) == 1 && a.S <= 64 * MAXB) {
            const int layer = __ffs(live) - 1;
            const bool have = (have_m >> layer & 1u) != 0;
            const float* tl = a.t + ray * LS + layer * a.S;
            const float4* rl = a.raw + ray * LS + layer * a.S;
            float tk[MAXB], tn[MAXB];
            float4 rw[MAXB];
            bool desc = false;
#pragma unroll
            for (int b = 0; b < MAXB; ++b) {
                const int k = b * 64 + lane;
                tk[b] = tn[b] = 0.f;
                rw[b] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (k < a.S) {
                    tk[b] = tl[k];
                    if (k + 1 < a.S) {
                        tn[b] = tl[k + 1];
                        desc = desc || (tn[b] < tk[b]);
                    }
                    if (have) rw[b] = rl[k];
                }
            }
            if (!__any(desc)) {  // (a descending list needs the merge to turn it round: general path)
                composite_single_layer<MAXB, true>(a, ray, layer, have, (unsigned)lane, tk, tn, rw);
                if (a.order) {  // ascending single layer + leading -1000 samples of the others: computed below
                    const float* tsrc = a.t + ray * LS;
                    for (int e = lane; e < LS; e += 64) ts[e] = tsrc[e];
                }
                done = true;
            }
        }
        CP(2);
        // ---- general path: stage the ray in LDS, applying the post-network density edits (a10); layer-major so
        // every edit switch is wave-uniform.
        if (active && !done) {
            const float* tsrc = a.t + ray * LS;
            const float4* rsrc = a.raw + ray * LS;
            for (int layer = 0; layer < a.l; ++layer) {
                const bool have = (have_m >> layer & 1u) != 0;
                const LayerEdit ed = layer_edit(a.p, layer);
                // every load of the layer is issued before the first one is consumed: written as a plain
                // load -> edit -> store loop each 64-sample block costs its own HBM round trip
                constexpr int SB = 3;
                for (int k0 = 0; k0 < a.S; k0 += 64 * SB) {
                    float tv[SB];
                    float4 rv[SB];
#pragma unroll
                    for (int b = 0; b < SB; ++b) {
                        const int k = k0 + b * 64 + lane;
                        tv[b] = 0.f;
                        rv[b] = make_float4(0.f, 0.f, 0.f, 0.f);  // zero tensors (:398-399); sigma = 0 makes the colour moot
                        if (k < a.S) {
                            tv[b] = tsrc[layer * a.S + k];
                            if (have) rv[b] = rsrc[layer * a.S + k];
                        }
                    }
#pragma unroll
                    for (int b = 0; b < SB; ++b) {
                        const int k = k0 + b * 64 + lane;
                        if (k < a.S) {
                            const int e = layer * a.S + k;
                            ts[e] = tv[b];
                            raws[e] = have ? edit_sample(rv[b], tv[b], ed.cut_neg, ed.thr, ed.scale, ed.cut_near, a.p.near, a.p.rgb_activated != 0) : rv[b];
                        }
                    }
                }
            }
        }
        wave_sync();
        CP(3);
        // ---- per-layer composites (:435-444 / :598-603)
        bool merged_done = false, sorted_ok = true;
        unsigned reversed = 0;  // bit i: layer i is strictly descending
        if (active && !done) {
            // a layer's list is ascending, unless its bin width is negative: a box edit, or a ray that misses the
            // background box (far = -1000, start clamped to 0: depths run from 0 down to -1000).  Such a list is strictly
            // descending and is merged through a reversed view; anything else (ties inside a descending list) takes
            // the general rank.
            const bool single = __popc(live) == 1;  // one live layer: the union IS that layer
            for (int layer = 0; layer < a.l; ++layer) {
                float* wdst = a.weights ? a.weights + (ray * a.l + layer) * a.S : nullptr;
                float* mdst = a.merged_weights ? a.merged_weights + (ray * a.l + layer) * a.S : nullptr;
                if (!(live >> layer & 1u)) {  // missed: every weight and every composite output is zero
                    if (wdst)
                        for (int k = lane; k < a.S; k += 64) wdst[k] = 0.f;
                    if (mdst)
                        for (int k = lane; k < a.S; k += 64) mdst[k] = 0.f;
                    if (a.layer_out && lane < 5) a.layer_out[(ray * a.l + layer) * 5 + lane] = 0.f;
                    continue;
                }
                const float* tl = ts + layer * a.S;
                const float4* rl = raws + layer * a.S;
                // merged weights of a single live layer without the near cut: these, if the list turns out ascending (a
                // descending one goes through the merged composite below, which writes every live sample's slot again)
                if (!(single && !(a.p.fine && tl[0] < a.p.near))) mdst = nullptr;
                CompositeAcc A;
                const int dir = composite_run(A, a.S, a.p.border, lane, [&](int k) { return tl[k]; }, [&](int k) { return rl[k]; },
                                              [&](int k, float w) {
                                                  if (wdst) wdst[k] = w;
                                                  if (mdst) mdst[k] = w;
                                              });
                const bool some_desc = __any(dir & 1), some_asc = __any(dir & 2);
                if (some_desc && !some_asc) reversed |= 1u << layer;
                sorted_ok = sorted_ok && !(some_desc && some_asc);
                // one live, ascending layer -- same samples, same deltas, same arithmetic: the layer's composite is the mix,
                // unless the fine stage's `t < near` cut (:605) bites
                merged_done = single && !some_desc && !(a.p.fine && tl[0] < a.p.near);
                composite_store5(A, a.layer_out ? a.layer_out + (ray * a.l + layer) * 5 : nullptr,
                                 merged_done && a.mixed_out ? a.mixed_out + ray * 5 : nullptr, (unsigned)lane);
            }
            CP(4);
            // ---- cross-layer merge by depth (:425-429 / :587-592): the live samples only
            if (!merged_done) n_merged = rank_samples(live, reversed, sorted_ok, [&](int rank, int e) { mord[rank] = (unsigned short)e; });
        }
        wave_sync();
        CP(5);
        // ---- merged composite (:448 / :605-606)
        if (active && !done && !merged_done && a.mixed_out) {
            const bool cut_near = a.p.fine != 0;
            const float nearv = a.p.near;
            CompositeAcc A;
            composite_run(A, n_merged, a.p.border, lane, [&](int m) { return ts[mord[m]]; },
                          [&](int m) {
                              const int src = mord[m];
                              float4 rw = raws[src];
                              if (cut_near && ts[src] < nearv) rw.w = 0.f;  // :605
                              return rw;
                          },
                          [&](int m, float w) {
                              if (a.merged_weights) a.merged_weights[ray * LS + mord[m]] = w;
                          });
            composite_store5(A, a.mixed_out + ray * 5, nullptr, (unsigned)lane);
        }
        CP(6);
        // ---- optional parity output: torch.sort's index over ALL l * S samples (the composites above leave the
        // layers a ray misses out; their samples, t = -1000, sort in front of everything and carry no weight)
        if (active && a.order) {
            int32_t* od = a.order + ray * LS;
            rank_samples(all_layers, reversed, sorted_ok, [&](int rank, int e) { od[rank] = e; });
        }
        wave_sync();
    }
    CP_FLUSH;
}

// ---------------------------------------------------------------------------------------------
// Rays with ONE live layer (about half the rays of a view: the background alone), software pipelined.
// composite_kernel spends ~10 us per ray on such a ray although it needs ~150 instructions: the chain
// "hit mask -> (which layer?) -> its samples -> composite -> store" is two dependent HBM round trips per ray with
// nothing else for the wave to do, and 8 waves per SIMD cannot hide that.  This kernel needs no LDS and runs the
// chain as a three-stage pipeline over the rays of a wave: while ray j is composited from registers, the samples of ray
// j+1 (whose mask arrived one iteration earlier) and the mask of ray j+2 are in flight.  It writes handled[ray] = 1
// for the rays it finishes and 0 for the others (several live layers, a descending list, a masked-out layer with real
// depths, ...), which composite_kernel then takes.  Same arithmetic, same lanes as composite_kernel: bit-identical.
// ---------------------------------------------------------------------------------------------
template <int MAXB, int MAXCHK>
struct SingleBuf {
    float tk[MAXB], tn[MAXB], chk[MAXCHK];
    float4 rw[MAXB];
    int layer;
    bool eligible;
};

// MW: the launch also writes a.merged_weights (the instantiation without it is the one every render without the pass runs).
template <int MAXB, int MAXCHK, bool MW>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(MAXB > 2 ? 4 : STNERF_WAVES_SINGLE, 8))) composite_single_kernel(CompositeArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t first = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int LS = a.l * a.S, B = (a.S + 63) >> 6;
    const EvalBits ev = eval_bits<false>(a.p, a.l);
    using Buf = SingleBuf<MAXB, MAXCHK>;
    auto mask_lane = [&](int64_t ray) -> int { return (a.mask && ray < a.n && lane < a.l) ? (int)a.mask[ray * a.l + lane] : 0; };
    auto have_of = [&](int mv) -> unsigned { return have_layers(ev, a.mask != nullptr, (unsigned)__ballot((mv & 1) != 0)); };
    auto miss_of = [&](int mv) -> unsigned { return (unsigned)__ballot((mv & 2) != 0); };   // (the sampler's hint: every depth -1000)
    const unsigned all_layers = a.l >= 32 ? ~0u : (1u << a.l) - 1u;
    auto issue = [&](Buf& b, int64_t ray, unsigned have, unsigned miss) {
        b.eligible = ray < a.n && __popc(have) == 1;
        b.layer = b.eligible ? __ffs(have) - 1 : 0;
#pragma unroll
        for (int i = 0; i < MAXB; ++i) {
            b.tk[i] = b.tn[i] = 0.f;
            b.rw[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int c = 0; c < MAXCHK; ++c) b.chk[c] = -1000.f;
        if (b.eligible) {
            const float* tsrc = a.t + ray * LS;
            const float* tl = tsrc + b.layer * a.S;
            const float4* rl = a.raw + ray * LS + b.layer * a.S;
#pragma unroll
            for (int i = 0; i < MAXB; ++i) {
                const int k = i * 64 + lane;
                if (k < a.S) {
                    b.tk[i] = tl[k];
                    if (k + 1 < a.S) b.tn[i] = tl[k + 1];
                    b.rw[i] = rl[k];
                }
            }
            const unsigned others = all_layers & ~(1u << b.layer);
            if ((miss & others) != others) {   // (uniform) not every other layer carries the sampler's "missed" hint: look
#pragma unroll
                for (int c = 0; c < MAXCHK; ++c) {  // depths of the other layers: "missed" means every one of them is -1000
                    const int oi = c / B, blk = c - oi * B;
                    const int x = oi < b.layer ? oi : oi + 1;
                    const int k = blk * 64 + lane;
                    if (oi < a.l - 1 && k < a.S) b.chk[c] = tsrc[x * a.S + k];
                }
            }
        }
    };
    int64_t r0 = first, r1 = first + stride, r2 = first + 2 * stride;
    Buf cur, nxt;
    int m1;
    {
        const int m0 = mask_lane(r0);
        m1 = mask_lane(r1);
        issue(cur, r0, have_of(m0), miss_of(m0));
    }
    for (; r0 < a.n; r0 = r1, r1 = r2, r2 += stride) {
        const unsigned have1 = have_of(m1), miss1 = miss_of(m1);
        const int m2 = mask_lane(r2);
        issue(nxt, r1, have1, miss1);
        __builtin_amdgcn_sched_barrier(0);  // keep the loads of the next ray ahead of this ray's arithmetic
        // ---- ray r0 from `cur`
        bool ok = cur.eligible;
        if (ok) {
            bool others_missed = true, desc = false;
#pragma unroll
            for (int c = 0; c < MAXCHK; ++c) others_missed = others_missed && cur.chk[c] == -1000.f;
#pragma unroll
            for (int i = 0; i < MAXB; ++i) desc = desc || (i * 64 + lane + 1 < a.S && cur.tn[i] < cur.tk[i]);
            ok = __all(others_missed) && !__any(desc);
        }
        if (ok) composite_single_layer<MAXB, MW>(a, r0, cur.layer, true, (unsigned)lane, cur.tk, cur.tn, cur.rw);
        if (lane == 0) a.handled[r0] = ok ? 1 : 0;
        cur = nxt;
        m1 = m2;
    }
}

// ---------------------------------------------------------------------------------------------
// Rays with SEVERAL live layers (round 3): layers in registers, merge by insertion.
//
// composite_kernel stages the whole ray in LDS (22 B per sample: 8.4 KB per wave at 3 x 128 samples, 38 KB at 9 x 192 --
// one wave per SIMD) and ranks every sample against every other layer (log2 S dependent LDS reads per sample and layer:
// cost ~ l^2).  This kernel keeps a layer in registers while it is composited (composite_regs, as the single-layer
// kernel above), and builds the merged order one layer at a time in a 6 B / sample LDS list
// (depth + source index):
//   * the samples of the NEW layer search the list merged so far (one upper_bound each: ties go behind the earlier
//     layers, the order of a stable sort of the concatenation) and mark their output slots in a bit mask (ds_or);
//   * every output slot then knows from the mask alone what it receives: bit set -> the next sample of the new layer,
//     clear -> list element (slot - set bits below it); the prefix count is s_bcnt1 + v_mbcnt on the mask words, no scan.
//     The list is rewritten in place from the top block down (a list element only ever moves up).
//   Search steps per ray: S log2(m) per inserted layer instead of S (l-1) log2(S) per layer -- 2.7 x fewer at l = 3,
//   10 x at l = 9 -- and the LDS footprint is 2.9 KB (3 x 128) / 11.4 KB (9 x 192) per wave.
//   * the merged composite gathers each sample's float4 from global memory by source index (the rows were read by this
//     wave a moment ago: L2 / L1 hits) and re-applies the layer's density edits per lane (edit_sample with the layer's
//     two switches from the LDS table of build_edit_table).
// Same merged order, same lanes, same arithmetic as composite_kernel: bit-identical outputs (the `order` parity call
// still takes composite_kernel; tests/test_gpu_ops.py::test_composite_production_shortcuts_are_bitwise_neutral compares
// the two).  A layer that is neither ascending nor strictly descending sends the ray to a brute-force rank (tests only).
// ---------------------------------------------------------------------------------------------
__host__ __device__ __forceinline__ int64_t merge_lds_per_wave(int l, int S) {   // l: layers the merged list holds
    const int64_t LS = (int64_t)l * S, SP = (S + 63) / 64 * 64, words = (LS + 63) / 64 * 2;
    return ((4 * LS + 4 * SP + 4 * words + 2 * LS + 15) / 16) * 16;
}

// occupancy target of composite_merge_kernel (waves per SIMD -> 512 / n registers); the host sizes the LDS tiers with it
__host__ __device__ constexpr int merge_waves_per_simd(int maxb, bool full) { return !full ? 5 : maxb > 2 ? 6 : 7; }

template <int MAXB>
struct LayerRegs {
    float tk[MAXB];
    float4 rw[MAXB];
};

// FULL: S == 64 * MAXB (64 / 128 / 192 samples per layer: every BASELINE configuration) -- no lane is ever idle, the
// `k < S` predicates and their exec-mask bookkeeping disappear.
// MW: a.merged_weights is written too.  The stores are compiled out of the instantiation every render without the pass runs,
// so its registers and occupancy are what they were; with them the scatter's address takes one wave per SIMD where the
// budget was tight.
template <int MAXB, bool FULL, bool MW>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(merge_waves_per_simd(MAXB, FULL) - (MW && FULL ? 1 : 0), 8))) composite_merge_kernel(CompositeArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    const unsigned lane = threadIdx.x & 63u;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned S = FULL ? 64u * MAXB : (unsigned)a.S, L = (unsigned)a.l, LS = L * S;
    const unsigned LC = (unsigned)a.lds_layers * S;   // capacity of the merged list (samples)
    float* tab = reinterpret_cast<float*>(smem_raw);
    const EvalBits ev = eval_bits<true>(a.p, a.l);
    build_edit_table(tab, a.p, a.l);
    __syncthreads();
    unsigned char* mine = smem_raw + EDIT_TAB_BYTES + (size_t)wave * merge_lds_per_wave(a.lds_layers, (int)S);
    float* mkey = reinterpret_cast<float*>(mine);            // [LC] merged depths, ascending
    float* ckey = mkey + LC;                                  // [SP] the layer being inserted, ascending (ckey = mkey + LC is used below)
    unsigned* bits = reinterpret_cast<unsigned*>(ckey + (S + 63u) / 64u * 64u);   // [2 ceil(LC / 64)] output slots of the new layer
    unsigned short* mpay = reinterpret_cast<unsigned short*>(bits + (LC + 63u) / 64u * 2u);   // [LC] source sample of a list entry
    const unsigned lmask = L >= 32u ? ~0u : (1u << L) - 1u;
    const float invS = 1.f / (float)S, nearv = a.p.near, border = a.p.border;
    const bool fine = a.p.fine != 0, activated = a.p.rgb_activated != 0;
    auto ok_lane = [&](int b) -> bool { return FULL || (unsigned)b * 64u + lane < S; };

    // A wave takes the rays wave_id + k * (number of waves), k = 0, 1, ... (neighbouring rays -- same performers, same cost --
    // go to different waves), GR of them at a time: one round trip fetches the `handled` bytes and hit masks of the whole
    // group (lane i < GR: the group's ray i; its mask packed into one word), one group ahead of the one being worked on.
    // The rays composite_single_kernel has finished (about 60 % of a view) then cost nothing here -- taken one at a time,
    // every one of them is a dependent HBM round trip with nothing behind it.
    constexpr unsigned GR = 16;
    const int64_t nwaves = (int64_t)gridDim.x * a.waves_per_block, wave_id = (int64_t)blockIdx.x * a.waves_per_block + wave;
    auto group_flags = [&](int64_t k0, unsigned& mk) -> int {
        int hnd = 1;
        mk = 0u;
        const int64_t ray = wave_id + (k0 + lane) * nwaves;
        if (lane < GR && ray < a.n) {
            hnd = a.handled ? (int)a.handled[ray] : 0;
            if (a.mask) {
#pragma unroll
                for (int i = 0; i < STNERF_MAX_LAYERS; ++i)
                    if (i < a.l) {   // bit i: hit (the reference's ray_mask); bit 16 + i: the sampler's "missed" hint
                        const unsigned mv = a.mask[ray * a.l + i];
                        mk |= (mv & 1u) << i | (mv >> 1 & 1u) << (16 + i);
                    }
            }
        }
        return hnd;
    };
    using Regs = LayerRegs<MAXB>;
    unsigned mk_next = 0u;
    int hnd_next = group_flags(0, mk_next);
    CP_DECL
    for (int64_t k0 = 0; wave_id + k0 * nwaves < a.n; k0 += GR) {
      const unsigned mk = mk_next;
      unsigned todo_rays = (unsigned)__ballot(hnd_next == 0);
      hnd_next = group_flags(k0 + GR, mk_next);
      CP(0);
      while (todo_rays) {  // (wave-uniform; no workgroup barrier inside the loops)
        const int jr = __ffs(todo_rays) - 1;
        todo_rays &= todo_rays - 1u;
        const int64_t ray = wave_id + (k0 + jr) * nwaves;
        const unsigned mask_word = (unsigned)__builtin_amdgcn_readlane((int)mk, jr);
        const unsigned mask_bits = mask_word & 0xffffu, miss_bits = mask_word >> 16;
        const unsigned have_m = have_layers(ev, a.mask != nullptr, mask_bits) & lmask;
        const float* __restrict__ tsrc = a.t + ray * LS;
        const float4* __restrict__ rsrc = a.raw + ray * LS;
        // (idle lanes of a ragged last block read the layer's last sample: no branch around the loads, nothing uses the value)
        auto sample_of = [&](int b) -> unsigned { const unsigned k = (unsigned)b * 64u + lane; return FULL ? k : (k < S ? k : S - 1u); };
        auto load = [&](Regs& r, unsigned layer) {   // raw is read for a layer without output as well (zeroed when used)
#pragma unroll
            for (int b = 0; b < MAXB; ++b) {
                r.tk[b] = tsrc[layer * S + sample_of(b)];
                r.rw[b] = rsrc[layer * S + sample_of(b)];
            }
        };
        // the first layer with network output is (almost always) the first live layer: its loads go out together with the
        // depth checks below instead of one round trip behind them
        const int first_have = have_m ? __ffs(have_m) - 1 : -1;
        Regs cur;
        load(cur, first_have >= 0 ? (unsigned)first_have : 0u);
        // ---- which layers take part: those with network output, and those without whose depths are real (a hidden layer,
        // a grazing hit: they shape their neighbours' deltas; see composite_kernel).  Eight layers' depths per round trip.
        unsigned live = have_m;
        constexpr int CB = 8;
        for (unsigned cand = ~have_m & ~miss_bits & lmask; cand;) {   // (layers the sampler flagged as missed are not even looked at)
            int ly[CB];
            float v[CB][MAXB];
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                ly[j] = cand ? __ffs(cand) - 1 : -1;
                cand &= cand - 1u;   // (0 stays 0)
#pragma unroll
                for (int b = 0; b < MAXB; ++b) v[j][b] = ly[j] >= 0 ? tsrc[(unsigned)ly[j] * S + sample_of(b)] : -1000.f;
            }
#pragma unroll
            for (int j = 0; j < CB; ++j) {
                bool missed = true;
#pragma unroll
                for (int b = 0; b < MAXB; ++b) missed = missed && v[j][b] == -1000.f;
                if (ly[j] >= 0 && !__all(missed)) live |= 1u << ly[j];
            }
        }
        const unsigned nlive = (unsigned)__popc(live);
        CP(1);
        if (nlive * S > LC) continue;   // more live layers than this launch's list holds: the next launch takes the ray
        // ---- the layers the ray misses: zero weights and outputs
        for (unsigned dead = ~live & lmask; dead; dead &= dead - 1u) {
            const unsigned other = (unsigned)__ffs(dead) - 1u;
            if (a.weights) {
                float* wz = a.weights + (ray * L + other) * S;
#pragma unroll
                for (int b = 0; b < MAXB; ++b)
                    if (ok_lane(b)) wz[(unsigned)b * 64u + lane] = 0.f;
            }
            if (MW) {
                float* mz = a.merged_weights + (ray * L + other) * S;
#pragma unroll
                for (int b = 0; b < MAXB; ++b)
                    if (ok_lane(b)) mz[(unsigned)b * 64u + lane] = 0.f;
            }
            if (a.layer_out && lane < 5u) a.layer_out[(ray * L + other) * 5 + lane] = 0.f;
        }
        if (a.handled && lane == 0u) a.handled[ray] = 1;
        if (nlive == 0u) {
            if (a.mixed_out && lane < 5u) a.mixed_out[ray * 5 + lane] = 0.f;
            continue;
        }
        unsigned m = 0;                    // length of the merged list
        bool any_unsorted = false, merged_done = false;
        unsigned todo = live;
        int layer = __ffs(todo) - 1;
        todo &= todo - 1u;
        if (layer != first_have) load(cur, (unsigned)layer);   // (a layer without output in front of it takes part: hidden / grazing)
        Regs nxt = cur;
        while (layer >= 0) {
            const int nlayer = todo ? __ffs(todo) - 1 : -1;
            todo &= todo - 1u;
            if (nlayer >= 0) load(nxt, (unsigned)nlayer);
            __builtin_amdgcn_sched_barrier(0);  // the next layer's loads go out ahead of this layer's arithmetic
            // ---- density edits (a10)
            {
                const bool have = (have_m >> layer & 1u) != 0;
                const bool cut_neg = !fine && a.p.cut_negative_t && layer > 0, cut_near = !fine && layer == 0;
                const float thr = tab[layer], sscale = tab[16 + layer];
#pragma unroll
                for (int b = 0; b < MAXB; ++b)   // (without output: zero tensors (:398-399); sigma = 0 makes the colour moot)
                    cur.rw[b] = have ? edit_sample(cur.rw[b], cur.tk[b], cut_neg, thr, sscale, cut_near, nearv, activated) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
            // ---- successor depths inside the layer (lane + 1; lane 63 takes the next block's lane 0) and the list's direction
            float tn[MAXB];
            bool desc = false, not_desc = false;
#pragma unroll
            for (int b = 0; b < MAXB; ++b) {
                float first_next = 0.f;
                if (b + 1 < MAXB) first_next = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cur.tk[b + 1 < MAXB ? b + 1 : b])));
                const float shifted = dpp_move<DPP_WAVE_SHL1>(0.f, cur.tk[b]);
                tn[b] = lane == 63u ? first_next : shifted;
                const bool has_next = FULL ? (b + 1 < MAXB || lane != 63u) : ((unsigned)b * 64u + lane + 1u < S);
                desc = desc || (has_next && tn[b] < cur.tk[b]);
                not_desc = not_desc || (has_next && !(tn[b] < cur.tk[b]));
            }
            const bool some_desc = __any(desc), some_asc = __any(not_desc);
            const bool rev = some_desc && !some_asc, unsorted = some_desc && some_asc;
            // ---- the layer's own composite (:435-444 / :598-603), from registers
            float* wdst = a.weights ? a.weights + (ray * L + (unsigned)layer) * S : nullptr;
            const bool single_asc = a.mixed_out && nlive == 1u && !some_desc;
            {
                float* mdst = nullptr;    // the layer's row of merged_weights
                bool mw_first = false;    // ... which the first pass writes: the mix is the layer's composite
                if (MW) {
                    mdst = a.merged_weights + (ray * L + (unsigned)layer) * S;
                    mw_first = single_asc && !(fine && __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cur.tk[0]))) < nearv);
                }
                CompositeAcc A;
                composite_regs<MAXB, FULL>(A, S, border, lane, cur.tk, tn, cur.rw, false, 0.f, wdst, MW && mw_first ? mdst : nullptr);
                const float t_first = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(cur.tk[0])));
                // one live, ascending layer: the union IS the layer; the mix differs from its composite only by the fine
                // stage's `t < near` cut (:605)
                const bool mix_is_layer = single_asc && !(fine && t_first < nearv);
                composite_store5(A, a.layer_out ? a.layer_out + (ray * L + (unsigned)layer) * 5 : nullptr,
                                 mix_is_layer ? a.mixed_out + ray * 5 : nullptr, lane);
                if (single_asc && !mix_is_layer) {
                    CompositeAcc M;
                    composite_regs<MAXB, FULL>(M, S, border, lane, cur.tk, tn, cur.rw, true, nearv, MW ? mdst : nullptr);
                    composite_store5(M, a.mixed_out + ray * 5, nullptr, lane);
                }
                merged_done = single_asc;
            }
            CP(2);
            if (a.mixed_out && !single_asc) {
                if (unsorted) {
                    any_unsorted = true;
                } else if (!any_unsorted) {
                    // ---- insert the layer into the merged list (:425-429 / :587-592)
                    const unsigned base_e = (unsigned)layer * S;
                    if (m == 0u) {
#pragma unroll
                        for (int b = 0; b < MAXB; ++b) {
                            const unsigned k = (unsigned)b * 64u + lane;
                            if (ok_lane(b)) {
                                const unsigned r = rev ? S - 1u - k : k;
                                mkey[r] = cur.tk[b];
                                mpay[r] = (unsigned short)(base_e + k);
                            }
                        }
                    } else {
                        const unsigned tot = m + S, nblk = (tot + 63u) >> 6;
                        for (unsigned w = lane; w < 2u * nblk; w += 64u) bits[w] = 0u;
#pragma unroll
                        for (int b = 0; b < MAXB; ++b) {
                            const unsigned k = (unsigned)b * 64u + lane;
                            if (ok_lane(b)) ckey[rev ? S - 1u - k : k] = cur.tk[b];
                        }
                        wave_sync();
                        // #{list entries <= v} for the MAXB samples of a lane in lockstep (independent LDS chains): a lower
                        // bound whose interval LENGTH is the same for every lane (a scalar), so that a probe is an add, a
                        // ds_read, a compare and a select -- no clamp against the list's end, no per-lane bound test.
                        // `at[b]` points at the entry in front of the interval (never read before it has moved).
                        const float* at[MAXB];
#pragma unroll
                        for (int b = 0; b < MAXB; ++b) at[b] = mkey - 1;
                        for (unsigned len = (unsigned)__builtin_amdgcn_readfirstlane((int)m); len > 1u;) {
                            const unsigned half = (unsigned)__builtin_amdgcn_readfirstlane((int)(len >> 1));
#pragma unroll
                            for (int b = 0; b < MAXB; ++b) {
                                const float* probe = at[b] + half;
                                at[b] = (*probe <= cur.tk[b]) ? probe : at[b];
                            }
                            len = (unsigned)__builtin_amdgcn_readfirstlane((int)(len - half));
                        }
                        unsigned pos[MAXB];
#pragma unroll
                        for (int b = 0; b < MAXB; ++b)   // (32-bit LDS addresses: `at` is one entry in front of the interval)
                            pos[b] = (((unsigned)(uintptr_t)at[b] - (unsigned)(uintptr_t)mkey + 4u) >> 2) + ((at[b][1] <= cur.tk[b]) ? 1u : 0u);
#pragma unroll
                        for (int b = 0; b < MAXB; ++b) {
                            const unsigned k = (unsigned)b * 64u + lane;
                            if (ok_lane(b)) {
                                const unsigned p = (rev ? S - 1u - k : k) + pos[b];
                                __hip_atomic_fetch_or(&bits[p >> 5], 1u << (p & 31u), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                            }
                        }
                        wave_sync();
                        unsigned above = 0;  // samples of the new layer in the blocks already written (higher slots)
                        for (int B = (int)nblk - 1; B >= 0; --B) {
                            const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)bits[2 * B]);
                            const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)bits[2 * B + 1]);
                            const unsigned cnt_in = (unsigned)(__popc(lo) + __popc(hi));
                            const unsigned below = S - above - cnt_in + __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));
                            const bool is_new = ((lane < 32u ? lo >> lane : hi >> (lane - 32u)) & 1u) != 0u;
                            const unsigned p = (unsigned)B * 64u + lane;
                            if (p < tot) {
                                const unsigned j = p - below;                        // list entries in front of slot p
                                const float key = mkey[is_new ? LC + below : j];     // (ckey = mkey + LC)
                                const unsigned short old = mpay[j];
                                const unsigned short pay = is_new ? (unsigned short)(base_e + (rev ? S - 1u - below : below)) : old;
                                mkey[p] = key;
                                mpay[p] = pay;
                            }
                            above += cnt_in;
                        }
                    }
                    m = (unsigned)__builtin_amdgcn_readfirstlane((int)(m + S));
                    wave_sync();
                }
            }
            CP(3);
            cur = nxt;
            layer = nlayer;
        }
        if (!a.mixed_out || merged_done) continue;
        if (any_unsorted) {  // general rank over the live samples: (depth, source index) lexicographic, O(n^2) (tests only)
            for (unsigned la_m = live; la_m; la_m &= la_m - 1u) {
                const unsigned la = (unsigned)__ffs(la_m) - 1u;
                for (unsigned k = lane; k < S; k += 64u) {
                    const unsigned e = la * S + k;
                    const float v = tsrc[e];
                    unsigned rank = 0;
                    for (unsigned lb_m = live; lb_m; lb_m &= lb_m - 1u) {
                        const unsigned lb = (unsigned)__ffs(lb_m) - 1u;
                        for (unsigned x = 0; x < S; ++x) {
                            const float xv = tsrc[lb * S + x];
                            rank += (xv < v || (xv == v && lb * S + x < e)) ? 1u : 0u;
                        }
                    }
                    mkey[rank] = v;
                    mpay[rank] = (unsigned short)e;
                }
            }
            m = nlive * S;
            wave_sync();
        }
        // ---- merged composite (:448 / :605-606): two blocks of the list per round trip of the float4 gather (four cost 13 registers = one wave per SIMD)
        {
            constexpr int G = 2;
            const bool cut_neg_on = !fine && a.p.cut_negative_t;
            CompositeAcc A;
            for (unsigned base = 0; base < m; base += 64u * G) {
                float key[G], keyn[G];
                float4 rw[G];
                unsigned src[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const unsigned mm = base + (unsigned)g * 64u + lane;
                    const unsigned mc = FULL ? mm : (mm < m ? mm : m - 1u);
                    if (base + (unsigned)g * 64u < m) {  // (uniform)
                        key[g] = mkey[mc];
                        keyn[g] = mkey[mc + 1u];          // (one past the list's end for its last sample: inside the LDS window, unused)
                        src[g] = mpay[mc];
                        rw[g] = rsrc[src[g]];
                    }
                }
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (base + (unsigned)g * 64u < m) {  // (uniform)
                        const unsigned mm = base + (unsigned)g * 64u + lane;
                        const bool ok = FULL || mm < m;
                        const unsigned ly = (unsigned)(((float)src[g] + 0.5f) * invS);
                        const float tk = key[g];
                        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                        if (have_m >> ly & 1u) v = edit_sample(rw[g], tk, cut_neg_on && ly > 0u, tab[ly], tab[16 + ly], !fine && ly == 0u, nearv, activated);
                        if (fine && tk < nearv) v.w = 0.f;                        // :605
                        const float delta = (mm + 1u < m) ? keyn[g] - tk : border;
                        const float w = composite_block<FULL>(A, v.w, delta, v.x, v.y, v.z, tk, ok);
                        if (MW && ok) a.merged_weights[ray * LS + src[g]] = w;   // (scattered: back to the source index)
                    }
                }
            }
            composite_store5(A, a.mixed_out + ray * 5, nullptr, lane);
        }
        CP(4);
        wave_sync();
      }
    }
    CP_FLUSH;
}

// (the instantiations without the merged weights first: they are the ones a render runs, and the ones the build's resource
// report is read for)
template __global__ void composite_merge_kernel<1, true, false>(CompositeArgs);
template __global__ void composite_merge_kernel<1, false, false>(CompositeArgs);
template __global__ void composite_merge_kernel<2, true, false>(CompositeArgs);
template __global__ void composite_merge_kernel<2, false, false>(CompositeArgs);
template __global__ void composite_merge_kernel<3, true, false>(CompositeArgs);
template __global__ void composite_merge_kernel<3, false, false>(CompositeArgs);

// ---------------------------------------------------------------------------------------------
// In-scene layer passes: layer i's share of the MIXED composite, scene_out[ray][i] = sum_k wM[i][k] {r, g, b, t, 1} with wM
// the merged weights the compositor kernels above left at the samples' source indices.  sum_i scene_out[i] is mixed_out up to
// the order of the fp32 sums.  One wave per ray; HBM-bound, 4 + 4 + 16 B per sample (density is loaded with the colour, not
// used).  The colour goes through edit_sample, whose switches are off here: sigmoid(rgb) unless the caller's is activated.
// A layer without network output on the ray (hidden, missed, a grazing hit) composited zero tensors: five exact zeros.
// ---------------------------------------------------------------------------------------------
struct LayerSceneArgs {
    const float* t;
    const float4* raw;
    const uint8_t* mask;
    const float* merged_weights;
    int64_t n;
    int l, S;
    stnerf_composite_params p;
    float* scene_out;
};

__global__ void __launch_bounds__(256) layer_scene_kernel(LayerSceneArgs a) {
    const unsigned lane = threadIdx.x & 63u;
    const int64_t stride = (int64_t)gridDim.x * (blockDim.x >> 6);
    const int64_t first = (int64_t)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t LS = (int64_t)a.l * a.S;
    const EvalBits ev = eval_bits<false>(a.p, a.l);
    const bool activated = a.p.rgb_activated != 0;
    for (int64_t ray = first; ray < a.n; ray += stride) {
        const int mv = (a.mask && (int)lane < a.l) ? (int)a.mask[ray * a.l + lane] : 0;
        const unsigned have_m = have_layers(ev, a.mask != nullptr, (unsigned)__ballot((mv & 1) != 0));
        for (int layer = 0; layer < a.l; ++layer) {
            float* dst = a.scene_out + (ray * a.l + layer) * 5;
            if (!(have_m >> layer & 1u)) {   // (uniform)
                if (lane < 5u) dst[lane] = 0.f;
                continue;
            }
            const float* tl = a.t + ray * LS + (int64_t)layer * a.S;
            const float* wl = a.merged_weights + ray * LS + (int64_t)layer * a.S;
            const float4* rl = a.raw + ray * LS + (int64_t)layer * a.S;
            CompositeAcc A;
            // every load of the layer (three blocks at a time) is issued before the first one is consumed
            constexpr int SB = 3;
            for (int k0 = 0; k0 < a.S; k0 += 64 * SB) {
                float tv[SB], wv[SB];
                float4 rv[SB];
#pragma unroll
                for (int b = 0; b < SB; ++b) {
                    const int k = k0 + b * 64 + (int)lane;
                    tv[b] = wv[b] = 0.f;
                    rv[b] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < a.S) {
                        wv[b] = wl[k];
                        tv[b] = tl[k];
                        rv[b] = rl[k];
                    }
                }
#pragma unroll
                for (int b = 0; b < SB; ++b) {
                    if (k0 + b * 64 + (int)lane < a.S) {
                        const float4 c = edit_sample(rv[b], tv[b], false, -INFINITY, 1.f, false, 0.f, activated);
                        A.cr += wv[b] * c.x;
                        A.cg += wv[b] * c.y;
                        A.cb += wv[b] * c.z;
                        A.cd += wv[b] * tv[b];
                        A.ca += wv[b];
                    }
                }
            }
            composite_store5(A, dst, nullptr, lane);
        }
    }
}

}  // namespace stnerf

using namespace stnerf;

#ifdef STNERF_COMP_PROF
extern "C" int stnerf_debug_composite_phases(unsigned long long* host8, int reset) {
    if (hipMemcpyFromSymbol(host8, HIP_SYMBOL(g_cphase), sizeof(unsigned long long) * 8) != hipSuccess) return STNERF_ELAUNCH;
    if (reset) {
        unsigned long long z[8] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_cphase), z, sizeof(z)) != hipSuccess) return STNERF_ELAUNCH;
    }
    return STNERF_OK;
}
#endif

extern "C" int stnerf_gen_weight(const float* sigma, const float* delta, int64_t n, int S, float* weights,
                                 stnerf_stream_t stream) {
    STNERF_REQUIRE(sigma && delta && weights, "gen_weight: null pointer");
    STNERF_REQUIRE(n >= 0 && S >= 1, "gen_weight: bad shape");
    if (n == 0) return STNERF_OK;
    hipLaunchKernelGGL(gen_weight_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, as_stream(stream), sigma, delta, n,
                       S, weights);
    STNERF_CHECK_LAUNCH("gen_weight");
    return STNERF_OK;
}

// Development switch: STNERF_COMPOSITE_KERNEL=staged sends every call to the LDS-staged kernel (A/B timing, bitwise checks).
static bool legacy_composite() {
    static const bool v = [] {
        const char* e = getenv("STNERF_COMPOSITE_KERNEL");
        return e && !strcmp(e, "staged");
    }();
    return v;
}

// Which kernels a stnerf_composite call launches, and with how much LDS (host arithmetic only; also exported as
// stnerf_composite_plan so that the sizing is testable without a GPU).
struct CompositePlan {
    int staged;      // 1: the LDS-staged kernel alone (`order` output, more than 192 samples per layer, development switch)
    int single;      // single-layer pre-pass: 0 none, 1 composite_single_kernel<2, 6>, 2 composite_single_kernel<3, 24>
    int tiers;       // launches of composite_merge_kernel: 1, or 2 when a list of all l layers would cost occupancy
    int cap;         // layers the first launch's merged list holds (= l with one launch)
    int clear;       // 1: scratch is cleared first (two launches, no pre-pass to write it)
    int wpb[2];      // waves per workgroup of the launch(es) (for the staged kernel: [0])
    int64_t lds[2];  // dynamic LDS bytes per workgroup
    int64_t need;    // LDS bytes per wave of the launch that needs most
};
constexpr int64_t COMPOSITE_LDS_BUDGET = 150 * 1024;   // of the CU's 160 KiB: the rest stays with the kernels' static LDS
constexpr int MERGE_MAXB = 3;

static bool plan_composite(int l, int S, bool scratch, bool order, bool any_output, bool staged_switch, CompositePlan& p) {
    p = CompositePlan{};
    const int nblk = (S + 63) / 64;
    if (order || nblk > MERGE_MAXB || staged_switch) {
        p.staged = 1;
        p.need = (((int64_t)l * S * 22 + 15) / 16) * 16;
        p.wpb[0] = (int)(COMPOSITE_LDS_BUDGET / p.need);
        if (p.wpb[0] > 4) p.wpb[0] = 4;
        p.lds[0] = p.need * p.wpb[0];
        return p.wpb[0] >= 1;
    }
    if (scratch && any_output) p.single = (nblk <= 2 && (l - 1) * nblk <= 6) ? 1 : ((l - 1) * nblk <= 24) ? 2 : 0;
    // The merged list lives in LDS, 6 B per sample and layer: 11.4 KB per wave at 9 x 192 samples -- three waves per SIMD,
    // where the registers allow six.  Few rays of such a scene cross every box, so with scratch the rays are served in two
    // launches: first with lists of as many layers as full occupancy leaves room for (a ray with more live layers is left
    // unmarked), then the rest with lists of l layers.
    const bool full = S == 64 * nblk;
    const int waves_per_simd = merge_waves_per_simd(nblk, full);   // (the kernels' amdgpu_waves_per_eu)
    int cap = l;
    while (cap > 2 && EDIT_TAB_BYTES + 4 * merge_lds_per_wave(cap, S) > COMPOSITE_LDS_BUDGET / waves_per_simd) --cap;
    const bool two = cap < l && scratch;
    p.tiers = two ? 2 : 1;
    p.cap = two ? cap : l;
    p.clear = two && !p.single;
    for (int tier = 0; tier < p.tiers; ++tier) {
        const int64_t per_wave = merge_lds_per_wave(tier == p.tiers - 1 ? l : cap, S);
        int wpb = (int)((COMPOSITE_LDS_BUDGET - EDIT_TAB_BYTES) / per_wave);
        if (wpb > 4) wpb = 4;
        p.wpb[tier] = wpb;
        p.lds[tier] = EDIT_TAB_BYTES + per_wave * wpb;
        p.need = per_wave;
        if (wpb < 1) return false;
    }
    return true;
}

extern "C" int stnerf_composite_plan(int l, int S, int with_scratch, int with_order, int64_t* plan) {
    STNERF_REQUIRE(plan, "composite_plan: null pointer");
    STNERF_REQUIRE(l >= 1 && l <= STNERF_MAX_LAYERS && S >= 1 && (int64_t)l * S <= 65535, "composite_plan: bad shape l=%d S=%d", l, S);
    CompositePlan p;
    const bool ok = plan_composite(l, S, with_scratch != 0, with_order != 0, true, false, p);
    const int64_t v[9] = {p.staged, p.single, p.tiers, p.cap, p.clear, p.wpb[0], p.lds[0], p.tiers == 2 ? p.wpb[1] : 0, p.tiers == 2 ? p.lds[1] : 0};
    for (int i = 0; i < 9; ++i) plan[i] = v[i];
    STNERF_REQUIRE(ok, "composite: %d samples per ray need %lld B of LDS per wave, more than the %lld B this kernel may use", l * S,
                   (long long)p.need, (long long)COMPOSITE_LDS_BUDGET);
    return STNERF_OK;
}

extern "C" int stnerf_composite(const float* t, const float* raw, const uint8_t* mask, int64_t n, int l, int S,
                                const stnerf_composite_params* params_host, float* layer_out, float* mixed_out,
                                float* weights, int32_t* order, uint8_t* scratch, stnerf_stream_t stream) {
    return stnerf_composite_scene(t, raw, mask, n, l, S, params_host, layer_out, mixed_out, weights, order, scratch, nullptr, nullptr,
                                  stream);
}

// layer_scene_kernel over the rays of a finished composite (merged_weights written by it on the same stream)
static int launch_layer_scene(const float* t, const float* raw, const uint8_t* mask, int64_t n, int l, int S,
                              const stnerf_composite_params& p, const float* merged_weights, float* scene_out, hipStream_t stream) {
    LayerSceneArgs a{t, reinterpret_cast<const float4*>(raw), mask, merged_weights, n, l, S, p, scene_out};
    int64_t blocks = (n + 3) / 4;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(layer_scene_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, a);
    STNERF_CHECK_LAUNCH("composite (layer passes)");
    return STNERF_OK;
}

extern "C" int stnerf_composite_scene(const float* t, const float* raw, const uint8_t* mask, int64_t n, int l, int S,
                                      const stnerf_composite_params* params_host, float* layer_out, float* mixed_out,
                                      float* weights, int32_t* order, uint8_t* scratch, float* merged_weights, float* scene_out,
                                      stnerf_stream_t stream) {
    STNERF_REQUIRE(t && raw && params_host, "composite: null pointer");
    STNERF_REQUIRE(!scene_out || merged_weights, "composite: scene_out needs merged_weights (the pass is a sum over them)");
    STNERF_REQUIRE(!merged_weights || mixed_out, "composite: merged_weights needs mixed_out (they are the merged composite's weights)");
    STNERF_REQUIRE(n >= 0 && l >= 1 && l <= STNERF_MAX_LAYERS && S >= 1, "composite: bad shape n=%lld l=%d S=%d",
                   (long long)n, l, S);
    STNERF_REQUIRE(((uintptr_t)raw & 15) == 0, "composite: raw must be 16-byte aligned");
    if (n == 0) return STNERF_OK;
    STNERF_REQUIRE((int64_t)l * S <= 65535, "composite: more than 65535 samples per ray");
    CompositePlan plan;
    const bool fits = plan_composite(l, S, scratch != nullptr, order != nullptr, layer_out || mixed_out || weights, legacy_composite(), plan);
    STNERF_REQUIRE(fits, "composite: %d samples per ray need %lld B of LDS per wave, more than the %lld B this kernel may use", l * S,
                   (long long)plan.need, (long long)COMPOSITE_LDS_BUDGET);
    LaunchTimer timer(PROF_COMPOSITE, 0, n, S,
                      20ll * l * S + l + 20ll * (l + 1) + (weights ? 4ll * l * S : 0) + (order ? 4ll * l * S : 0) +
                          (merged_weights ? 4ll * l * S : 0) + (scene_out ? 24ll * l * S + l + 20ll * l : 0),
                      as_stream(stream));
    const bool mw = merged_weights != nullptr;
    const int nblk = (S + 63) / 64;
    if (!plan.staged) {
        // ---- production path: rays with one live layer first when the caller lends n bytes of scratch (pipelined over
        // the rays of a wave, no LDS), the others -- or all of them -- in the register / insertion-merge kernel
        CompositeArgs a{t, reinterpret_cast<const float4*>(raw), mask, n, l, S, *params_host, layer_out, mixed_out,
                        weights, nullptr, 4, floor_pow2(S), nullptr};
        a.merged_weights = merged_weights;
        if (plan.single) {
            int64_t waves = n < 256 * 32 ? n : 256 * 32;  // 8 waves per SIMD, every wave strides over the rays
            const dim3 grid((unsigned)((waves + 3) / 4));
            a.handled = scratch;
            if (plan.single == 1) {
                if (mw) hipLaunchKernelGGL((composite_single_kernel<2, 6, true>), grid, dim3(256), 0, as_stream(stream), a);
                else hipLaunchKernelGGL((composite_single_kernel<2, 6, false>), grid, dim3(256), 0, as_stream(stream), a);
            } else {
                if (mw) hipLaunchKernelGGL((composite_single_kernel<3, 24, true>), grid, dim3(256), 0, as_stream(stream), a);
                else hipLaunchKernelGGL((composite_single_kernel<3, 24, false>), grid, dim3(256), 0, as_stream(stream), a);
            }
            STNERF_CHECK_LAUNCH("composite (single-layer rays)");
        }
        if (plan.clear) {
            if (hipMemsetAsync(scratch, 0, (size_t)n, as_stream(stream)) != hipSuccess) return STNERF_ELAUNCH;
            a.handled = scratch;
        }
        const bool full = S == 64 * nblk;
        for (int tier = 0; tier < plan.tiers; ++tier) {
            a.lds_layers = tier == plan.tiers - 1 ? l : plan.cap;
            const int wpb = plan.wpb[tier], lds = (int)plan.lds[tier];
            a.waves_per_block = wpb;
            int64_t blocks = (n + wpb - 1) / wpb;
            if (blocks > 256 * 16) blocks = 256 * 16;
            const dim3 grid((unsigned)blocks), block(wpb * 64);
            auto launch = [&](auto kernel) -> int {
                if (lds > 64 * 1024)
                    if (const int rc = reserve_dynamic_lds(reinterpret_cast<const void*>(kernel), lds, "composite")) return rc;
                hipLaunchKernelGGL(kernel, grid, block, lds, as_stream(stream), a);
                return STNERF_OK;
            };
            const int rc = mw ? (nblk == 1 ? (full ? launch(composite_merge_kernel<1, true, true>) : launch(composite_merge_kernel<1, false, true>))
                               : nblk == 2 ? (full ? launch(composite_merge_kernel<2, true, true>) : launch(composite_merge_kernel<2, false, true>))
                                           : (full ? launch(composite_merge_kernel<3, true, true>) : launch(composite_merge_kernel<3, false, true>)))
                         : nblk == 1 ? (full ? launch(composite_merge_kernel<1, true, false>) : launch(composite_merge_kernel<1, false, false>))
                         : nblk == 2 ? (full ? launch(composite_merge_kernel<2, true, false>) : launch(composite_merge_kernel<2, false, false>))
                                     : (full ? launch(composite_merge_kernel<3, true, false>) : launch(composite_merge_kernel<3, false, false>));
            if (rc) return rc;
            STNERF_CHECK_LAUNCH("composite");
        }
        return scene_out ? launch_layer_scene(t, raw, mask, n, l, S, *params_host, merged_weights, scene_out, as_stream(stream)) : STNERF_OK;
    }
    // ---- the `order` parity output and layers of more than 192 samples: the LDS-staged kernel (every ray on its own)
    const int wpb = plan.wpb[0], lds = (int)plan.lds[0];
    if (lds > 64 * 1024)
        if (const int rc = reserve_dynamic_lds(reinterpret_cast<const void*>(composite_kernel), lds, "composite")) return rc;
    CompositeArgs a{t, reinterpret_cast<const float4*>(raw), mask, n, l, S, *params_host, layer_out, mixed_out,
                    weights, order, wpb, floor_pow2(S), nullptr};
    a.merged_weights = merged_weights;
    int64_t blocks = (n + wpb - 1) / wpb;
    if (blocks > 256 * 16) blocks = 256 * 16;
    hipLaunchKernelGGL(composite_kernel, dim3((unsigned)blocks), dim3(wpb * 64), lds, as_stream(stream), a);
    STNERF_CHECK_LAUNCH("composite");
    return scene_out ? launch_layer_scene(t, raw, mask, n, l, S, *params_host, merged_weights, scene_out, as_stream(stream)) : STNERF_OK;
}
