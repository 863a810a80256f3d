// Argument block and row bookkeeping shared by the persistent stage kernels behind stnerf_mlp_stage (launched from
// stage_entry.hip): mlp_wave.hip (exact f32) and mlp_bf16x3.hip (split bf16) -- sample-split waves, activations in registers;
// their common prologue / epilogue code is mlp_wave_common.h.  (The round-2 organisation with feature-split waves and
// activations in LDS, mlp_stage.hip, was removed in round 3.)
#pragma once
#include <type_traits>

#include "mlp_common.h"

namespace stnerf {

struct StageLayer {
    const float* space;        // packed SpaceNet
    const float* motion;       // packed MotionNet or nullptr
    const int32_t* ray_list;   // compacted hit rays or nullptr (every ray)
    const int32_t* ray_count;
    const float* xyz;          // this layer's sample points (ray stride StageArgs::xyz_ray_stride)
    float* raw;                // this layer's {r,g,b,sigma} (ray stride StageArgs::raw_ray_stride)
    const float* times;        // this layer's frame-id column or nullptr
    int32_t use_time;          // the SpaceNet takes the time encoding
    int32_t motion_flags;      // STNERF_MOTION_PLAIN_TIME
    const float* raybias;      // [n_rays][128]: rgb_net.1's bias row per ray, added behind its product (mlp_raybias.hip)
};

struct StageArgs {
    StageLayer layer[STNERF_MAX_LAYERS];
    int32_t n_layers, ns;
    int64_t n_rays;
    int64_t xyz_ray_stride, raw_ray_stride, dirs_ray_stride, times_ray_stride;
    const float* dirs;
    uint32_t* queue;           // one counter, zero at launch; nullptr: workgroup b takes the items b, b + grid, ...
    int32_t sigmoid_rgb;       // store sigmoid(rgb) (layers/render_layer.py:47) instead of the raw colour output
    // development builds of mlp_wave.hip (-DSTNERF_WAVE_DEBUG): activations of queue slot 0 after stage `dbg_stage` go to
    // dbg[row][256] (tools/ab_wave.py localises a wrong layer with them); null otherwise
    float* dbg;
    int32_t dbg_stage;
};

// rows of a work list (include/stnerf.h) = hit rays x samples per ray
__device__ __forceinline__ int64_t layer_rows(const int32_t* ray_count, int64_t n_rays, int ns) {
    int64_t cnt = n_rays;
    if (ray_count) {
        const int64_t c = *ray_count;
        cnt = c < cnt ? c : cnt;
    }
    return cnt * ns;
}
__device__ __forceinline__ int64_t layer_rows(const StageLayer& ly, int64_t n_rays, int ns) { return layer_rows(ly.ray_count, n_rays, ns); }

struct RowRef {
    int64_t ray;
    int k;
    bool valid;
};
__device__ __forceinline__ RowRef locate_row(const int32_t* ray_list, int64_t row, int64_t rows, int ns) {
    RowRef r{0, 0, row < rows};
    if (r.valid) {
        const int64_t slot = row / ns;
        r.k = (int)(row - slot * ns);
        r.ray = ray_list ? (int64_t)ray_list[slot] : slot;
    }
    return r;
}

// The fractional-time lerp of the MotionNet encodings (modeling/motion_net.py:49-60); one definition so that every
// kernel evaluates the same expression.
__device__ __forceinline__ float lerp_enc(bool frac, float om, float wgt, float va, float vb) {
    return frac ? om * va + wgt * vb : va;
}

// Training: where a stage kernel's tap writes every layer's input (mlp_wave.hip: StoreTap, exact f32; mlp_bf16x3_core.h:
// BxStoreTap, split bf16).  Row r of the launch <-> row r of every matrix.
struct NoTapArgs {};
constexpr int TAP_PE = 100;   // the taps' stage id of the staged encoding
struct StoreTapArgs {
    float* buf[8];     // stage s: the input of stage1.2 .. stage2.4 (0 .. 5), of the heads / rgb_net.1 (6: 256 wide), of rgb_net.3 (7: 128)
    int32_t ld[8];     // row strides in floats (multiples of 4; 16-byte aligned bases)
    float* pe;         // PE(pos): 63 features + one zero
    int32_t ld_pe;
    uint32_t* bits;    // [8][.. bits_stride ..]: rows x 8 words per stage: the ReLU masks of stages 0 .. 7 as bit planes (see StoreTap), or null
    int64_t bits_stride;   // uint32 words between two stages' planes
};

// Row lists (include/stnerf.h: stnerf_stage_rows): the second argument of the row-list flavours of the stage
// kernels (mlp_wave_rows.hip, mlp_bf16x3_rows.hip).  Queue slot j with row_list[j] != nullptr has *row_count[j] rows, and row r
// of it is sample k = v & 255 of ray v >> 8, v = row_list[j][r]; a slot without a list has hit rays x ns rows as ever.
struct StageRowsArgs {
    const int32_t* row_list[STNERF_MAX_LAYERS];
    const int32_t* row_count[STNERF_MAX_LAYERS];
};
// rows of queue slot j: of its row list (never more than a full layer's n_rays x ns) or of its work list
template <class TapArgs>
__device__ __forceinline__ int64_t slot_rows(const StageLayer& ly, const TapArgs& targs, int j, int64_t n_rays, int ns) {
    if constexpr (std::is_same<TapArgs, StageRowsArgs>::value) {
        if (targs.row_list[j]) {
            const int64_t c = *targs.row_count[j], cap = n_rays * ns;
            return c < 0 ? 0 : (c < cap ? c : cap);
        }
    }
    return layer_rows(ly, n_rays, ns);
}

// mlp_wave.hip, mlp_wave_rows.hip
int launch_wave_stage_rows(const StageArgs& a, const StageRowsArgs& r, bool deep_rgb, int cus, hipStream_t stream);
int launch_wave_stage(const StageArgs& a, bool deep_rgb, int cus, hipStream_t stream);
int launch_wave_stage_store(const StageArgs& a, float* const (&buf)[8], const int32_t (&ld)[8], float* pe, int32_t ld_pe, uint32_t* bits,
                            int64_t bits_stride, int cus, hipStream_t stream);

}  // namespace stnerf
